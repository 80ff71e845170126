"""The event exposure on the host: the oracle against hand-computed values, the validation errors (raised before any device
work), the empty cases, and the public path -- region ranks, areas, windows, the sort, the CSR offsets and the host finish --
on a NumPy stand-in for the engine call.  No GPU needed."""
import os
import sys

import numpy as np
import pytest

import marex_amd
import marex_amd._stream as mi
import marex_amd.exposure as mx
from marex_amd.engine import HotPath
from marex_amd.exceptions import ConfigurationError, DataValidationError, ProcessingError
from marex_amd.xr_compat import DataArray

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import event_exposure_cases as xc  # noqa: E402
import event_exposure_oracle as eo  # noqa: E402
from event_exposure_host_engine import HostEngine  # noqa: E402

NAN, INF = np.nan, np.inf
F = np.float32

DTYPES = {"pair_ID": np.int64, "pair_region": np.int64, "pair_steps": np.int64, "pair_cell_steps": np.int64,
          "pair_area_steps": np.float64, "pair_cells_max": np.int64, "pair_area_max": np.float64, "pair_share_of_event": np.float64,
          "pair_region_share_max": np.float64, "pair_intensity_max": np.float32, "pair_intensity_integral": np.float64,
          "pair_intensity_mean": np.float64, "pair_invalid_cells": np.int64, "event_regions": np.int64,
          "event_main_region": np.int64, "event_outside_share": np.float64, "region_events": np.int64,
          "region_event_steps": np.int64, "region_cells": np.int64, "region_area": np.float64, "pair_record_offsets": np.int64,
          "record_cells": np.int64, "record_area": np.float64, "record_intensity_max": np.float32,
          "record_intensity_integral": np.float64, "record_intensity_mean": np.float64, "record_invalid_cells": np.int64}
DIMS = {"pair": "pair", "even": "ID", "regi": "region", "reco": "record"}


def assert_equals_oracle(ds, exp):
    want, coords = exp
    assert sorted(ds.data_vars) == sorted(want)
    for k, w in want.items():
        got = np.asarray(ds[k].values)
        assert got.dtype == w.dtype, (k, got.dtype, w.dtype)
        if k in DTYPES:
            assert got.dtype == DTYPES[k], (k, got.dtype)
        assert got.shape == w.shape, (k, got.shape, w.shape)
        assert np.array_equal(got, w, equal_nan=got.dtype.kind in "fmM"), (k, got, w)
        assert tuple(ds[k].dims) == ("pair_edge" if k == "pair_record_offsets" else DIMS[k[:4]],), (k, ds[k].dims)
    assert np.array_equal(np.asarray(ds["event_regions"].coords["ID"].values), coords["ID"])
    assert np.array_equal(np.asarray(ds["region_events"].coords["region"].values), coords["region"])


def same(a, b):
    assert list(a.data_vars) == list(b.data_vars)
    for k in a.data_vars:
        assert np.asarray(a[k].values).tobytes() == np.asarray(b[k].values).tobytes(), k
        assert np.asarray(a[k].values).dtype == np.asarray(b[k].values).dtype and tuple(a[k].dims) == tuple(b[k].dims), k


def test_oracle_on_a_hand_computed_field():
    #                 cell 0    1     2     3     4     5
    regions = np.array([10,     10,   20,   20,   -1,   30])
    x = np.array([[1,           1,    1,    0,    1,    2],
                  [0,           1,    1,    1,    2,    0],
                  [0,           0,    0,    0,    0,    0],
                  [3,           0,    1,    0,    0,    0]], np.int32)
    a = np.array([[1.0,         -2.0, NAN,  9.0,  9.0,  INF],
                  [9.0,         0.5,  -1.0, -3.0, 9.0,  9.0],
                  [9.0] * 6,
                  [2.0,         9.0,  4.0,  9.0,  9.0,  9.0]], F)
    areas = np.array([1.0, 2.0, 1.0, 0.5, 4.0, 1.0])
    rvals, rank = eo.ranks(regions)
    recs = eo.step_records(x, rank, 3, anom=a, wf=areas.astype(F))
    assert [(d["id"], d["rank"], d["t"], d["cells"], d["finite"]) for d in recs] == [
        (1, 0, 0, 2, 2), (1, 0, 1, 1, 1), (1, 1, 0, 1, 0), (1, 1, 1, 2, 2), (1, 1, 3, 1, 1), (1, 3, 0, 1, 1),
        (2, 2, 0, 1, 0), (2, 3, 1, 1, 1), (3, 0, 3, 1, 1)]
    assert [d["swa"] for d in recs[:5]] == [-3.0, 1.0, 0.0, -2.5, 4.0] and recs[2]["vmax"] is None and recs[3]["vmax"] == -1.0
    o, c = eo.exposure(x, regions, areas, a, per_timestep=True)
    assert c["region"].tolist() == [10, 20, 30] and c["ID"].tolist() == [1, 2, 3]
    assert o["pair_ID"].tolist() == [1, 1, 2, 3] and o["pair_region"].tolist() == [10, 20, 30, 10]
    assert o["pair_steps"].tolist() == [2, 3, 1, 1] and o["pair_time_start"].tolist() == [0, 0, 0, 3]
    assert o["pair_time_end"].tolist() == [1, 3, 0, 3] and o["pair_cell_steps"].tolist() == [3, 4, 1, 1]
    assert o["pair_area_steps"].tolist() == [5.0, 3.5, 1.0, 1.0] and o["pair_cells_max"].tolist() == [2, 2, 1, 1]
    assert o["pair_area_max"].tolist() == [3.0, 1.5, 1.0, 1.0] and o["pair_time_of_max_area"].tolist() == [0, 1, 0, 3]
    assert o["pair_share_of_event"].tolist() == [5.0 / 12.5, 3.5 / 12.5, 1.0 / 5.0, 1.0]
    assert o["pair_region_share_max"].tolist() == [1.0, 1.0, 1.0, 1.0 / 3.0]
    assert np.array_equal(o["pair_intensity_max"], np.array([1.0, 4.0, NAN, 2.0], F), equal_nan=True)
    assert np.array_equal(o["pair_time_of_intensity_max"], [0.0, 3.0, NAN, 3.0], equal_nan=True)
    assert o["pair_intensity_integral"].tolist() == [-2.0, 1.5, 0.0, 2.0] and o["pair_invalid_cells"].tolist() == [0, 1, 1, 0]
    assert np.array_equal(o["pair_intensity_mean"], [-2.0 / 5.0, 1.5 / 2.5, NAN, 2.0], equal_nan=True)
    assert o["event_regions"].tolist() == [2, 1, 1] and o["event_main_region"].tolist() == [10, 30, 10]
    assert o["event_outside_share"].tolist() == [4.0 / 12.5, 4.0 / 5.0, 0.0]
    assert o["region_events"].tolist() == [2, 1, 1] and o["region_event_steps"].tolist() == [3, 3, 1]
    assert o["region_cells"].tolist() == [2, 2, 1] and o["region_area"].tolist() == [3.0, 1.5, 1.0]
    assert o["pair_record_offsets"].tolist() == [0, 2, 5, 6, 7] and o["record_time"].tolist() == [0, 1, 0, 1, 3, 0, 3]
    assert o["record_area"].tolist() == [3.0, 2.0, 1.0, 1.5, 1.0, 1.0, 1.0] and o["record_invalid_cells"].tolist() == [0, 0, 1, 0, 0, 1, 0]
    # without anomalies and areas: cells
    o, _ = eo.exposure(x, regions)
    assert o["pair_area_steps"].tolist() == [3.0, 4.0, 1.0, 1.0] and "pair_intensity_max" not in o and "record_time" not in o


def _no_gpu(monkeypatch):
    import marex_amd.detect as det

    def no_gpu(*a, **k):
        raise AssertionError("the call touched the GPU engine")

    monkeypatch.setattr(det, "get_engine", no_gpu)


def test_every_refusal_comes_before_the_device(monkeypatch):
    _no_gpu(monkeypatch)
    x = np.zeros((3, 4, 5), np.int32)
    an = np.zeros((3, 4, 5), F)
    reg = np.zeros((4, 5), np.int32)
    V, Cf = DataValidationError, ConfigurationError
    tx = DataArray(x, dims=("time", "y", "x"), coords={"time": ("time", np.arange(3))})
    cases = [
        (dict(ID_field=x.astype(bool)), V, "event_exposure needs an ID field, not a mask"),
        (dict(ID_field=x.astype(np.uint8)), V, "event_exposure needs an ID field, not a mask"),
        (dict(ID_field=x.astype(F)), V, "field must be a mask .* or an integer ID field"),
        (dict(ID_field=x[0, 0]), V, r"field must be \(time, y, x\) or \(time, cells\)"),
        (dict(regions=None), V, "event_exposure needs regions"),
        (dict(regions=np.zeros((4, 5))), V, "regions must be an integer map"),
        (dict(regions=np.zeros((5, 4), np.int32)), V, "regions does not match the spatial shape"),
        (dict(regions=np.zeros(19, np.int32)), V, "regions does not match the spatial shape"),
        (dict(dat_anomaly=an[:2]), V, "ID_field and dat_anomaly differ in shape"),
        (dict(dat_anomaly=x), V, "dat_anomaly must be a floating-point field"),
        (dict(ID_field=tx, dat_anomaly=DataArray(an, dims=("time", "x", "y"))), V, "differ in shape|differ in their dimensions"),
        (dict(ID_field=DataArray(x[:, :4, :4], dims=("time", "y", "x")), regions=reg[:4, :4],
              dat_anomaly=DataArray(an[:, :4, :4], dims=("time", "x", "y"))), V, "ID_field and dat_anomaly differ in their dimensions"),
        (dict(ID_field=tx, dat_anomaly=DataArray(an, dims=("time", "y", "x"), coords={"time": ("time", np.arange(1, 4))})), V,
         "ID_field and dat_anomaly differ in their time coordinate"),
        (dict(mask=np.ones((4, 4), bool)), V, "mask does not match the spatial shape"),
        (dict(mask=np.ones((4, 5))), V, "mask must be boolean or integer"),
        (dict(cell_areas=np.ones(5)), V, "cell_areas does not match the spatial shape"),
        (dict(cell_areas=np.ones((4, 5), bool)), V, "cell_areas must be numbers"),
        (dict(cell_areas=np.array([1.0, NAN, 1.0, 1.0])), V, "cell_areas must be finite and non-negative"),
        (dict(cell_areas=np.array([1.0, -1.0, 1.0, 1.0])), V, "cell_areas must be finite and non-negative"),
        (dict(cell_areas=np.full((4, 5), INF)), V, "cell_areas must be finite and non-negative"),
        (dict(cell_areas=np.zeros((4, 5))), V, "cell_areas must have a positive, finite sum"),
    ]
    cases += [(dict(block_steps=b), Cf, "block_steps must be a positive number of timesteps, 'auto' or None")
              for b in (0, -2, 2.5, True, "all")]
    for kw, cls, msg in cases:
        args = dict(ID_field=x, regions=reg)
        args.update(kw)
        with pytest.raises(cls, match=msg):
            marex_amd.event_exposure(**args)
    big = np.zeros((1, 40000), np.int32)
    with pytest.raises(V, match="regions holds 32768 distinct regions, at most 32767 are taken"):
        marex_amd.event_exposure(big, np.minimum(np.arange(40000), 32767))
    with pytest.raises(TypeError):
        marex_amd.event_exposure(x)  # regions is required


def test_event_exposure_is_public():
    assert "event_exposure" in marex_amd.__all__ and marex_amd.event_exposure is mx.event_exposure
    assert hasattr(marex_amd.tracker, "event_exposure") and hasattr(HotPath, "event_exposure")
    from marex_amd import _lib
    from marex_amd.csrc import build

    for name in ("marex_event_exposure_count_i32", "marex_event_exposure_i32", "marex_event_exposure_layout"):
        assert name in _lib.PROTOTYPES
    assert "marex_event_exposure" in build.UNITS and "event_exposure" in marex_amd.__doc__
    build.build(verbose=False)  # hipcc cross-compiles without a GPU
    L = HotPath.exposure_layout()
    assert L["piece"] == 64 and L["wave"] % 64 == 0 and L["wg"] == 4 * L["wave"] and L["row_stride"] >= 1
    assert L["id_bits"] + L["rank_bits"] + L["step_bits"] == 64 and L["id_bits"] >= 31 and 2 ** L["rank_bits"] > 32767 + 1
    assert L == HostEngine.exposure_layout()
    assert int(HotPath.exposure_key(5, 3, 7)) == (7 << 33) | (3 << 17) | 5
    assert int(HotPath.exposure_key(2**17 - 1, 32767, 2**31 - 1)) == 2**64 - 1 - (1 << 32)
    assert HotPath.exposure_cap(0) == 64 and HotPath.exposure_cap(32) == 64 and HotPath.exposure_cap(33) == 128
    assert HotPath.exposure_cap(1000) == 2048 and HotPath.exposure_cap(1024) == 2048 and HotPath.exposure_cap(1025) == 4096
    assert HotPath.exposure_entry_bytes(False, False) == 16 and HotPath.exposure_entry_bytes(True, True) == 44
    h = HotPath.exposure_home(np.arange(1, 1000, dtype=np.uint64), 64)
    assert h.min() >= 0 and h.max() < 64 and np.unique(h).size > 48  # a hash, not the identity
    M = 2**64 - 1
    for k in (1, 12345678901234567, M):  # splitmix64's finaliser in Python integers
        z = k
        z = ((z ^ (z >> 30)) * 0xbf58476d1ce4e5b9) & M
        z = ((z ^ (z >> 27)) * 0x94d049bb133111eb) & M
        assert int(HotPath.exposure_home(np.uint64(k), 1 << 20)) == (z ^ (z >> 31)) & ((1 << 20) - 1)


@pytest.fixture
def host_engine(monkeypatch):
    import marex_amd.detect as det

    eng = HostEngine()
    monkeypatch.setattr(det, "get_engine", lambda device=0: eng)
    monkeypatch.setattr(mi, "_free_bytes", lambda e: 1 << 30)
    return eng


TIMES = np.array(["2001-12-30", "2001-12-31", "2002-01-01", "2002-02-28", "2002-03-01", "2002-06-01", "2002-12-01"],
                 dtype="datetime64[D]").astype("datetime64[ns]")


@pytest.mark.parametrize("areas", [False, True])
@pytest.mark.parametrize("anomalies", [False, True])
def test_grid_against_the_oracle_with_windows(host_engine, areas, anomalies):
    rng = np.random.default_rng(1)
    T, ny, nx = TIMES.size, 5, 8
    C = ny * nx
    x = xc.id_field(rng, T, C, n_ids=4)
    x[x == 3] = 0  # an ID that no cell holds
    x[:, 5] = np.where(x[:, 5] > 0, 4, 0)  # column 5 lies in no region: event 4 is partly outside
    anom = xc.spoil(rng, xc.dyadic_anomalies(rng, (T, C)), x)
    regions = np.repeat([[40, 40, 7, 7, 7, -1, 900, 900]], ny, axis=0)
    regions[0, :2] = -5
    valid = np.ones((ny, nx), bool)
    valid[:, 6] = False  # region 900 keeps one column
    area_y = np.array([1.0, 2.5, 4.0, 2.5, 1.0])
    dims = ("time", "lat", "lon")
    coords = {"time": ("time", TIMES), "lat": ("lat", np.linspace(-30, 30, ny)), "lon": ("lon", np.linspace(0, 70, nx))}
    f = DataArray(x.reshape(T, ny, nx), dims=dims, coords=coords)
    kw = dict(regions=DataArray(regions, dims=("lat", "lon")), mask=valid)
    okw = dict(mask=valid.reshape(-1), tv=TIMES)
    if areas:
        kw["cell_areas"], okw["cell_areas"] = area_y, np.repeat(area_y, nx)
    if anomalies:
        kw["dat_anomaly"], okw["anom"] = DataArray(anom.reshape(T, ny, nx), dims=dims, coords=coords), anom
    for per in (False, True):
        whole = marex_amd.event_exposure(f, per_timestep=per, **kw)
        assert_equals_oracle(whole, eo.exposure(x, regions.reshape(-1), per_timestep=per, **okw))
        assert host_engine.calls[-1] == ("event_exposure", 0, T, 3, areas, areas and anomalies, anomalies)
        for b in (1, 2, T, "auto"):  # window plans: the same Dataset
            host_engine.calls.clear()
            same(whole, marex_amd.event_exposure(f, per_timestep=per, block_steps=b, **kw))
            if b == 2:
                assert [c[1:3] for c in host_engine.calls] == [(s, min(2, T - s)) for s in range(0, T, 2)]
    # the sort order and the CSR offsets
    pid, preg, off = (np.asarray(whole[k].values) for k in ("pair_ID", "pair_region", "pair_record_offsets"))
    key = pid * 1000 + preg
    assert (np.diff(key) > 0).all() and off[0] == 0 and off[-1] == np.asarray(whole["record_time"].values).size
    assert np.array_equal(np.diff(off), np.asarray(whole["pair_steps"].values))
    rt = np.asarray(whole["record_time"].values)
    for k in range(pid.size):
        seg = rt[off[k]:off[k + 1]]
        assert (np.diff(seg) > np.timedelta64(0)).all() and seg[0] == np.asarray(whole["pair_time_start"].values)[k]
        assert seg[-1] == np.asarray(whole["pair_time_end"].values)[k]
    assert np.asarray(whole["region_events"].coords["region"].values).tolist() == [7, 40, 900]
    assert np.asarray(whole["event_regions"].values)[2] == 0 and np.asarray(whole["event_main_region"].values)[2] == -1
    assert np.isnan(np.asarray(whole["event_outside_share"].values)[2]) and 0 < np.asarray(whole["event_outside_share"].values)[3] < 1
    if anomalies:
        assert np.asarray(whole["pair_invalid_cells"].values).sum() > 0
    # the [y, x] areas written out, another integer type: the same bytes
    kw2 = dict(kw, cell_areas=np.repeat(area_y[:, None], nx, axis=1)) if areas else kw
    same(whole, marex_amd.event_exposure(DataArray(x.reshape(T, ny, nx).astype(np.int64), dims=dims, coords=coords), per_timestep=True, **kw2))


def test_mesh_ties_outside_events_and_untouched_regions(host_engine):
    T, C = 4, 12
    x = np.zeros((T, C), np.int32)
    regions = np.array([5, 5, 5, 3, 3, 3, -1, -1, 9, 9, 2, 2])
    x[0, 0:2] = 1
    x[1, 3:5] = 1       # event 1: two cell-steps in region 5, two in region 3 -- the tie goes to the smaller value, 3
    x[1, 6:8] = 2
    x[2, 6] = 2         # event 2: wholly outside every region
    x[0, 8] = x[1, 8:10] = x[2, 8:10] = x[3, 9] = 3  # event 3 in region 9: the area 2 at steps 1 and 2 -- the first wins
    anom = np.ones((T, C), F)
    anom[1, 8], anom[1, 9], anom[2, 8], anom[2, 9] = 2.0, 0.5, 0.5, 2.0  # the maximum 2.0 at steps 1 and 2 -- the first wins
    ds = marex_amd.event_exposure(x, regions, dat_anomaly=anom, per_timestep=True)
    assert_equals_oracle(ds, eo.exposure(x, regions, anom=anom, per_timestep=True))
    v = {k: np.asarray(ds[k].values) for k in ds.data_vars}
    assert v["pair_ID"].tolist() == [1, 1, 3] and v["pair_region"].tolist() == [3, 5, 9]
    assert v["event_main_region"].tolist() == [3, -1, 9] and v["event_regions"].tolist() == [2, 0, 1]
    assert v["event_outside_share"].tolist() == [0.0, 1.0, 0.0]
    assert v["pair_time_of_max_area"].tolist() == [1, 0, 1] and v["pair_time_of_intensity_max"].tolist() == [1, 0, 1]
    assert v["pair_cells_max"].tolist() == [2, 2, 2] and v["pair_steps"].tolist() == [1, 1, 4]
    assert np.asarray(ds["region_events"].coords["region"].values).tolist() == [2, 3, 5, 9]
    assert v["region_events"].tolist() == [0, 1, 1, 1] and v["region_event_steps"].tolist() == [0, 1, 1, 4]  # region 2: untouched
    assert v["region_cells"].tolist() == [2, 3, 3, 2] and v["pair_region_share_max"].tolist() == [2 / 3, 2 / 3, 1.0]
    for b in (1, 2, T):
        same(ds, marex_amd.event_exposure(x, regions, dat_anomaly=anom, per_timestep=True, block_steps=b))
    # areas on a mesh, mask, and the negative ID
    rng = np.random.default_rng(5)
    x = xc.blob_field(rng, 9, 61)
    regions = np.arange(61) // 8 * 3
    areas = rng.integers(1, 2**10, 61) * 2.0 ** rng.integers(0, 12, 61)
    anom = xc.spoil(rng, xc.dyadic_anomalies(rng, x.shape), x)
    m = np.arange(61) % 5 != 2
    f = DataArray(x, dims=("time", "ncells"))
    ds = marex_amd.event_exposure(f, regions, cell_areas=areas, dat_anomaly=DataArray(anom, dims=("time", "ncells")), mask=m,
                                  per_timestep=True, block_steps=4)
    assert_equals_oracle(ds, eo.exposure(x, regions, areas, anom, m, per_timestep=True))
    assert [c[1:3] for c in host_engine.calls[-3:]] == [(0, 4), (4, 4), (8, 1)]
    with pytest.raises(DataValidationError, match="Object IDs must be non-negative"):
        marex_amd.event_exposure(np.where(x == 3, -1, x), regions, block_steps=2)
    with pytest.raises(marex_amd.TrackingError, match=r"event_exposure: needs .* GB of device memory, .* GB are free"):
        marex_amd.event_exposure(np.ones((64, 1 << 25), np.int32), np.zeros(1 << 25, np.int32))


def test_the_empty_cases_need_no_device(monkeypatch):
    _no_gpu(monkeypatch)
    cases = [(np.zeros((0, 5), np.int32), np.zeros(5, int)), (np.zeros((4, 0), np.int32), np.zeros(0, int)),
             (np.zeros((0, 2, 3), np.int32), np.zeros((2, 3), int)), (np.zeros((3, 5), np.int32), np.arange(5)),  # no events
             (np.ones((3, 5), np.int32), np.full(5, -1))]  # no regions
    for x, reg in cases:
        C = int(np.prod(x.shape[1:]))
        for an in (False, True):
            ds = marex_amd.event_exposure(x, reg, dat_anomaly=np.zeros(x.shape, F) if an else None, per_timestep=True,
                                          cell_areas=np.ones(x.shape[1:]) if C else None)
            exp = eo.exposure(x.reshape(x.shape[0], C), reg.reshape(-1), anom=np.zeros((x.shape[0], C), F) if an else None,
                              per_timestep=True, cell_areas=np.ones(C) if C else None)
            if an:  # an empty time column has no missing value: it keeps the type of the axis
                assert np.asarray(ds["pair_time_of_intensity_max"].values).size == 0
                exp[0]["pair_time_of_intensity_max"] = np.asarray(ds["pair_time_of_intensity_max"].values)
            assert_equals_oracle(ds, exp)
            assert np.asarray(ds["pair_ID"].values).size == 0 and np.asarray(ds["event_regions"].values).size == 0
            assert np.asarray(ds["pair_record_offsets"].values).tolist() == [0]
    assert np.asarray(marex_amd.event_exposure(*cases[3])["region_events"].values).tolist() == [0] * 5
    assert np.asarray(marex_amd.event_exposure(*cases[4])["region_events"].values).size == 0


def test_area_steps_near_2_62_over_several_steps_against_python_integers(host_engine):
    """Fixed-point sums near 2^62 per step: the sum over the steps passes 2^63 and is still exact before its one rounding."""
    S = np.array([2**62 - 1, 2**62 - 3, 2**61 + 12345, 2**62 - 2**9 - 1, 2**53 + 1, 3], np.int64)
    for n in range(1, S.size + 1):
        got = mx._int_sum_f64(S[:n], np.zeros(1, np.int64))
        assert got.dtype == np.float64 and got[0] == float(sum(int(v) for v in S[:n])), n
    rng = np.random.default_rng(0)
    big = rng.integers(2**61, 2**62, 40, dtype=np.int64)
    starts = np.array([0, 1, 9, 33], np.int64)
    want = [float(sum(int(v) for v in big[a:b])) for a, b in zip(starts, list(starts[1:]) + [40])]
    assert mx._int_sum_f64(big, starts).tolist() == want and mx._int_sum_f64(big[:0], starts[:0]).size == 0
    # through the public path: one event over the whole mesh, areas that sum to just under 2^61 fixed-point units, six steps
    C, T = 50, 6
    a = rng.uniform(0.5, 1.0, C)
    x = np.ones((T, C), np.int32)
    ds = marex_amd.event_exposure(x, np.zeros(C, int), cell_areas=a)
    from marex_amd.regional import area_weight_table

    e, q = area_weight_table(a)
    total = sum(int(v) for v in q)
    assert total > 2**60 and T * total > 2**62
    assert np.asarray(ds["pair_area_steps"].values).tolist() == [np.ldexp(float(T * total), -e)]
    assert np.asarray(ds["pair_area_max"].values).tolist() == [np.ldexp(float(total), -e)]
    assert np.asarray(ds["pair_share_of_event"].values).tolist() == [1.0]


def test_tracker_method_takes_the_fields_from_the_datasets(monkeypatch):
    seen = {}
    monkeypatch.setattr(mx, "_event_exposure", lambda field, regions, **kw: seen.update(field=field, regions=regions, **kw) or "ds")

    class T:  # the attributes the method reads
        device, unstructured_grid, cell_area, mask = 0, True, np.arange(5.0), np.ones(5, bool)
        timedim, timecoord, time_values = "step", "date", np.array([3, 4])

    ev = marex_amd.Dataset({"ID_field": DataArray(np.zeros((2, 5), np.int32), dims=("time", "ncells")),
                            "ID": DataArray(np.arange(1, 4), dims=("ID",))})
    ex = marex_amd.Dataset({"dat_anomaly": DataArray(np.zeros((2, 5), F), dims=("time", "ncells"))})
    reg = np.zeros(5, np.int32)
    assert marex_amd.tracker.event_exposure(T(), ev, reg, ex, per_timestep=True) == "ds"
    assert seen["field"] is ev["ID_field"] and seen["dat_anomaly"] is ex["dat_anomaly"] and seen["regions"] is reg
    assert seen["cell_areas"].tolist() == [0, 1, 2, 3, 4] and seen["mask"] is T.mask and seen["per_timestep"] is True
    assert seen["n_events"] == 3 and seen["device"] == 0 and seen["time"][:2] == ("step", "date") and seen["time"][2] is T.time_values
    seen.clear()
    T.unstructured_grid, T._cell_weights = False, np.ones((1, 5), F)
    marex_amd.tracker.event_exposure(T(), ev["ID_field"], reg, block_steps=3, mask=None)
    assert seen["field"] is ev["ID_field"] and seen["dat_anomaly"] is None and seen["mask"] is None and seen["n_events"] is None
    assert seen["cell_areas"] is T._cell_weights and seen["block_steps"] == 3
    with pytest.raises(TypeError, match="unexpected keyword argument 'by'"):
        marex_amd.tracker.event_exposure(T(), ev, reg, by="year")
    bad = marex_amd.Dataset({"ID_field": ev["ID_field"], "ID": DataArray(np.array([1, 3]), dims=("ID",))})
    with pytest.raises(ProcessingError, match="the ID axis of the events Dataset is not 1 .. N"):
        marex_amd.tracker.event_exposure(T(), bad, reg)


def test_the_id_axis_of_the_events_dataset_is_checked(host_engine):
    x = np.array([[1, 2, 0, 4]], np.int32)
    with pytest.raises(ProcessingError, match="the ID field holds event 4, the events Dataset ends at 3"):
        mx._event_exposure(x, np.zeros(4, int), None, None, None, False, None, None, n_events=3)
    ds = mx._event_exposure(x, np.zeros(4, int), None, None, None, False, None, None, n_events=6, time=("step", "date", np.array([7])))
    assert np.asarray(ds["event_regions"].values).tolist() == [1, 1, 0, 1, 0, 0] and np.asarray(ds["pair_time_start"].values).tolist() == [7] * 3
