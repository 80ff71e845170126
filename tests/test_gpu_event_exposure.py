"""The event exposure on the device: ``marex_event_exposure_count_i32`` / ``marex_event_exposure_i32`` through
``HotPath.event_exposure`` against the NumPy oracle at the edges of the kernel's layout, of its key and of its table --
integers equal, float64 sums byte for byte on dyadic inputs and within the derived bound on normal ones -- the cross-checks
against the statistics that exist already, and the public path on a grid, a mesh and the trackers' own fields."""
import os
import sys

import numpy as np
import pytest

import marex_amd
from marex_amd.engine import HotPath
from marex_amd.exceptions import DataValidationError, ProcessingError
from marex_amd.xr_compat import DataArray

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import event_exposure_cases as xc  # noqa: E402
import event_exposure_oracle as eo  # noqa: E402

pytestmark = pytest.mark.gpu
F = np.float32


def layout():
    from marex_amd.csrc import build as _build

    _build.build(verbose=False)
    return HotPath.exposure_layout()


L = layout()
PIECE, WAVE, WG, STRIDE = L["piece"], L["wave"], L["wg"], L["row_stride"]
SHAPES = sorted({1, 63, 64, 65, 255, 257, WAVE - 1, WAVE, WAVE + 1, WG - 1, WG, WG + 1})


def cuts_below(C):
    return sorted({p for step in (PIECE, WAVE, WG) for p in range(step, C, step)})


def run(hot, ids, rank, R, q=None, wf=None, anom=None, cap=None, windows=None):
    """``HotPath.event_exposure`` over the windows between the cuts (one call by default), joined as the public path does."""
    import torch

    T = ids.shape[0]
    xt = torch.from_numpy(np.ascontiguousarray(ids, dtype=np.int32)).to(hot.device)
    at = None if anom is None else torch.from_numpy(np.ascontiguousarray(anom, dtype=F)).to(hot.device)
    w = sorted(set(windows or (0, T)))
    parts = [hot.event_exposure(xt[a:b], rank, R, t0=a, q=q, wf=wf, anom=None if at is None else at[a:b], cap=cap)
             for a, b in zip(w[:-1], w[1:])]
    r = {k: (None if parts[0][k] is None else np.concatenate([p[k] for p in parts])) for k in ("t", "rank", "id", "cells", "finite",
                                                                                               "area", "sums", "vmax")}
    order = np.lexsort((r["rank"], r["id"]))
    return {k: (None if v is None else v[order]) for k, v in r.items()}, parts


def check(hot, ids, rank, R, q=None, wf=None, anom=None, float_bytes=True, **kw):
    r, parts = run(hot, ids, rank, R, q, wf, anom, **kw)
    xc.assert_same(r, eo.step_records(ids, rank, R, q, wf, anom), anom is not None, float_bytes)
    return r, parts


def full_inputs(rng, T, C, blobs=True):
    ids = xc.blob_field(rng, T, C, n_ids=max(3, C // 40), width=min(C, 23)) if blobs else xc.id_field(rng, T, C)
    ids[:, 0] = 7  # a cell of an event throughout
    return ids, rng.integers(0, 2**40, C).astype(np.int64), xc.dyadic_weights(rng, C), xc.spoil(rng, xc.dyadic_anomalies(rng, (T, C)), ids)


@pytest.mark.parametrize("C", SHAPES)
def test_at_the_layout_edges(hot, C):
    rng = np.random.default_rng(C)
    rank, R = xc.region_map("edges", C, cuts_below(C)) if C > 64 else xc.region_map("mod3", C)
    for blobs in (True, False):
        ids, q, wf, anom = full_inputs(rng, 2, C, blobs)
        check(hot, ids, rank, R)
        check(hot, ids, rank, R, q=q)
        check(hot, ids, rank, R, anom=anom)
        check(hot, ids, rank, R, q=q, wf=wf, anom=anom)


@pytest.mark.parametrize("T", [1, 2, STRIDE - 1, STRIDE, STRIDE + 1])
def test_rows_around_the_row_stride(hot, T):
    rng = np.random.default_rng(100 + T)
    C = WG + 70
    ids, q, wf, anom = full_inputs(rng, T, C)
    rank, R = xc.region_map("edges", C, cuts_below(C))
    r, _ = check(hot, ids, rank, R, q=q, wf=wf, anom=anom)
    assert set(r["t"].tolist()) == set(range(T))


@pytest.mark.parametrize("name", ["one", "own", "mod3", "edges", "holes", "none"])
def test_region_maps(hot, name):
    rng = np.random.default_rng(7)
    C = WG + WAVE + 5
    ids, q, wf, anom = full_inputs(rng, 3, C)
    rank, R = xc.region_map(name, C, cuts_below(C))
    r, _ = check(hot, ids, rank, R, q=q, wf=wf, anom=anom)
    if name == "none":
        assert (r["rank"] == R).all()
    if name == "own":
        assert (r["cells"] == 1).all()  # nothing folds


@pytest.mark.parametrize("name", ["one_event", "own_ids", "alternating", "key_corners", "empty_step"])
def test_id_fields(hot, name):
    rng = np.random.default_rng(8)
    T, C = 3, WAVE + 130
    q, wf = rng.integers(0, 2**40, C).astype(np.int64), xc.dyadic_weights(rng, C)
    rank, R = xc.region_map("holes", C)
    if name == "one_event":
        ids = np.full((T, C), 5, np.int32)
    elif name == "own_ids":
        ids = (1 + np.arange(T * C, dtype=np.int32)).reshape(T, C)
    elif name == "alternating":
        ids = np.tile(1 + (np.arange(C, dtype=np.int32) % 2), (T, 1))
    elif name == "key_corners":  # IDs 1 and 2^31 - 1 under rank 0 and rank 32 766 in one field
        R = 32767
        rank = np.full(C, -1, np.int32)
        rank[0:4], rank[4:8] = 0, R - 1
        ids = np.zeros((T, C), np.int32)
        ids[:, [0, 4, 9]], ids[:, [1, 5, 10]] = 1, 2**31 - 1
    else:  # a step in which nothing is present, between steps that are
        ids = xc.blob_field(rng, T, C)
        ids[0, 3], ids[1], ids[2, 5] = 2, 0, 4
    anom = xc.spoil(rng, xc.dyadic_anomalies(rng, (T, C)), ids)
    r, _ = check(hot, ids, rank, R, q=q, wf=wf, anom=anom)
    if name == "key_corners":
        assert sorted(set(zip(r["id"].tolist(), r["rank"].tolist()))) == [(1, 0), (1, R - 1), (1, R), (2**31 - 1, 0), (2**31 - 1, R - 1),
                                                                          (2**31 - 1, R)]
    if name == "empty_step":
        assert 1 not in r["t"]


def test_the_table_at_load_one_half_at_its_end_and_too_small(hot):
    # cap = 64 with exactly 32 distinct keys
    ids = (1 + np.arange(32, dtype=np.int32)).reshape(1, 32)
    rank = np.zeros(32, np.int32)
    r, parts = check(hot, ids, rank, 1, cap=64)
    assert r["id"].size == 32 and parts[0]["cap"] == 64 and parts[0]["runs"] == 32 and HotPath.exposure_cap(32) == 64
    # keys that the hash sends to the last two entries: the probes wrap around the table's end
    T, C, cap = 4, 64, 64
    t, c, i = np.meshgrid(np.arange(T), np.arange(C), np.arange(1, 400), indexing="ij")
    home = HotPath.exposure_home(HotPath.exposure_key(t, c, i), cap)
    ids = np.zeros((T, C), np.int32)
    picked = 0
    for tt, cc, ii in zip(*(v[home >= cap - 2] for v in (t, c, i))):
        if picked < 14 and ids[tt, cc] == 0:
            ids[tt, cc] = ii
            picked += 1
    assert picked == 14
    own = np.arange(C, dtype=np.int32)
    anom = xc.dyadic_anomalies(np.random.default_rng(3), (T, C))
    r, parts = check(hot, ids, own, C, anom=anom, cap=cap)
    assert r["id"].size == 14 and (HotPath.exposure_home(HotPath.exposure_key(r["t"], r["rank"], r["id"]), cap) >= cap - 2).all()
    # a table below the number of distinct keys: a handled status, and the engine goes on
    ids = (1 + np.arange(100, dtype=np.int32)).reshape(1, 100)
    with pytest.raises(ProcessingError, match="the table of 64 entries does not hold the keys of 100 runs"):
        run(hot, ids, np.zeros(100, np.int32), 1, cap=64)
    with pytest.raises(ProcessingError, match="cap=100 is not a power of two"):
        run(hot, ids, np.zeros(100, np.int32), 1, cap=100)
    check(hot, ids, np.zeros(100, np.int32), 1)
    with pytest.raises(DataValidationError, match="Object IDs must be non-negative"):
        run(hot, np.where(ids == 50, -3, ids), np.zeros(100, np.int32), 1)
    check(hot, ids, np.zeros(100, np.int32), 1, cap=256)


def test_floats_dyadic_normal_and_invalid(hot):
    rng = np.random.default_rng(9)
    T, C = 4, WG + 300
    ids = xc.blob_field(rng, T, C, n_ids=12, width=150)
    rank, R = np.where(np.arange(C) % 7 == 3, -1, np.arange(C) // 400).astype(np.int32), (C - 1) // 400 + 1  # records across pieces
    # ordinary float32 weights and anomalies: within 2 n u sum|w a| of the exactly rounded sum
    wf = rng.uniform(0.1, 3.0, C).astype(F)
    anom = xc.spoil(rng, rng.normal(0, 2, (T, C)).astype(F), ids)
    r, _ = check(hot, ids, rank, R, wf=wf, anom=anom, float_bytes=False)
    assert (r["cells"] - r["finite"]).sum() > 0 and (r["finite"] > 64).any()
    # an all-NaN record: counted as cells and area, no sums, no maximum
    anom2 = xc.dyadic_anomalies(rng, (T, C))
    anom2[0, ids[0] == ids[0].max()] = np.nan
    anom2[1, ids[1] > 0] = np.inf
    q = rng.integers(1, 2**40, C).astype(np.int64)
    r, _ = check(hot, ids, rank, R, q=q, wf=xc.dyadic_weights(rng, C), anom=anom2)
    dead = (r["finite"] == 0)
    assert dead.any() and np.isnan(r["vmax"][dead]).all() and not r["sums"][dead].any() and (r["area"][dead] > 0).all()
    assert not np.isnan(r["vmax"][~dead]).any()
    # -0 and +0 as the only anomalies of a record: +0 is the maximum
    z = np.full((1, 8), -0.0, F)
    z[0, 3] = 0.0
    r, _ = check(hot, np.ones((1, 8), np.int32), np.zeros(8, np.int32), 1, anom=z)
    assert not np.signbit(r["vmax"][0])


def test_windows_and_residency_give_the_same_records(hot):
    import torch

    rng = np.random.default_rng(10)
    T, C = 7, 700
    ids, q, wf, anom = full_inputs(rng, T, C)
    rank, R = xc.region_map("holes", C)
    whole, _ = check(hot, ids, rank, R, q=q, wf=wf, anom=anom)
    for w in ([0, 1, 2, 3, 4, 5, 6, 7], [0, 2, 4, 6, 7], [0, 7]):
        r, _ = run(hot, ids, rank, R, q=q, wf=wf, anom=anom, windows=w)
        for k in whole:
            assert r[k].tobytes() == whole[k].tobytes(), (k, w)
    # the tables as host arrays and as device tensors
    dev = [torch.from_numpy(v).to(hot.device) for v in (rank, q, wf)]
    r, _ = run(hot, ids, dev[0], R, q=dev[1], wf=dev[2], anom=anom)
    assert all(r[k].tobytes() == whole[k].tobytes() for k in whole)
    # the public path: host and resident fields, block_steps in {1, 2, T}
    regions, areas = np.where(rank < 0, -1, rank * 10), wf.astype(np.float64)
    ds = marex_amd.event_exposure(ids, regions, cell_areas=areas, dat_anomaly=anom, per_timestep=True)
    others = [marex_amd.event_exposure(ids, regions, cell_areas=areas, dat_anomaly=anom, per_timestep=True, block_steps=b) for b in (1, 2, T)]
    others.append(marex_amd.event_exposure(torch.from_numpy(ids).to(hot.device), regions, cell_areas=areas,
                                           dat_anomaly=torch.from_numpy(anom).to(hot.device), per_timestep=True, block_steps=3))
    for o in others:
        assert list(o.data_vars) == list(ds.data_vars)
        for k in ds.data_vars:
            assert np.asarray(o[k].values).tobytes() == np.asarray(ds[k].values).tobytes(), k


def _assert_dataset(ds, exp):
    want, coords = exp
    assert sorted(ds.data_vars) == sorted(want)
    for k, w in want.items():
        got = np.asarray(ds[k].values)
        assert got.shape == w.shape and got.dtype == w.dtype, (k, got.shape, w.shape, got.dtype, w.dtype)
        assert np.array_equal(got, w, equal_nan=got.dtype.kind in "fmM"), k
    assert np.array_equal(np.asarray(ds["event_regions"].coords["ID"].values), coords["ID"])
    assert np.array_equal(np.asarray(ds["region_events"].coords["region"].values), coords["region"])


def test_cross_checks_against_regional_series_and_event_intensity(hot):
    rng = np.random.default_rng(11)
    T, ny, nx = 6, 40, 64
    C = ny * nx
    ids = xc.blob_field(rng, T, C, n_ids=9, width=300)
    anom = xc.spoil(rng, xc.dyadic_anomalies(rng, (T, C)), ids)
    regions = (np.arange(C) // 900).astype(np.int64) * 4  # three regions ...
    regions[regions > 8] = -1
    regions[np.arange(C) % 11 == 5] = -1  # ... plus holes
    w = xc.dyadic_weights(rng, C) + F(1)
    ds = marex_amd.event_exposure(ids.reshape(T, ny, nx), regions.reshape(ny, nx), cell_areas=w.reshape(ny, nx),
                                  dat_anomaly=anom.reshape(T, ny, nx), per_timestep=True)
    v = {k: np.asarray(ds[k].values) for k in ds.data_vars}
    N, P = v["event_regions"].size, v["pair_ID"].size
    pair_of = np.repeat(np.arange(P), np.diff(v["pair_record_offsets"]))
    rt, rreg = v["record_time"], np.searchsorted([0, 4, 8], v["pair_region"][pair_of])
    # summed over the IDs: the regional series -- without anomalies for the cells and the area (every event cell counts
    # here, with a finite anomaly or not), with them for the integral and the invalid cells
    rs = marex_amd.regional_series(ids, regions=regions, cell_areas=w)
    rsa = marex_amd.regional_series(ids, regions=regions, cell_areas=w, dat_anomaly=anom)

    def over(vals, dt):
        o = np.zeros((T, 3), dt)
        np.add.at(o, (rt, rreg), vals)
        return o

    assert np.array_equal(over(v["record_cells"], np.int64), np.asarray(rs["cells"].values))
    assert np.array_equal(over(v["record_area"], np.float64), np.asarray(rs["area"].values))  # dyadic areas: exact sums
    assert np.array_equal(over(v["record_invalid_cells"], np.int64), np.asarray(rsa["invalid_cells"].values))
    assert np.array_equal(over(v["record_cells"] - v["record_invalid_cells"], np.int64), np.asarray(rsa["cells"].values))
    got, want = over(v["record_intensity_integral"], np.float64), np.nan_to_num(np.asarray(rsa["intensity_integral"].values))
    assert np.array_equal(got, want)  # dyadic: every partial sum is representable, so the bound is 0
    assert v["record_invalid_cells"].sum() > 0 and P > N > 3
    # summed over the regions, "none" included: event_intensity per (time, ID) -- through the engine, which keeps "none"
    rvals, rank = eo.ranks(regions)
    r, _ = run(hot, ids, rank, 3, wf=w, anom=anom)
    ei = marex_amd.event_intensity(ids, anom, cell_areas=w)
    cells, integ = (np.asarray(ei[k].values) for k in ("intensity_cells", "intensity_integral"))
    assert cells.shape == (T, N), cells.shape
    fin, sa = np.zeros((T, N), np.int64), np.zeros((T, N), np.float64)
    np.add.at(fin, (r["t"], r["id"] - 1), r["finite"])
    np.add.at(sa, (r["t"], r["id"] - 1), r["sums"][:, 1])
    assert np.array_equal(fin, cells) and np.array_equal(sa, np.nan_to_num(integ)) and (r["rank"] == 3).any()
    # one region: the steps of a pair are the duration of its event
    one = marex_amd.event_exposure(ids, np.zeros(C, int))
    assert np.array_equal(np.asarray(one["pair_steps"].values), np.asarray(ei["event_duration"].values))
    assert np.asarray(one["pair_ID"].values).tolist() == list(range(1, N + 1))


def test_public_path_on_a_grid_and_a_mesh(hot):
    rng = np.random.default_rng(12)
    T, ny, nx = 12, 9, 44
    C = ny * nx
    tv = (np.datetime64("2003-12-25") + np.arange(T)).astype("datetime64[ns]")
    ids = xc.blob_field(rng, T, C, n_ids=10, width=30)
    anom = xc.spoil(rng, xc.dyadic_anomalies(rng, (T, C)), ids)
    regions = (np.add.outer(np.arange(ny) // 3, 10 * (np.arange(nx) // 15))).reshape(-1) * 7 - 7  # -7 is no region
    valid = rng.random(C) < 0.9
    area_y = np.array([1.0, 2.5, 4.0, 6.0, 8.0, 6.0, 4.0, 2.5, 1.0])
    dims = ("time", "lat", "lon")
    f = DataArray(ids.reshape(T, ny, nx), dims=dims, coords={"time": ("time", tv)})
    a = DataArray(anom.reshape(T, ny, nx), dims=dims, coords={"time": ("time", tv)})
    for per in (False, True):
        ds = marex_amd.event_exposure(f, regions.reshape(ny, nx), cell_areas=area_y, dat_anomaly=a, mask=valid.reshape(ny, nx), per_timestep=per)
        _assert_dataset(ds, eo.exposure(ids, regions, np.repeat(area_y, nx), anom, valid, per_timestep=per, tv=tv))
    _assert_dataset(marex_amd.event_exposure(f, regions.reshape(ny, nx)), eo.exposure(ids, regions, tv=tv))
    # a mesh: areas orders of magnitude apart, whole numbers: the sums of area x anomaly stay exact
    T, C = 9, 3001
    ids = xc.blob_field(rng, T, C, n_ids=20, width=60)
    anom = xc.spoil(rng, xc.dyadic_anomalies(rng, (T, C)), ids)
    areas = rng.integers(1, 2**10, C) * 2.0 ** rng.integers(0, 12, C)
    regions = rng.integers(-1, 12, C) * 3
    ds = marex_amd.event_exposure(DataArray(ids, dims=("time", "ncells")), regions, cell_areas=areas,
                                  dat_anomaly=DataArray(anom, dims=("time", "ncells")), per_timestep=True, block_steps=4)
    _assert_dataset(ds, eo.exposure(ids, regions, areas, anom, per_timestep=True))


def _same_bytes(a, b):
    assert list(a.data_vars) == list(b.data_vars)
    for k in a.data_vars:
        assert np.asarray(a[k].values).tobytes() == np.asarray(b[k].values).tobytes(), k


@pytest.mark.parametrize("merging", [True, False], ids=["merge", "basic"])
def test_tracker_method_on_its_own_tracked_field(hot, merging):
    from intensity_cases import blob_anomalies, blobs

    ev = blobs()
    T, ny, nx = ev.shape
    tv = np.arange(T).astype("datetime64[D]").astype("datetime64[ns]")
    lat, lon = np.linspace(-57.5, 57.5, ny).astype(F), np.linspace(3.75, 356.25, nx).astype(F)
    valid = np.ones((ny, nx), bool)
    valid[5:9, 6:12] = False
    ev = ev & valid[None]
    dims = ("time", "lat", "lon")
    coords = {"time": ("time", tv), "lat": ("lat", lat), "lon": ("lon", lon)}
    trk = marex_amd.tracker(DataArray(ev, dims=dims, coords=coords, name="extreme_events"), DataArray(valid, dims=("lat", "lon")),
                            R_fill=1, T_fill=2, area_filter_quartile=0.2, timechunks=4, coordinate_units="degrees",
                            allow_merging=merging, grid_resolution=7.5)
    events = trk.run()
    ids = np.asarray(events["ID_field"].values)
    assert ids.max() >= 2
    anom = blob_anomalies(ev.shape)
    ex = marex_amd.Dataset({"dat_anomaly": DataArray(anom, dims=dims, coords=coords)})
    regions = np.add.outer(np.arange(ny) // 8, 3 * (np.arange(nx) // 16))
    regions[:, :5] = -1
    areas = trk._cell_weights if merging else None
    n = int(np.asarray(events["ID"].values).size) if "ID" in events else None
    # the tracker's own mask and areas.  The merge tracker's float32 areas are any float32, so the partial sums of w a need
    # not be representable and the four variables behind them are left to the dyadic run below; everything else is equal.
    ds = trk.event_exposure(events, regions, ex, per_timestep=True)
    exp = eo.exposure(ids.reshape(T, -1), regions.reshape(-1), None if areas is None else areas.reshape(-1), anom.reshape(T, -1),
                      valid.reshape(-1), per_timestep=True, tv=tv, n_events=n)
    loose = ("pair_intensity_integral", "pair_intensity_mean", "record_intensity_integral", "record_intensity_mean") if merging else ()
    assert sorted(ds.data_vars) == sorted(exp[0])
    for k, w in exp[0].items():
        got = np.asarray(ds[k].values)
        assert got.shape == w.shape and got.dtype == w.dtype, k
        assert k in loose or np.array_equal(got, w, equal_nan=got.dtype.kind in "fmM"), k
    if merging:
        assert not np.array_equal(np.asarray(ds["record_area"].values), np.asarray(ds["record_cells"].values).astype(np.float64))
    # whole-number areas per row: every sum is exact, the Dataset is the oracle's and that of the free function
    wy = np.arange(1.0, ny + 1)
    ds = trk.event_exposure(events, regions, ex, per_timestep=True, cell_areas=wy, block_steps=5)
    _assert_dataset(ds, eo.exposure(ids.reshape(T, -1), regions.reshape(-1), np.repeat(wy, nx), anom.reshape(T, -1), valid.reshape(-1),
                                    per_timestep=True, tv=tv, n_events=n))
    _same_bytes(ds, marex_amd.event_exposure(events["ID_field"], regions, mask=valid, cell_areas=wy, dat_anomaly=ex["dat_anomaly"],
                                             per_timestep=True))
    assert np.asarray(ds["pair_ID"].values).size > 0 and np.asarray(ds["event_outside_share"].values).max() > 0
    if merging:
        assert np.asarray(ds["event_regions"].values).size == n
        bad = marex_amd.Dataset({"ID_field": events["ID_field"], "ID": DataArray(np.arange(1, 2), dims=("ID",))})
        if n > 1:
            with pytest.raises(ProcessingError, match="the ID field holds event"):
                trk.event_exposure(bad, regions)
    with pytest.raises(TypeError, match="unexpected keyword argument 'by'"):
        trk.event_exposure(events, regions, by="year")


def test_mesh_tracker_method_on_its_own_tracked_field(hot):
    from test_mesh_merge_host import THRESHOLD, load_merging_fixture

    f = load_merging_fixture()  # the fixture and the tracker of tests/test_gpu_mesh_events.py
    mask = DataArray(f["ev"], dims=("time", "ncells"),
                     coords={"time": ("time", f["time"]), "lat": ("ncells", f["lat"]), "lon": ("ncells", f["lon"])})
    trk = marex_amd.tracker(mask, DataArray(f["mask"], dims=("ncells",)), R_fill=1, area_filter_quartile=None, area_filter_absolute=5,
                            T_fill=2, overlap_threshold=THRESHOLD, nn_partitioning=True, unstructured_grid=True,
                            dimensions={"x": "ncells"}, coordinates={"x": "lon", "y": "lat"}, coordinate_units="degrees",
                            neighbours=DataArray(f["nb"], dims=("nv", "ncells")), cell_areas=DataArray(f["areas"], dims=("ncells",)),
                            timechunks=5)
    events = trk.run()
    ids = np.asarray(events["ID_field"].values)
    assert ids.max() >= 2
    valid, areas = np.asarray(f["mask"]).astype(bool), np.asarray(f["areas"])
    regions = (np.asarray(f["lat"]) > np.median(f["lat"])).astype(np.int64) * 5 + 2  # two regions, 2 and 7
    regions[::9] = -1
    n = int(np.asarray(events["ID"].values).size) if "ID" in events else None
    # without anomalies everything is an exact integer or one conversion of one: the tracker's mask and areas are the defaults
    ds = trk.event_exposure(events, regions, per_timestep=True)
    _assert_dataset(ds, eo.exposure(ids, regions, areas, None, valid, per_timestep=True, tv=np.asarray(f["time"]), n_events=n))
    assert np.asarray(ds["pair_ID"].values).size >= 2 and np.asarray(ds["region_events"].coords["region"].values).tolist() == [2, 7]
