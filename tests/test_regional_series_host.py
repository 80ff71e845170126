"""The regional series on the host: the oracle against hand-computed values, the area table against the mesh tracker's, the
validation errors (raised before any device work), and the public path -- region ranks, areas, threshold layouts, windows,
the carried slots, the host finish and the ``by=`` groups -- on a NumPy stand-in for the engine call.  No GPU needed."""
import os
import sys

import numpy as np
import pytest

import marex_amd
import marex_amd._stream as mi
import marex_amd.regional as mr
from marex_amd import calendar
from marex_amd.engine import HotPath
from marex_amd.exceptions import ConfigurationError, DataValidationError
from marex_amd.track_mesh import mesh_weight_tables
from marex_amd.xr_compat import DataArray

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import regional_series_cases as rc  # noqa: E402
import regional_series_oracle as ro  # noqa: E402
from regional_series_host_engine import HostEngine  # noqa: E402

NAN, INF = np.nan, np.inf
F = np.float32


def test_oracle_on_a_hand_computed_field():
    #              cell 0    1     2     3     4     5
    reg = np.array([0,       0,    1,    1,    -1,   2])
    x = np.array([[1,        1,    1,    0,    1,    1],
                  [0,        2,    2,    2,    2,    0]], np.int32)
    a = np.array([[1.0,      -2.0, NAN,  9.0,  9.0,  INF],
                  [9.0,      0.5,  -1.0, -3.0, 9.0,  9.0]], F)
    q = np.array([10, 20, 30, 40, 50, 60], np.int64)
    w = np.array([1.0, 2.0, 1.0, 0.5, 1.0, 1.0], F)
    thr = np.array([[1.0, 1.0, 1.0, 1.0, 1.0, 1.0], [0.25, 0.25, NAN, 1.0, 1.0, 1.0]], F)
    s = ro.finish(ro.accumulate(x, reg, 3, 2, q=q, wf=w, anom=a, thr=thr, doy=[0, 1]))
    assert s["cnt"].tolist() == [[[2, 0], [0, 1], [0, 1]], [[1, 0], [2, 0], [0, 0]]]
    assert s["area"].tolist() == [[30, 0, 0], [20, 70, 0]]  # a cell with a NaN or infinite anomaly adds no area
    assert s["sums"].tolist() == [[[3.0, -3.0], [0.0, 0.0], [0.0, 0.0]], [[2.0, 1.0], [1.5, -2.5], [0.0, 0.0]]]
    assert np.array_equal(s["vmax"], np.array([[1.0, NAN, NAN], [0.5, -1.0, NAN]], F), equal_nan=True)
    assert s["cat_cnt"][0, 0].tolist() == [1, 1, 0, 0, 0, 0] and s["cat_cnt"][1].tolist() == [[0, 0, 1, 0, 0, 0], [1, 0, 0, 0, 0, 1], [0] * 6]
    assert s["cat_area"][1].tolist() == [[0, 0, 20, 0, 0, 0], [40, 0, 0, 0, 0, 30], [0] * 6] and s["status"] == [0, 0]
    # without anomalies every present cell counts
    p = ro.finish(ro.accumulate(x, reg, 3, 2, q=q))
    assert p["cnt"][..., 0].tolist() == [[2, 1, 1], [1, 2, 0]] and p["area"].tolist() == [[30, 30, 60], [20, 70, 0]]
    assert ro.finish(ro.accumulate(x, reg, 3, 2, match=2))["area"].tolist() == [[0, 0, 0], [1, 2, 0]]
    # any cut gives the state of the whole; a label outside its range counts the cells and nothing else; negative IDs
    st = ro.accumulate(x[:1], reg, 3, 2, 0, q, w, a[:1], thr, [0, 1])
    st = ro.finish(ro.accumulate(x[1:], reg, 3, 2, 1, q, w, a[1:], thr, [0, 1], state=st))
    assert all(np.array_equal(st[k], s[k], equal_nan=k == "vmax") for k in ("area", "cnt", "sums", "vmax", "cat_cnt", "cat_area"))
    b = ro.accumulate(x, reg, 3, 2, anom=a, thr=thr, doy=[0, 2])
    assert b["status"] == [0, 3] and b["cnt"][1].sum() == 0
    assert ro.accumulate(np.array([[-1, 2, 0, -3, 0, 0]], np.int32), reg, 3, 1)["status"] == [2, 0]
    W, S, A, n = ro.exact_sums(x, reg, 3, w, a)
    assert S.tolist() == [[-3.0, 0.0, 0.0], [1.0, -2.5, 0.0]] and A[0, 0] == 5.0 and n.tolist() == [[2, 0, 0], [1, 2, 0]]


def test_area_table_has_the_bits_of_the_mesh_trackers():
    rng = np.random.default_rng(0)
    for a in (rng.uniform(1e3, 1e9, 500), rng.uniform(0, 1, 77).astype(F), np.array([0.0, 3.0, 0.0]), np.full(64, 2.0 ** -3),
              np.cos(np.radians(np.linspace(-89, 89, 90))) * 111.0 ** 2):
        e, q = mr.area_weight_table(a)
        e4, q4 = mesh_weight_tables(a, np.zeros(a.size), np.zeros(a.size))
        assert e == e4 and q.dtype == np.int64 and q.tobytes() == q4[0].tobytes()
        assert 2**60 - a.size < sum(int(v) for v in q) <= 2**61 + a.size
    e, q = mr.area_weight_table(np.ones((3, 4)))
    assert q.shape == (3, 4) and e == 61 - 4 and (q == 2**57).all()
    for bad in ([1.0, NAN], [1.0, -1.0], [INF, 1.0], [0.0, 0.0], []):
        with pytest.raises(DataValidationError, match="cell_areas must"):
            mr.area_weight_table(np.array(bad))
    e, q, wf = rc.near_2_61(rng, 1000)
    assert wf.dtype == F and q.min() > 0


def _no_gpu(monkeypatch):
    import marex_amd.detect as det

    def no_gpu(*a, **k):
        raise AssertionError("the validation touched the GPU engine")

    monkeypatch.setattr(det, "get_engine", no_gpu)


def test_validation_errors_come_before_the_device(monkeypatch):
    _no_gpu(monkeypatch)
    x = np.zeros((3, 4, 5), np.uint8)
    an = np.zeros((3, 4, 5), F)
    V, Cf = DataValidationError, ConfigurationError
    cases = [
        (dict(field=x[0, 0]), V, r"field must be \(time, y, x\) or \(time, cells\)"),
        (dict(field=x.astype(F)), V, "field must be a mask .* or an integer ID field"),
        (dict(dat_anomaly=an[:2]), V, "field and dat_anomaly differ in shape"),
        (dict(dat_anomaly=x), V, "dat_anomaly must be a floating-point field"),
        (dict(regions=np.zeros((5, 4), np.int32)), V, "regions does not match the spatial shape"),
        (dict(regions=np.zeros(19, np.int32)), V, "regions does not match the spatial shape"),
        (dict(regions=np.zeros((4, 5))), V, "regions must be an integer map"),
        (dict(mask=np.ones((4, 4), bool)), V, "mask does not match the spatial shape"),
        (dict(mask=np.ones((4, 5))), V, "mask must be boolean or integer"),
        (dict(cell_areas=np.ones(5)), V, "cell_areas does not match the spatial shape"),
        (dict(cell_areas=np.ones((4, 5), bool)), V, "cell_areas must be numbers"),
        (dict(cell_areas=np.array([1.0, NAN, 1.0, 1.0])), V, "cell_areas must be finite and non-negative"),
        (dict(cell_areas=np.array([1.0, -1.0, 1.0, 1.0])), V, "cell_areas must be finite and non-negative"),
        (dict(cell_areas=np.full((4, 5), INF)), V, "cell_areas must be finite and non-negative"),
        (dict(cell_areas=np.zeros((4, 5))), V, "cell_areas must have a positive, finite sum"),
        (dict(thresholds=np.ones((4, 5), F)), V, "thresholds need dat_anomaly"),
        (dict(dat_anomaly=an, thresholds=np.ones((5, 4), F)), V, "thresholds do not match the spatial shape of the field"),
        (dict(dat_anomaly=an, thresholds=np.ones((4, 5), np.int32)), V, "thresholds must be a floating-point field"),
        (dict(dat_anomaly=an, thresholds=np.ones((366, 4, 5), F)), V, "thresholds by dayofyear needs a datetime time coordinate"),
        (dict(event_id=3), V, "event_id needs an ID field, not a mask"),
        (dict(field=x.astype(np.int32), event_id=0), V, "event_id must be a positive int32 ID"),
        (dict(field=x.astype(np.int32), event_id=1.5), V, "event_id must be a positive int32 ID"),
        (dict(by="week"), Cf, "by must be one of"),
        (dict(by="year"), V, "by='year' needs a datetime time coordinate"),
        (dict(by=np.zeros(4, np.int32)), V, "by labels must be one integer per timestep"),
    ]
    cases += [(dict(block_steps=b), Cf, "block_steps must be a positive number of timesteps, 'auto' or None")
              for b in (0, -2, 2.5, True, "all")]
    for kw, cls, msg in cases:
        args = dict(field=x)
        args.update(kw)
        with pytest.raises(cls, match=msg):
            marex_amd.regional_series(**args)
    big = np.zeros((1, 40000), np.uint8)
    with pytest.raises(V, match="regions holds 32768 distinct regions, at most 32767 are taken"):
        marex_amd.regional_series(big, regions=np.minimum(np.arange(40000), 32767))


def test_regional_series_is_public():
    assert "regional_series" in marex_amd.__all__ and marex_amd.regional_series is mr.regional_series
    assert hasattr(marex_amd.tracker, "regional_series") and hasattr(HotPath, "regional_series")
    from marex_amd import _lib
    from marex_amd.csrc import build

    assert "marex_regional_series_u8" in _lib.PROTOTYPES and "marex_regional_series_i32" in _lib.PROTOTYPES
    assert "marex_regional" in build.UNITS and "regional_series" in marex_amd.__doc__
    assert "marex_regional_layout" in _lib.PROTOTYPES and mr.MAX_REGIONS == HotPath.REGIONAL_MAX_REGIONS == 32767
    # the layout comes from the library: a wave's run must fit the packed counts of the kernel's reductions
    for v in (1, 4):
        wave, wg, stride = HotPath.regional_layout(v)
        assert wave % (64 * v) == 0 and wg == 4 * wave and stride >= 1 and wave <= 1024
    assert HotPath.regional_layout(1)[0] < 1024  # six class counts of ten bits each
    with pytest.raises(marex_amd.ProcessingError, match="cells_per_lane must be 1 or 4"):
        HotPath.regional_layout(2)
    assert HotPath.regional_slot_bytes(10, 3, False, False, False) == 11 * 3 * 24
    assert HotPath.regional_slot_bytes(10, 3, True, True, True) == 11 * 3 * 144
    assert rc.layout_edges() == sorted({rc.WAVE[v] + d for v in (1, 4) for d in (-1, 0, 1)} | {rc.WG[v] + d for v in (1, 4) for d in (-1, 0, 1)}
                                       | {rc.WAVE[4] - 4, rc.WAVE[4] + 4, rc.WG[4] - 4, rc.WG[4] + 4})


@pytest.fixture
def host_engine(monkeypatch):
    import marex_amd.detect as det

    eng = HostEngine()
    monkeypatch.setattr(det, "get_engine", lambda device=0: eng)
    monkeypatch.setattr(mi, "_free_bytes", lambda e: 1 << 30)
    return eng


def same(a, b):
    assert list(a.data_vars) == list(b.data_vars)
    for k in a.data_vars:
        assert np.asarray(a[k].values).tobytes() == np.asarray(b[k].values).tobytes(), k
        assert tuple(a[k].dims) == tuple(b[k].dims), k


DTYPES = {"cells": np.int64, "area": np.float64, "area_share": np.float64, "cells_share": np.float64, "region_cells": np.int64,
          "region_area": np.float64, "intensity_mean": np.float64, "intensity_max": np.float32, "intensity_integral": np.float64,
          "invalid_cells": np.int64, "category_cells": np.int64, "category_area": np.float64, "category_share": np.float64,
          "steps_by": np.int64, "cell_steps_by": np.int64, "area_steps_by": np.float64, "share_by": np.float64,
          "intensity_max_by": np.float32, "category_cell_steps_by": np.int64, "category_area_steps_by": np.float64}


def assert_equals_oracle(ds, exp):
    assert sorted(ds.data_vars) == sorted(exp)
    for k, want in exp.items():
        got = np.asarray(ds[k].values)
        assert got.dtype == DTYPES[k] == want.dtype, (k, got.dtype, want.dtype)
        assert got.shape == want.shape, (k, got.shape, want.shape)
        assert np.array_equal(got, want, equal_nan=got.dtype.kind == "f"), k


TIMES = np.array(["2001-12-30", "2001-12-31", "2002-01-01", "2002-02-28", "2002-03-01", "2002-06-01", "2002-12-01", "2003-01-01",
                  "2003-07-04", "2004-02-29", "2004-12-31"], dtype="datetime64[D]").astype("datetime64[ns]")
YEAR = np.array([0, 0, 1, 1, 1, 1, 1, 2, 2, 3, 3], np.int32)
DOY = np.array([364, 365, 1, 59, 60, 152, 335, 1, 185, 60, 366], np.int32)


@pytest.mark.parametrize("by", [None, "year", "labels"])
def test_grid_schema_groups_and_windows_on_the_host_engine(host_engine, by):
    import torch

    rng = np.random.default_rng(1)
    T, ny, nx = TIMES.size, 5, 8
    C = ny * nx
    x = rc.mask_field(rng, T, C)
    anom = rc.spoil(rng, rc.dyadic_anomalies(rng, (T, C)), x)
    thr = rc.thresholds(rng, calendar.N_DOY, C)
    regions = np.repeat([[40, 40, 7, 7, 7, -1, 900, 900]], ny, axis=0)
    regions[0, :2] = -5
    valid = np.ones((ny, nx), bool)
    valid[:, 6] = False  # region 900 keeps one column
    valid[4, 7] = False
    area_y = np.array([1.0, 2.5, 4.0, 2.5, 1.0])
    labels = np.array([2, 0, 0, 2, 2, 0, 4, 4, 0, 2, 0], np.int32)
    lab, G = {None: (None, 1), "year": (YEAR, 4), "labels": (labels, 5)}[by]
    exp = ro.regional_series(x, regions.reshape(-1), np.repeat(area_y, nx), anom, thr, DOY - 1, valid.reshape(-1), lab, G)
    dims = ("time", "lat", "lon")
    coords = {"time": ("time", TIMES), "lat": ("lat", np.linspace(-30, 30, ny)), "lon": ("lon", np.linspace(0, 70, nx))}
    f = DataArray(x.reshape(T, ny, nx), dims=dims, coords=coords)
    a = DataArray(anom.reshape(T, ny, nx), dims=dims, coords=coords)
    h = DataArray(thr.reshape(-1, ny, nx), dims=("dayofyear", "lat", "lon"))
    kw = dict(regions=DataArray(regions, dims=("lat", "lon")), cell_areas=area_y, dat_anomaly=a, thresholds=h, mask=valid,
              by=labels if by == "labels" else by)
    whole = marex_amd.regional_series(f, **kw)
    assert_equals_oracle(whole, exp)
    assert host_engine.calls == [("regional_series", "uint8", 0, T, 3, 366)]
    assert np.asarray(whole["cells"].coords["region"].values).tolist() == [7, 40, 900]
    assert np.asarray(whole["region_cells"].values).tolist() == [15, 8, 4]
    assert np.asarray(whole["region_area"].values).tolist() == [33.0, 20.0, 10.0]
    assert tuple(whole["cells"].dims) == ("time", "region") and tuple(whole["category_area"].dims) == ("time", "region", "category")
    assert np.array_equal(whole["area"].coords["time"].values, TIMES)
    assert np.asarray(whole["category_cells"].coords["category"].values).tolist() == list(mr.CATEGORIES)
    area, cat = np.asarray(whole["area"].values), np.asarray(whole["category_area"].values)
    assert np.array_equal(cat.sum(axis=2), area) and (np.asarray(whole["invalid_cells"].values) > 0).any()
    assert (np.asarray(whole["area_share"].values) <= 1).all() and (area > 0).any()
    if by is not None:
        gname = "year" if by == "year" else "group"
        assert tuple(whole["cell_steps_by"].dims) == (gname, "region") and tuple(whole["steps_by"].dims) == (gname,)
        assert tuple(whole["category_area_steps_by"].dims) == (gname, "region", "category")
        assert np.asarray(whole["cell_steps_by"].values).sum() == np.asarray(whole["cells"].values).sum()
        if by == "year":
            assert np.asarray(whole["steps_by"].coords["year"].values).tolist() == [2001, 2002, 2003, 2004]
            assert np.asarray(whole["steps_by"].values).tolist() == [2, 5, 2, 2]
        else:
            assert np.isnan(np.asarray(whole["share_by"].values)[1]).all() and np.isnan(np.asarray(whole["intensity_max_by"].values)[3]).all()
    for b in (1, 4, "auto"):  # window plans: the same Dataset
        host_engine.calls.clear()
        same(whole, marex_amd.regional_series(f, block_steps=b, **kw))
        if b == 4:
            assert [c[2:4] for c in host_engine.calls] == [(s, min(4, T - s)) for s in range(0, T, 4)]
    # bool, a tensor, thresholds (*space, dayofyear), the [y, x] areas written out: the same bytes
    kw2 = dict(kw, cell_areas=np.repeat(area_y[:, None], nx, axis=1),
               thresholds=np.ascontiguousarray(np.moveaxis(thr.reshape(-1, ny, nx), 0, -1)))
    same(whole, marex_amd.regional_series(DataArray(x.reshape(T, ny, nx).astype(bool), dims=dims, coords=coords), **kw2))
    same(whole, marex_amd.regional_series(f, **dict(kw2, thresholds=torch.from_numpy(thr.reshape(-1, ny, nx)))))


def test_mesh_defaults_event_id_and_empty_regions(host_engine):
    rng = np.random.default_rng(2)
    T, C = 7, 61
    ids = rc.id_field(rng, T, C)
    anom = rc.spoil(rng, rc.dyadic_anomalies(rng, (T, C)), ids)
    areas = rng.integers(1, 2**10, C) * 2.0 ** rng.integers(0, 12, C)
    # no regions: one region 0 of every cell; no areas: cells
    ds = marex_amd.regional_series(ids)
    assert_equals_oracle(ds, ro.regional_series(ids))
    assert np.asarray(ds["cells"].coords["region"].values).tolist() == [0] and np.asarray(ds["region_cells"].values).tolist() == [C]
    assert np.array_equal(np.asarray(ds["area"].values), np.asarray(ds["cells"].values).astype(np.float64))
    assert np.array_equal(np.asarray(ds["cells"].coords["time"].values), np.arange(T))
    assert_equals_oracle(marex_amd.regional_series(ids, cell_areas=areas, dat_anomaly=anom, event_id=np.int64(3)),
                         ro.regional_series(ids, None, areas, anom, match=3))
    assert host_engine.calls[-1][1] == "int32"
    assert_equals_oracle(marex_amd.regional_series(ids.astype(np.int16), dat_anomaly=anom.astype(np.float64)),
                         ro.regional_series(ids, anom=anom))
    # (*space) thresholds: one row, no calendar
    g = np.linspace(0.2, 1.4, C)
    assert_equals_oracle(marex_amd.regional_series(ids, dat_anomaly=anom, thresholds=g, cell_areas=areas),
                         ro.regional_series(ids, None, areas, anom, g.astype(F)[None], np.zeros(T, np.int32)))
    assert host_engine.calls[-1] == ("regional_series", "int32", 0, T, 1, 1)
    # a region that the mask empties, and a map without any region: shares are NaN, not an error
    regions = np.arange(C) % 3
    ds = marex_amd.regional_series(ids, regions=regions, mask=regions != 1, cell_areas=areas, dat_anomaly=anom)
    assert_equals_oracle(ds, ro.regional_series(ids, regions, areas, anom, mask=regions != 1))
    assert np.asarray(ds["region_cells"].values)[1] == 0 and np.isnan(np.asarray(ds["area_share"].values)[:, 1]).all()
    assert np.isnan(np.asarray(ds["cells_share"].values)[:, 1]).all() and np.isnan(np.asarray(ds["intensity_mean"].values)[:, 1]).all()
    assert not np.isnan(np.asarray(ds["area_share"].values)[:, 0]).any() and (np.asarray(ds["cells"].values)[:, 1] == 0).all()
    none = marex_amd.regional_series(ids, regions=np.full(C, -1))
    assert np.asarray(none["cells"].values).shape == (T, 1) and np.isnan(np.asarray(none["area_share"].values)).all()
    # a union of regions is the exact integer sum of its parts
    both = marex_amd.regional_series(ids, regions=np.where(regions == 1, -1, 0), cell_areas=areas, dat_anomaly=anom)
    parts = marex_amd.regional_series(ids, regions=regions, cell_areas=areas, dat_anomaly=anom)
    assert np.array_equal(np.asarray(both["cells"].values)[:, 0], np.asarray(parts["cells"].values)[:, [0, 2]].sum(axis=1))
    with pytest.raises(DataValidationError, match="Object IDs must be non-negative"):
        marex_amd.regional_series(np.where(ids == 3, -1, ids), block_steps=2)
    with pytest.raises(marex_amd.TrackingError, match=r"regional_series: needs .* GB of device memory, .* GB are free"):
        marex_amd.regional_series(np.zeros((64, 1 << 25), bool))


def test_empty_fields_need_no_device(monkeypatch):
    _no_gpu(monkeypatch)
    for shape in ((0, 5), (4, 0), (0, 2, 3)):
        e = marex_amd.regional_series(np.zeros(shape, np.uint8), dat_anomaly=np.zeros(shape, F), thresholds=np.ones(shape[1:], F))
        assert np.asarray(e["cells"].values).shape == (shape[0], 1) and np.asarray(e["category_cells"].values).shape == (shape[0], 1, 6)
        assert not np.asarray(e["cells"].values).any() and np.isnan(np.asarray(e["intensity_max"].values)).all()
        assert np.asarray(e["region_cells"].values).tolist() == [int(np.prod(shape[1:]))]


def test_tracker_method_takes_the_fields_from_the_datasets(monkeypatch):
    seen = {}
    monkeypatch.setattr(mr, "_regional_series", lambda field, regions, **kw: seen.update(field=field, regions=regions, **kw) or "ds")

    class T:  # the attributes the method reads
        device, unstructured_grid, cell_area, mask = 0, True, np.arange(5.0), np.ones(5, bool)
        timedim, timecoord, time_values = "step", "date", np.array([3, 4])

    ev = marex_amd.Dataset({"ID_field": DataArray(np.zeros((2, 5), np.int32), dims=("time", "ncells"))})
    ex = marex_amd.Dataset({"dat_anomaly": DataArray(np.zeros((2, 5), F), dims=("time", "ncells")),
                            "extreme_events": DataArray(np.zeros((2, 5), bool), dims=("time", "ncells")),
                            "thresholds": DataArray(np.ones(5, F), dims=("ncells",))})
    reg = np.zeros(5, np.int32)
    assert marex_amd.tracker.regional_series(T(), ev, ex, regions=reg, by="year") == "ds"
    assert seen["field"] is ev["ID_field"] and seen["dat_anomaly"] is ex["dat_anomaly"] and seen["thresholds"] is ex["thresholds"]
    assert seen["regions"] is reg and seen["cell_areas"].tolist() == [0, 1, 2, 3, 4] and seen["mask"] is T.mask and seen["by"] == "year"
    seen.clear()
    T.unstructured_grid, T._cell_weights = False, np.ones((1, 5), F)
    marex_amd.tracker.regional_series(T(), ex["extreme_events"], thresholds=None, block_steps=3, mask=None)
    assert seen["field"] is ex["extreme_events"] and seen["dat_anomaly"] is None and seen["thresholds"] is None and seen["mask"] is None
    assert seen["cell_areas"] is T._cell_weights and seen["block_steps"] == 3 and seen["device"] == 0 and seen["regions"] is None
    assert seen["time"][:2] == ("step", "date") and seen["time"][2] is T.time_values
    with pytest.raises(TypeError, match="unexpected keyword argument 'zonal'"):
        marex_amd.tracker.regional_series(T(), ev, zonal=True)


def test_the_trackers_time_names_and_values(host_engine):
    """``time=`` of the tracker's call: its dimension and coordinate names, and its values where the field has none."""
    rng = np.random.default_rng(3)
    T, C = TIMES.size, 9
    x = rc.mask_field(rng, T, C)
    ds = mr._regional_series(x, None, None, None, None, None, "year", None, None, None, time=("step", "date", TIMES))
    assert tuple(ds["cells"].dims) == ("step", "region") and np.array_equal(ds["cells"].coords["date"].values, TIMES)
    assert np.asarray(ds["steps_by"].values).tolist() == [2, 5, 2, 2]  # by="year" from the tracker's dates
    plain = marex_amd.regional_series(DataArray(x, dims=("time", "cells"), coords={"time": ("time", TIMES)}), by="year")
    for k in plain.data_vars:
        assert np.asarray(plain[k].values).tobytes() == np.asarray(ds[k].values).tobytes(), k
    short = mr._regional_series(x, None, None, None, None, None, None, None, None, None, time=("step", "date", TIMES[:3]))
    assert np.array_equal(short["cells"].coords["date"].values, np.arange(T))  # values of another length are not used
