"""Occurrence statistics on the host: the oracle against hand-computed values, the time labels derived from datetime64,
the latitude bin rule, the validation errors (raised before any device work) and the public path -- labels, windows, the
carried run state, the host finish -- on a NumPy stand-in for the engine call.  No GPU needed."""
import os
import sys

import numpy as np
import pytest

import marex_amd
import marex_amd._stream as mi
import marex_amd.occurrence as mo
from marex_amd.engine import HotPath
from marex_amd.exceptions import ConfigurationError, DataValidationError
from marex_amd.xr_compat import DataArray

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import occurrence_oracle as oo  # noqa: E402
from occurrence_host_engine import HostEngine  # noqa: E402

NAN = np.nan
# cell 0: one run over the whole axis; cell 1: two runs separated by one step; cell 2: never present; cell 3: events 2 and 3
FIELD = np.array([[1, 1, 0, 2, 0, 0, 5, 0],
                  [1, 1, 0, 2, 0, 4, 5, 0],
                  [1, 0, 0, 3, 0, 4, 0, 0],
                  [1, 1, 0, 3, 0, 0, 5, 7]], np.int32)


def test_oracle_on_a_hand_computed_field():
    r = oo.occurrence(FIELD, event_ids=[3, 5, 9])
    assert r["occurrence"].tolist() == [4, 3, 0, 4, 0, 2, 3, 1] and r["occurrence"].dtype == np.uint32
    assert r["frequency"].tolist() == [1.0, 0.75, 0.0, 1.0, 0.0, 0.5, 0.75, 0.25]
    assert r["n_runs"].tolist() == [1, 2, 0, 1, 0, 1, 2, 1]
    assert r["longest_run"].tolist() == [4, 2, 0, 4, 0, 2, 2, 1]
    assert np.array_equal(r["mean_run"], [4.0, 1.5, NAN, 4.0, NAN, 2.0, 1.5, 1.0], equal_nan=True)
    assert r["local_duration"].tolist() == [[0, 0, 0, 2, 0, 0, 0, 0], [0, 0, 0, 0, 0, 0, 3, 0], [0] * 8]
    assert oo.run_stats(FIELD)[0].tolist() == [4, 1, 0, 4, 0, 0, 1, 1]  # the run open after the last row
    # a selected ID: the run of event 2 in cell 3 ends where event 3 takes over
    assert oo.run_stats(FIELD, match=2)[:, 3].tolist() == [0, 1, 2]
    # the carried state: any cut gives the arrays of the whole
    for cut in (1, 2, 3):
        assert np.array_equal(oo.run_stats(FIELD[cut:], state=oo.run_stats(FIELD[:cut])), oo.run_stats(FIELD))
    # groups: steps 0, 3 -> 0; step 1 -> 2; step 2 -> 5 (outside G = 3: counted nowhere)
    cc = oo.cell_counts(FIELD, [0, 2, 5, 0], 3)
    assert cc[0].tolist() == [2, 2, 0, 2, 0, 0, 2, 1] and not cc[1].any() and cc[2].tolist() == [1, 1, 0, 1, 0, 1, 1, 0]
    assert oo.status(FIELD, [0, 2, 5, 0], 3) == [0, 3]
    # sections: classes 0, 0, 1, 1, -1, 2, 2, 3 with R = 3 (the last one outside); labels 0, 0, 1, 1
    sc = oo.section_counts(FIELD, [0, 0, 1, 1], 2, [0, 0, 1, 1, -1, 2, 2, 3], 3)
    assert sc.tolist() == [[4, 2, 3], [3, 2, 2]] and sc.dtype == np.uint64
    assert oo.status(np.array([[-1, 2], [0, -3]], np.int32)) == [2, 0]


def _days(*dates):
    return np.array(dates, dtype="datetime64[D]").astype("datetime64[ns]")


def test_labels_from_datetime64():
    tv = _days("1999-12-31", "2000-01-01", "2000-02-29", "2000-03-01", "2000-06-30", "2000-09-01", "2000-12-01", "2001-02-28")
    lab, G, name, vals = mo.group_labels("season", tv, tv.size)
    assert vals.tolist() == ["DJF", "JJA", "MAM", "SON"] and G == 4 and name == "season" and lab.dtype == np.int32
    assert lab.tolist() == [0, 0, 0, 2, 1, 3, 0, 0]  # 1999-12-31 and 2000-02-29 are DJF, December belongs to DJF
    lab, G, name, vals = mo.group_labels("dayofyear", tv, tv.size)
    assert vals[lab].tolist() == [365, 1, 60, 61, 182, 245, 336, 59] and name == "dayofyear" and G == vals.size == 8
    lab, G, _, vals = mo.group_labels("year", tv, tv.size)
    assert vals.tolist() == [1999, 2000, 2001] and lab.tolist() == [0, 1, 1, 1, 1, 1, 1, 2]
    lab, G, _, vals = mo.group_labels("month", tv, tv.size)
    assert G == 12 and vals.tolist() == list(range(1, 13)) and (lab + 1).tolist() == [12, 1, 2, 3, 6, 9, 12, 2]
    # the month groups of a series that starts mid-month: one per calendar month of the series, empty ones included
    tv = _days("2001-01-17", "2001-01-31", "2001-02-01", "2001-04-30", "2001-05-01")
    lab, G2, name, vals = mo.zonal_labels("month", tv, tv.size)
    assert lab.tolist() == [0, 0, 1, 3, 4] and G2 == 5 and name == "zonal_month"
    assert vals.astype("datetime64[D]").astype(str).tolist() == ["2001-01-01", "2001-02-01", "2001-03-01", "2001-04-01", "2001-05-01"]
    lab, G2, name, vals = mo.zonal_labels("step", tv, tv.size)
    assert lab.tolist() == [0, 1, 2, 3, 4] and G2 == 5 and np.array_equal(vals, tv)
    lab, G2, _, _ = mo.zonal_labels(np.array([3, 0, 0, 1, 3]), None, 5)
    assert lab.tolist() == [3, 0, 0, 1, 3] and G2 == 4


def test_latitude_bins_are_right_closed():
    edges = np.array([-10.0, 0.0, 10.0, 30.0])
    lat = np.array([-10.0, -9.999, 0.0, 1e-9, 10.0, 30.0, 30.001, -11.0, np.nan, np.inf, -np.inf, 20.0])
    cls, R, e = mo.lat_classes(lat, edges, lat.size)
    assert R == 3 and cls.dtype == np.int32
    assert cls.tolist() == [-1, 0, 0, 1, 1, 2, -1, -1, -1, -1, -1, 2]  # on an edge: the lower bin; the lowest edge: no bin
    assert np.array_equal(cls, oo.lat_bin(lat, edges))
    rng = np.random.default_rng(5)
    lat = np.round(rng.uniform(-95, 95, 500))  # many values exactly on the 1-degree edges
    edges = np.arange(-90.0, 91.0)
    assert np.array_equal(mo.lat_classes(lat, edges, 500)[0], oo.lat_bin(lat, edges))


def _no_gpu(monkeypatch):
    import marex_amd.detect as det

    def no_gpu(*a, **k):
        raise AssertionError("the validation touched the GPU engine")

    monkeypatch.setattr(det, "get_engine", no_gpu)


def _da(a, tv=None, dims=("time", "lat", "lon")):
    return DataArray(a, dims=dims, coords={dims[0]: (dims[0], np.arange(a.shape[0]) if tv is None else tv)})


def test_validation_errors_come_before_the_device(monkeypatch):
    _no_gpu(monkeypatch)
    ids = np.zeros((3, 4, 5), np.int32)
    mesh = np.zeros((3, 20), np.int32)
    lat = np.linspace(-9, 9, 20)
    tv = _days("2000-01-01", "2000-01-02", "2000-01-03")
    V, Cf = DataValidationError, ConfigurationError
    cases = [
        (dict(field=ids[0, 0]), V, r"field must be \(time, y, x\) or \(time, cells\)"),
        (dict(field=np.zeros((2, 2, 2, 2), np.int32)), V, r"field must be \(time, y, x\) or \(time, cells\)"),
        (dict(field=ids.astype(np.float32)), V, "field must be a mask .* or an integer ID field"),
        (dict(field=ids.astype(np.complex64)), V, "field must be a mask"),
        (dict(field=ids > 0, event_ids=[1]), V, "event_ids need an ID field, not a boolean mask"),
        (dict(event_ids=[0]), V, "event_ids must be positive int32 IDs"),
        (dict(event_ids=[2, -1]), V, "event_ids must be positive int32 IDs"),
        (dict(event_ids=[1.5]), V, "event_ids must be positive int32 IDs"),
        (dict(event_ids=[2**31]), V, "event_ids must be positive int32 IDs"),
        (dict(by="week"), Cf, "by must be one of"),
        (dict(by="season"), V, "by='season' needs a datetime time coordinate"),          # a bare array has no time coordinate
        (dict(field=_da(ids), by="month"), V, "by='month' needs a datetime time coordinate"),  # integer time values
        (dict(by=np.zeros(4, np.int32)), V, "by labels must be one integer per timestep"),
        (dict(by=np.zeros(3)), V, "by labels must be one integer per timestep"),
        (dict(by=np.array([0, -1, 0])), V, "by labels must not be negative"),
        (dict(zonal=True, zonal_by="week"), Cf, "zonal_by must be one of"),
        (dict(zonal=True), V, "zonal_by='month' needs a datetime time coordinate"),
        (dict(zonal=True, zonal_by=np.array([0, 1])), V, "zonal_by labels must be one integer per timestep"),
        (dict(zonal=True, zonal_by=np.array([0, 1, -2])), V, "zonal_by labels must not be negative"),
        (dict(zonal=True, zonal_by="step", lat_bins=[0, 1]), V, "lat and lat_bins belong to a mesh"),
        (dict(field=mesh, zonal=True, zonal_by="step"), V, "zonal presence on a mesh needs lat"),
        (dict(field=mesh, zonal=True, zonal_by="step", lat=lat), V, "zonal presence on a mesh needs lat"),
        (dict(field=mesh, zonal=True, zonal_by="step", lat=lat[:-1], lat_bins=[0, 1]), V, "lat does not match the cells"),
        (dict(field=mesh, zonal=True, zonal_by="step", lat=lat, lat_bins=[0, 2, 1]), V, "lat_bins must be at least two finite, strictly"),
        (dict(field=mesh, zonal=True, zonal_by="step", lat=lat, lat_bins=[0, 0, 1]), V, "lat_bins must be at least two finite, strictly"),
        (dict(field=mesh, zonal=True, zonal_by="step", lat=lat, lat_bins=[0]), V, "lat_bins must be at least two finite, strictly"),
        (dict(field=mesh, zonal=True, zonal_by="step", lat=lat, lat_bins=[0, np.nan]), V, "lat_bins must be at least two finite, strictly"),
        (dict(field=_da(ids, tv), by="season", zonal=True, zonal_by=np.zeros((3, 1), np.int32)), V, "zonal_by labels must be one integer"),
    ]
    cases += [(dict(block_steps=b), Cf, "block_steps must be a positive number of timesteps, 'auto' or None")
              for b in (0, -2, 2.5, True, "all")]
    for kw, cls, msg in cases:
        args = dict(field=ids)
        args.update(kw)
        with pytest.raises(cls, match=msg):
            marex_amd.event_occurrence(**args)


def test_event_occurrence_is_public():
    assert "event_occurrence" in marex_amd.__all__ and marex_amd.event_occurrence is mo.event_occurrence
    assert hasattr(marex_amd.tracker, "event_occurrence") and hasattr(HotPath, "occurrence")
    from marex_amd import _lib

    assert "marex_occurrence_u8" in _lib.PROTOTYPES and "marex_occurrence_i32" in _lib.PROTOTYPES


@pytest.fixture
def host_engine(monkeypatch):
    import marex_amd.detect as det

    eng = HostEngine()
    monkeypatch.setattr(det, "get_engine", lambda device=0: eng)
    monkeypatch.setattr(mi, "_free_bytes", lambda e: 1 << 30)
    return eng


DTYPES = {"occurrence": np.uint32, "frequency": np.float64, "n_runs": np.uint32, "longest_run": np.uint32, "mean_run": np.float64,
          "occurrence_by": np.uint32, "steps_by": np.int64, "frequency_by": np.float64, "presence_cells": np.uint64,
          "presence": np.float64, "class_cells": np.int64, "local_duration": np.uint32}


def assert_equals_oracle(ds, exp, space):
    """Every variable the oracle has, and no other: dtype, shape (the oracle is flat in space) and every value."""
    assert sorted(ds.data_vars) == sorted(exp)
    for k, want in exp.items():
        got = np.asarray(ds[k].values)
        assert got.dtype == DTYPES[k], (k, got.dtype)
        if k not in ("steps_by", "presence_cells", "presence", "class_cells"):
            assert got.shape[got.ndim - len(space):] == tuple(space), (k, got.shape)
            got = got.reshape(got.shape[:got.ndim - len(space)] + (-1,))
        assert got.shape == want.shape, (k, got.shape, want.shape)
        assert np.array_equal(got, want, equal_nan=got.dtype.kind == "f"), k


def case_field(T=9, ny=7, nx=11, seed=11):
    """An ID field with runs of every kind: events 1..6, about a third of the cells present, long runs along time."""
    rng = np.random.default_rng(seed)
    on = rng.random((T, ny * nx)) < 0.45
    on[:, 0] = True               # present throughout
    on[:, 1] = False              # never
    on[:, 2] = np.arange(T) != 4  # two runs separated by one step
    ids = np.where(on, rng.integers(1, 7, (T, ny * nx)), 0).astype(np.int32)
    ids[:, 3] = 4                 # one event throughout
    return ids


def test_public_path_on_the_host_engine(host_engine):
    import torch

    T, ny, nx = 9, 7, 11
    ids = case_field(T, ny, nx)
    tv = _days(*[f"2003-{m:02d}-{d:02d}" for m, d in ((1, 30), (1, 31), (2, 1), (2, 28), (3, 1), (3, 2), (6, 1), (12, 1), (12, 31))])
    season = np.array([0, 0, 0, 0, 2, 2, 1, 0, 0], np.int32)   # no step of SON in this year
    months = np.array([0, 0, 1, 1, 2, 2, 5, 11, 11], np.int32)  # the months of the series: January .. December
    cls = np.repeat(np.arange(ny, dtype=np.int32), nx)
    exp = oo.occurrence(ids.reshape(T, -1), season, 4, months, 12, cls, ny, np.full(ny, nx), [4, 2, 9])
    assert exp["steps_by"].tolist() == [6, 1, 2, 0] and np.isnan(exp["frequency_by"][3]).all() and not exp["occurrence_by"][3].any()
    assert np.isnan(exp["presence"][3]).all() and not np.isnan(exp["presence"][0]).any()
    lat, lon = np.linspace(-30, 30, ny), np.linspace(0, 100, nx)
    da = DataArray(ids.reshape(T, ny, nx), dims=("time", "lat", "lon"),
                   coords={"time": ("time", tv), "lat": ("lat", lat), "lon": ("lon", lon)})
    kw = dict(by="season", zonal=True, zonal_by="month", event_ids=[4, 2, 9])
    whole = marex_amd.event_occurrence(da, **kw)
    assert_equals_oracle(whole, exp, (ny, nx))
    assert host_engine.calls == [("occurrence", "int32", 0, T)]
    assert tuple(whole["occurrence"].dims) == ("lat", "lon") and tuple(whole["occurrence_by"].dims) == ("season", "lat", "lon")
    assert tuple(whole["presence"].dims) == ("zonal_month", "lat") and tuple(whole["local_duration"].dims) == ("event", "lat", "lon")
    assert np.array_equal(whole["occurrence"].coords["lat"].values, lat) and np.array_equal(whole["presence"].coords["lat"].values, lat)
    assert np.asarray(whole["occurrence_by"].coords["season"].values).tolist() == ["DJF", "JJA", "MAM", "SON"]
    assert np.asarray(whole["local_duration"].coords["event"].values).tolist() == [4, 2, 9]
    assert str(np.asarray(whole["presence"].coords["zonal_month"].values)[0])[:10] == "2003-01-01"
    for b in (1, 2, 3, T, "auto"):  # windows of 1, 2, 3 and T steps: the same Dataset
        host_engine.calls.clear()
        ds = marex_amd.event_occurrence(da, block_steps=b, **kw)
        assert list(ds.data_vars) == list(whole.data_vars)
        for k in whole.data_vars:
            assert np.asarray(ds[k].values).tobytes() == np.asarray(whole[k].values).tobytes(), (b, k)
        if b == 2:
            assert host_engine.calls == [("occurrence", "int32", a, min(2, T - a)) for a in range(0, T, 2)]
    # a bare int64 tensor, label arrays instead of names, no event_ids: the defaults' dimension names
    ds = marex_amd.event_occurrence(torch.from_numpy(ids.astype(np.int64).reshape(T, ny, nx)), by=season, zonal=True, zonal_by=months,
                                    block_steps=4)
    exp2 = {k: v for k, v in exp.items() if k != "local_duration"}
    exp2.update(oo.occurrence(ids.reshape(T, -1), season, 3, months, 12, cls, ny, np.full(ny, nx)))  # groups 0 .. max = 2
    assert_equals_oracle(ds, exp2, (ny, nx))
    assert tuple(ds["occurrence_by"].dims) == ("group", "y", "x") and tuple(ds["presence"].dims) == ("zonal_group", "y")


def test_masks_and_meshes_on_the_host_engine(host_engine):
    import torch

    T, C = 9, 77
    ids = case_field(T, 7, 11).reshape(T, C)
    mask = ids > 0
    rng = np.random.default_rng(2)
    lat = np.round(rng.uniform(-12, 12, C))
    edges = np.arange(-10.0, 11.0, 2.0)
    cls = oo.lat_bin(lat, edges)
    assert (cls < 0).any() and (lat == -10.0).any() and not (cls[lat == -10.0] >= 0).any()
    step = np.arange(T, dtype=np.int32)
    exp = oo.occurrence(mask, None, 1, step, T, cls, edges.size - 1, np.bincount(cls[cls >= 0], minlength=edges.size - 1))
    for f in (mask, mask.astype(np.uint8), torch.from_numpy(mask), DataArray(mask, dims=("time", "ncells"))):
        host_engine.calls.clear()
        ds = marex_amd.event_occurrence(f, zonal=True, zonal_by="step", lat=lat, lat_bins=edges, block_steps=4)
        assert_equals_oracle(ds, exp, (C,))
        assert [c[1] for c in host_engine.calls] == ["uint8"] * 3  # a mask travels at one byte per cell
    assert tuple(ds["occurrence"].dims) == ("ncells",) and tuple(ds["presence_cells"].dims) == ("zonal_step", "lat_bins")
    assert np.array_equal(ds["presence"].coords["lat_bins"].values, 0.5 * (edges[:-1] + edges[1:]))
    # a uint8 field may select a value; an ID field given as int16 is converted
    ds = marex_amd.event_occurrence(ids.astype(np.uint8), event_ids=[3])
    assert np.array_equal(ds["local_duration"].values[0], (ids == 3).sum(0))
    ds = marex_amd.event_occurrence(ids.astype(np.int16), event_ids=[3])
    assert np.array_equal(ds["local_duration"].values[0], (ids == 3).sum(0)) and host_engine.calls[-1][1] == "int32"
    with pytest.raises(DataValidationError, match="Object IDs must be non-negative"):
        marex_amd.event_occurrence(np.where(ids == 3, -1, ids).astype(np.int64))
    with pytest.raises(marex_amd.TrackingError, match=r"event_occurrence: needs .* GB of device memory, .* GB are free"):
        marex_amd.event_occurrence(np.zeros((8, 1 << 28), bool))
    empty = marex_amd.event_occurrence(np.zeros((0, 5), np.int32))
    assert np.asarray(empty["occurrence"].values).tolist() == [0] * 5 and np.isnan(np.asarray(empty["frequency"].values)).all()


def test_tracker_method_passes_the_field_and_the_mesh_latitudes(host_engine, monkeypatch):
    seen = {}
    monkeypatch.setattr(mo, "event_occurrence", lambda field, **kw: seen.update(field=field, **kw) or "ds")

    class T:  # the attributes the method reads
        device, unstructured_grid, lat = 0, True, np.arange(5.0)

    ds = marex_amd.Dataset({"ID_field": DataArray(np.zeros((2, 5), np.int32), dims=("time", "ncells"))})
    assert marex_amd.tracker.event_occurrence(T(), ds, zonal=True, lat_bins=[0, 2, 4]) == "ds"
    assert seen["field"] is ds["ID_field"] and seen["lat"].tolist() == [0, 1, 2, 3, 4] and seen["device"] == 0
    seen.clear()
    T.unstructured_grid = False
    marex_amd.tracker.event_occurrence(T(), ds, zonal=True, zonal_by="step", block_steps=3)
    assert "lat" not in seen and seen["block_steps"] == 3
