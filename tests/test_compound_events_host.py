"""Compound events on the host: the oracle against a plain per-cell, per-step loop, the refusals (raised before any device
work) and the public path -- labels, windows, the carried state, the joint mask, the host finish -- on a NumPy stand-in for
the engine call.  No GPU needed."""
import os
import sys

import numpy as np
import pytest
import torch

import marex_amd
import marex_amd._stream as ms
import marex_amd.compound as mc
from marex_amd.engine import HotPath
from marex_amd.exceptions import ConfigurationError, DataValidationError
from marex_amd.xr_compat import DataArray, Dataset

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import compound_cases as cc  # noqa: E402
import compound_oracle as co  # noqa: E402
import occurrence_oracle as oo  # noqa: E402
from compound_host_engine import HostEngine  # noqa: E402


# ------------------------------------------------------------------ the oracle against a plain loop
def loop_reference(A, B, L, K):
    """One cell and one step after the other, straight from the definitions; nothing shared with the oracle."""
    T, C = A.shape
    days = np.zeros((3, C), np.int64)
    lag = np.zeros((2 * L + 1, C), np.int64)
    runs = np.zeros((3, C), np.int64)  # open, begun, longest of the joint mask
    co_ = np.zeros((4, C), np.int64)
    for c in range(C):
        a, b = [bool(v) for v in A[:, c]], [bool(v) for v in B[:, c]]
        open_run = 0
        for t in range(T):
            days[0, c] += a[t]
            days[1, c] += b[t]
            days[2, c] += a[t] and b[t]
            if a[t] and b[t]:
                open_run += 1
                runs[1, c] += open_run == 1
                runs[2, c] = max(runs[2, c], open_run)
            else:
                open_run = 0
            for l in range(-L, L + 1):
                if 0 <= t + l < T and a[t] and b[t + l]:
                    lag[L + l, c] += 1
        runs[0, c] = open_run
        for row, (x, y) in ((0, (a, b)), (2, (b, a))):
            t = 0
            while t < T:
                if not x[t]:
                    t += 1
                    continue
                s = t
                while t + 1 < T and x[t + 1]:
                    t += 1
                e = t
                co_[row, c] += 1
                co_[row + 1, c] += any(y[u] for u in range(max(0, s - K), min(T - 1, e + K) + 1))
                t += 1
    return days, lag, runs, co_


TINY = {"random": lambda: cc.pair(23, 6, 0.4, 1), "sparse": lambda: cc.pair(40, 5, 0.1, 2), "shifted": lambda: cc.pair(31, 4, 0.3, 3, shift=3),
        "all present": lambda: cc.pair(9, 3, 1.0), "all absent": lambda: cc.pair(7, 2, 0.0), "one step": lambda: cc.pair(1, 4, 0.5, 4),
        "full against random": lambda: (cc.chain(17, 5, 1.0, 0), cc.chain(17, 5, 0.3, 9))}


@pytest.mark.parametrize("name", list(TINY))
def test_oracle_equals_a_plain_loop(name):
    A, B = TINY[name]()
    assert A.shape[0] <= 40 and A.shape[1] <= 6
    for L in (0, 1, 3, 30):
        for K in (0, 1, 3, 30):
            days, lag, runs, co_ = loop_reference(A, B, L, K)
            r = co.compound(A, B, L, K)
            assert np.array_equal(r["days"][:, 0], days) and r["days"].dtype == np.uint32, (L, K)
            assert np.array_equal(r["runs"], runs), (L, K)
            assert np.array_equal(r["co"], co_) and r["co"].dtype == np.uint32, (L, K)
            if L:
                assert np.array_equal(r["lag_days"], lag) and np.array_equal(r["lag_days"][L], days[2]), (L, K)
            else:
                assert r["lag_days"] is None
    if name == "all present":
        T = A.shape[0]
        r = co.compound(A, B, 3, 0)
        assert r["co"].tolist() == [[1] * 3] * 4 and r["runs"].tolist() == [[T] * 3, [1] * 3, [T] * 3]
        assert r["lag_days"][:, 0].tolist() == [T - 3, T - 2, T - 1, T, T - 1, T - 2, T - 3]
    if name == "all absent":
        assert not any(v.any() for v in loop_reference(A, B, 3, 3))


def test_oracle_on_hand_computed_cells():
    #            t: 0  1  2  3  4  5  6  7  8  9
    A = np.array([[0, 1, 1, 0, 0, 1, 0, 1, 0, 0]], bool).T
    B = np.array([[0, 0, 0, 0, 1, 0, 0, 0, 0, 1]], bool).T
    assert co.run_coincidence(A, B, 0)[:, 0].tolist() == [3, 0] and co.run_coincidence(B, A, 0)[:, 0].tolist() == [2, 0]
    assert co.run_coincidence(A, B, 1)[:, 0].tolist() == [3, 1]   # the run at 5 meets b at 4
    assert co.run_coincidence(A, B, 2)[:, 0].tolist() == [3, 3]   # [1, 2] meets 4; 7 meets 9
    assert co.run_coincidence(B, A, 1)[:, 0].tolist() == [2, 1] and co.run_coincidence(B, A, 2)[:, 0].tolist() == [2, 2]
    assert co.lag_days(A, B, 3)[:, 0].tolist() == [1, 0, 1, 0, 0, 2, 1]  # lags -3 .. 3: b - a = 3, 2, -1, -3 for b at 4, 2 for b at 9
    # the state: any cut gives the arrays of the whole
    whole = co.compound(A, B, 3, 2)
    for cut in (1, 4, 9):
        first = co.compound(A[:cut], B[:cut], 3, 2)
        second = co.compound(A[cut:], B[cut:], 3, 2, state=first["state"])
        for k in ("days", "runs", "co", "lag_days"):
            assert np.array_equal(second[k], whole[k]), (cut, k)


# ------------------------------------------------------------------ refusals before the device
def _days(n, start="2001-01-01"):
    return (np.datetime64(start) + np.arange(n)).astype("datetime64[ns]")


def _da(a, tv=None, dims=("time", "lat", "lon")):
    return DataArray(a, dims=dims, coords={dims[0]: (dims[0], np.arange(a.shape[0]) if tv is None else tv)})


def test_refusals_come_before_the_device(monkeypatch):
    import marex_amd.detect as det

    def no_gpu(*a, **k):
        raise AssertionError("the validation touched the GPU engine")

    monkeypatch.setattr(det, "get_engine", no_gpu)
    m = np.zeros((3, 4, 5), bool)
    mesh = np.zeros((3, 20), bool)
    lat = np.linspace(-9, 9, 20)
    V, Cf = DataValidationError, ConfigurationError
    cases = [
        (dict(field_b=np.zeros((3, 4, 6), bool)), V, "field_a and field_b differ in shape"),
        (dict(field_b=np.zeros((4, 4, 5), bool)), V, "field_a and field_b differ in shape"),
        (dict(field_b=mesh), V, "field_a and field_b differ in shape"),
        (dict(field_a=m[0, 0], field_b=m[0, 0]), V, r"field must be \(time, y, x\) or \(time, cells\)"),
        (dict(field_a=_da(m), field_b=_da(m, dims=("time", "y", "x"))), V, "field_a and field_b differ in their dimensions"),
        (dict(field_a=_da(m, dims=("time", "lon", "lat")), field_b=_da(m)), V, "field_a and field_b differ in their dimensions"),
        (dict(field_a=_da(m, _days(3)), field_b=_da(m, _days(3, "2001-01-02"))), V, "field_a and field_b differ in their time coordinate"),
        (dict(field_b=m.astype(np.float32)), V, "field must be a mask .* or an integer ID field"),
        (dict(field_a=m.astype(np.float64)), V, "field must be a mask .* or an integer ID field"),
        (dict(field_b=m.astype(np.complex64)), V, "field must be a mask"),
        (dict(by="week"), Cf, "by must be one of"),
        (dict(by="season"), V, "by='season' needs a datetime time coordinate"),
        (dict(field_a=_da(m), field_b=_da(m), by="month"), V, "by='month' needs a datetime time coordinate"),
        (dict(by=np.zeros(4, np.int32)), V, "by labels must be one integer per timestep"),
        (dict(zonal=True), V, "zonal_by='month' needs a datetime time coordinate"),
        (dict(zonal=True, zonal_by="step", lat=lat), V, "lat and lat_bins belong to a mesh"),
        (dict(zonal=True, zonal_by="step", lat_bins=[0, 1]), V, "lat and lat_bins belong to a mesh"),
        (dict(field_a=mesh, field_b=mesh, zonal=True, zonal_by="step"), V, "zonal presence on a mesh needs lat"),
    ]
    for name in ("max_lag", "tolerance"):
        cases += [(dict(**{name: v}), Cf, f"{name} must be an integer in 0 .. 30") for v in (-1, 31, 2.0, True, "3", None)]
    cases += [(dict(block_steps=b), Cf, "block_steps must be a positive number of timesteps, 'auto' or None") for b in (0, 2.5, "all")]
    for kw, cls, msg in cases:
        args = dict(field_a=m, field_b=m)
        args.update(kw)
        with pytest.raises(cls, match=msg):
            marex_amd.compound_events(**args)


def test_compound_events_is_public():
    assert "compound_events" in marex_amd.__all__ and marex_amd.compound_events is mc.compound_events
    assert hasattr(HotPath, "compound") and HotPath.COMPOUND_STATE_ROWS == mc.STATE_ROWS and HotPath.COMPOUND_MAX_LAG == mc.MAX_LAG
    from marex_amd import _lib

    assert "marex_compound_u8" in _lib.PROTOTYPES
    doc = marex_amd.compound_events.__doc__
    assert "negated variable" in doc and "threshold_percentile=5" in doc


# ------------------------------------------------------------------ the public path on the host engine
@pytest.fixture
def host_engine(monkeypatch):
    import marex_amd.detect as det

    eng = HostEngine()
    monkeypatch.setattr(det, "get_engine", lambda device=0: eng)
    monkeypatch.setattr(ms, "_free_bytes", lambda e: 1 << 30)
    return eng


DTYPES = {k: np.uint32 for k in ("days_a", "days_b", "days_both", "n_runs", "longest_run", "runs_a", "runs_a_coincident", "runs_b",
                                 "runs_b_coincident", "lag_days", "days_a_by", "days_b_by", "days_both_by")}
DTYPES.update({k: np.float64 for k in ("mean_run", "lmf", "jaccard", "coincidence_a", "coincidence_b", "lmf_by", "share_both")})
DTYPES.update({k: np.uint64 for k in ("cells_a", "cells_b", "cells_both")})
DTYPES.update(steps_by=np.int64, class_cells=np.int64)
NOT_SPATIAL = ("steps_by", "cells_a", "cells_b", "cells_both", "share_both", "class_cells")


def assert_equals_oracle(ds, exp, space):
    """Every variable the oracle has, and no other but the mask: dtype, shape (the oracle is flat in space), every value."""
    assert sorted(k for k in ds.data_vars if k != "compound_events") == sorted(exp)
    for k, want in exp.items():
        got = np.asarray(ds[k].values)
        assert got.dtype == DTYPES[k], (k, got.dtype)
        if k not in NOT_SPATIAL:
            assert got.shape[got.ndim - len(space):] == tuple(space), (k, got.shape)
            got = got.reshape(got.shape[:got.ndim - len(space)] + (-1,))
        assert got.shape == want.shape, (k, got.shape, want.shape)
        assert np.array_equal(got, want, equal_nan=got.dtype.kind == "f"), k


def same(x, y):
    assert list(x.data_vars) == list(y.data_vars)
    for k in x.data_vars:
        assert np.asarray(x[k].values).tobytes() == np.asarray(y[k].values).tobytes(), k
        assert tuple(x[k].dims) == tuple(y[k].dims), k


def test_grid_on_the_host_engine(host_engine):
    T, ny, nx, L, K = 40, 5, 13, 7, 2
    A, B = cc.pair(T, ny * nx, 0.3, 7)
    tv = _days(T, "2003-11-20")  # 11 days of November, 29 of December: two months, two seasons
    season, G, _, _ = marex_amd.occurrence.group_labels("season", tv, T)
    months, G2, _, _ = marex_amd.occurrence.zonal_labels("month", tv, T)
    assert G2 == 2 and set(season.tolist()) == {0, 3}
    cls = np.repeat(np.arange(ny, dtype=np.int32), nx)
    exp = co.variables(A, B, L, K, season, 4, months, G2, cls, ny, np.full(ny, nx))
    lat, lon = np.linspace(-30, 30, ny), np.linspace(0, 100, nx)
    coords = {"time": ("time", tv), "lat": ("lat", lat), "lon": ("lon", lon)}
    da, db = (DataArray(v.reshape(T, ny, nx), dims=("time", "lat", "lon"), coords=coords) for v in (A, B))
    kw = dict(max_lag=L, tolerance=K, by="season", zonal=True, zonal_by="month", return_mask=True)
    whole = marex_amd.compound_events(da, db, **kw)
    assert_equals_oracle(whole, exp, (ny, nx))
    assert host_engine.calls == [("compound", "uint8", "uint8", 0, T)]
    assert tuple(whole["days_both"].dims) == ("lat", "lon") and tuple(whole["lag_days"].dims) == ("lag", "lat", "lon")
    assert np.asarray(whole["lag_days"].coords["lag"].values).tolist() == list(range(-L, L + 1))
    assert tuple(whole["days_both_by"].dims) == ("season", "lat", "lon") and tuple(whole["share_both"].dims) == ("zonal_month", "lat")
    assert np.array_equal(whole["lmf"].coords["lat"].values, lat) and whole["steps_by"].values.tolist() == [29, 0, 0, 11]
    assert np.isnan(whole["lmf_by"].values[1]).all()
    m = whole["compound_events"]
    assert m.values.dtype == np.bool_ and isinstance(m.data, np.ndarray) and np.array_equal(m.values, (A & B).reshape(T, ny, nx))
    assert tuple(m.dims) == ("time", "lat", "lon") and np.array_equal(m.coords["time"].values, tv)
    # the identities
    assert np.array_equal(whole["lag_days"].values[L], whole["days_both"].values)
    assert (whole["runs_a_coincident"].values <= whole["runs_a"].values).all()
    assert (whole["runs_b_coincident"].values <= whole["runs_b"].values).all()
    assert (whole["days_both"].values <= np.minimum(whole["days_a"].values, whole["days_b"].values)).all()
    # windows: the same Dataset
    for bs in (1, 2, 7, "auto"):
        host_engine.calls.clear()
        same(whole, marex_amd.compound_events(da, db, block_steps=bs, **kw))
        if bs == 7:
            assert host_engine.calls == [("compound", "uint8", "uint8", a, min(7, T - a)) for a in range(0, T, 7)]
    # the composition: the joint statistics are event_occurrence of the joint mask, through its own host engine
    occ = marex_amd.event_occurrence(m, by="season", zonal=True, zonal_by="month")
    for k, j in (("days_both", "occurrence"), ("n_runs", "n_runs"), ("longest_run", "longest_run"), ("mean_run", "mean_run"),
                 ("days_both_by", "occurrence_by"), ("cells_both", "presence_cells"), ("share_both", "presence")):
        assert np.asarray(whole[k].values).tobytes() == np.asarray(occ[j].values).tobytes(), k
    occ = marex_amd.event_occurrence((A & B).reshape(T, ny, nx))
    assert np.array_equal(occ["occurrence"].values, whole["days_both"].values)
    assert np.array_equal(occ["n_runs"].values, whole["n_runs"].values) and np.array_equal(occ["longest_run"].values, whole["longest_run"].values)


def test_meshes_containers_and_types_on_the_host_engine(host_engine):
    T, C, L, K = 23, 77, 3, 1
    A, B = cc.pair(T, C, 0.4, 11)
    ids = np.where(B, np.arange(1, T * C + 1).reshape(T, C) % 9 + 1, 0).astype(np.int32)
    rng = np.random.default_rng(2)
    lat = np.round(rng.uniform(-12, 12, C))
    edges = np.arange(-10.0, 11.0, 2.0)
    cls = oo.lat_bin(lat, edges)
    step = np.arange(T, dtype=np.int32)
    by = (np.arange(T) // 5 % 3).astype(np.int32)
    exp = co.variables(A, B, L, K, by, 3, step, T, cls, edges.size - 1, np.bincount(cls[cls >= 0], minlength=edges.size - 1))
    kw = dict(max_lag=L, tolerance=K, by=by, zonal=True, zonal_by="step", lat=lat, lat_bins=edges, block_steps=4)
    pairs = [(A, B, ["uint8", "uint8"]), (A.astype(np.uint8) * 3, B, ["uint8", "uint8"]), (torch.from_numpy(A), torch.from_numpy(B), ["uint8", "uint8"]),
             (DataArray(A, dims=("time", "ncells")), DataArray(B, dims=("time", "ncells")), ["uint8", "uint8"]),
             (A, ids, ["uint8", "uint8"]), (A, ids.astype(np.int64), ["uint8", "uint8"]), (torch.from_numpy(ids), torch.from_numpy(A), None),
             (Dataset({"extreme_events": DataArray(A, dims=("time", "ncells")), "thresholds": DataArray(np.zeros(C), dims=("ncells",))}), B, None)]
    for fa, fb, kinds in pairs:
        host_engine.calls.clear()
        ds = marex_amd.compound_events(fa, fb, **kw)
        if fb is not B and fa is A:  # the ID field stands for B
            assert_equals_oracle(ds, exp, (C,))
        elif torch.is_tensor(fa) and fa.dtype == torch.int32:  # ... or for A, with the roles swapped
            assert np.array_equal(ds["days_a"].values, exp["days_b"]) and np.array_equal(ds["runs_a_coincident"].values, exp["runs_b_coincident"])
            assert np.array_equal(ds["lag_days"].values, exp["lag_days"][::-1])
        else:
            assert_equals_oracle(ds, exp, (C,))
        assert len(host_engine.calls) == 6 and all(c[0] == "compound" for c in host_engine.calls)
        if kinds:
            assert [list(c[1:3]) for c in host_engine.calls] == [kinds] * 6  # the kernel sees presence bytes only
    assert tuple(ds["days_a"].dims) == ("ncells",) and tuple(ds["cells_both"].dims) == ("zonal_step", "lat_bins")
    assert tuple(ds["days_a_by"].dims) == ("group", "ncells")
    # the mask: bool where both were bool, uint8 otherwise; a tensor when field_a was one
    for fa, fb, dt, tensor in ((A, B, np.bool_, False), (A.astype(np.uint8), B, np.uint8, False), (A, ids, np.uint8, False),
                               (torch.from_numpy(A), B, torch.bool, True), (torch.from_numpy(A), ids, torch.uint8, True),
                               (A, torch.from_numpy(B), np.bool_, False)):
        m = marex_amd.compound_events(fa, fb, return_mask=True, block_steps=5)["compound_events"].data
        assert torch.is_tensor(m) == tensor and m.dtype == dt and tuple(m.shape) == (T, C)
        assert np.array_equal(np.asarray(m).astype(bool), A & B)
    # a negative ID, in the first window or in a later one, on the host or in a tensor
    bad = ids.copy()
    bad[T - 1, 3] = -2
    for f in (bad, torch.from_numpy(bad), bad.astype(np.int64)):
        with pytest.raises(DataValidationError, match="Object IDs must be non-negative"):
            marex_amd.compound_events(A, f, block_steps=4)
    with pytest.raises(marex_amd.TrackingError, match=r"compound_events: needs .* GB of device memory, .* GB are free"):
        marex_amd.compound_events(np.zeros((8, 1 << 27), bool), np.zeros((8, 1 << 27), bool))
    with pytest.raises(marex_amd.TrackingError, match="block_steps='auto'"):
        marex_amd.compound_events(np.zeros((2, 1 << 25), bool), np.zeros((2, 1 << 25), bool), max_lag=30, block_steps=1)


def test_empty_records_touch_no_device(monkeypatch):
    import marex_amd.detect as det

    monkeypatch.setattr(det, "get_engine", lambda *a, **k: (_ for _ in ()).throw(AssertionError("touched the engine")))
    ds = marex_amd.compound_events(np.zeros((0, 5), bool), np.zeros((0, 5), np.uint8), max_lag=2, by=np.zeros(0, np.int32), return_mask=True)
    assert ds["days_both"].values.tolist() == [0] * 5 and np.isnan(ds["lmf"].values).all() and np.isnan(ds["jaccard"].values).all()
    assert ds["lag_days"].values.shape == (5, 5) and ds["compound_events"].values.shape == (0, 5)
    assert ds["compound_events"].values.dtype == np.uint8 and ds["days_both_by"].values.shape == (1, 5)
    ds = marex_amd.compound_events(np.zeros((4, 0), bool), np.zeros((4, 0), bool), zonal=True, zonal_by="step", lat=np.zeros(0),
                                   lat_bins=[0.0, 1.0], return_mask=True)
    assert ds["days_a"].values.shape == (0,) and ds["cells_both"].values.shape == (4, 1) and not ds["cells_both"].values.any()
    assert ds["compound_events"].values.shape == (4, 0) and ds["compound_events"].values.dtype == np.bool_


@pytest.mark.parametrize("k", [1, 3])
def test_a_shifted_copy_is_found_at_its_lag(host_engine, k):
    T, C = 37, 20
    A = cc.chain(T, C, 0.3, 21)
    A[T - k:] = False  # the copy of a run that starts later would lie past the record
    B = cc.shifted(A, k)
    ds = marex_amd.compound_events(A, B, max_lag=7, tolerance=k, block_steps=2)
    assert np.array_equal(ds["lag_days"].values[7 + k], A[:T - k].sum(0)) and ds["lag_days"].values[7 + k].sum() > 0
    started = (A & ~np.concatenate([np.zeros((1, C), bool), A[:-1]])).sum(0)
    assert np.array_equal(ds["runs_a"].values, started) and np.array_equal(ds["runs_a_coincident"].values, ds["runs_a"].values)
    # below the shift a one-step run at the record's end, or any run shorter than the shift, may stay alone
    fewer = marex_amd.compound_events(A, B, tolerance=0)
    assert (fewer["runs_a_coincident"].values <= ds["runs_a_coincident"].values).all()
    assert (fewer["runs_a_coincident"].values < ds["runs_a_coincident"].values).any()
