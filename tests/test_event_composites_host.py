"""Lagged composites on the host: the oracle against a naive triple loop and against literals on hand-made columns, the
refusals (raised before any device work) and the public path -- labels, windows with their halo, input types, the host
finish -- on a NumPy stand-in for the engine call.  No GPU needed."""
import math
import os
import sys

import numpy as np
import pytest
import torch

import marex_amd
import marex_amd._stream as ms
import marex_amd.composites as mp
from marex_amd.engine import HotPath
from marex_amd.exceptions import ConfigurationError, DataValidationError
from marex_amd.xr_compat import DataArray, Dataset

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import event_composites_cases as ec  # noqa: E402
import event_composites_oracle as eo  # noqa: E402
from event_composites_host_engine import HostEngine  # noqa: E402


# ------------------------------------------------------------------ the oracle against a plain loop
def loop_reference(X, V, L, anchor, grp=None, G=1):
    """One cell, one step and one lag after the other, in Python floats (doubles), straight from the definitions; nothing
    shared with the oracle."""
    T, C = X.shape
    W = 2 * L + 1
    anchors = [[0] * C for _ in range(G)]
    cnt = [[[0] * C for _ in range(W)] for _ in range(G)]
    tot = [[[0.0] * C for _ in range(W)] for _ in range(G)]
    sq = [[[0.0] * C for _ in range(W)] for _ in range(G)]
    for c in range(C):
        x = [bool(k) for k in X[:, c]]
        for t in range(T):
            if anchor == "onset":
                hit = t > 0 and x[t] and not x[t - 1]
            else:
                hit = t < T - 1 and x[t] and not x[t + 1]
            if not hit:
                continue
            g = 0 if grp is None else int(grp[t])
            anchors[g][c] += 1
            for lag in range(-L, L + 1):
                if 0 <= t + lag < T:
                    val = float(np.float32(V[t + lag, c]))
                    if math.isfinite(val):
                        cnt[g][lag + L][c] += 1
                        tot[g][lag + L][c] += val
                        sq[g][lag + L][c] += val * val
    return np.array(anchors, np.uint32).reshape(G, C), np.array(cnt, np.uint32).reshape(G, W, C), \
        np.array(tot, np.float64).reshape(G, W, C), np.array(sq, np.float64).reshape(G, W, C)


TINY = {"random": (12, 5, 0.4), "sparse": (12, 4, 0.15), "dense": (11, 5, 0.7), "all present": (9, 3, 1.0), "none present": (7, 2, 0.0),
        "one step": (1, 4, 0.5), "two steps": (2, 5, 0.5), "three steps": (3, 5, 0.5)}


@pytest.mark.parametrize("name", list(TINY))
@pytest.mark.parametrize("anchor", ec.ANCHORS)
def test_oracle_equals_a_plain_loop(name, anchor):
    T, C, cover = TINY[name]
    assert T <= 12 and C <= 5
    X = ec.chain(T, C, cover, 3 + T, mean_run=2.0)
    V = ec.values(T, C, T)
    grp = ec.labels(T, 3)
    for L in (0, 1, 3, 30):
        for g, G in ((None, 1), (grp, 3)):
            r = eo.composites(X, V, L, anchor, g, G)
            want = loop_reference(X, V, L, anchor, g, G)
            for k, w in zip(("anchors", "count", "sum", "sumsq"), want):
                assert r[k].dtype == w.dtype and r[k].tobytes() == w.tobytes(), (k, L, G)
            assert r["lost"] == 0
    if name in ("all present", "none present", "one step"):
        assert not eo.composites(X, V, 2, anchor)["anchors"].any()


def test_oracle_on_the_hand_made_columns():
    T = 12
    X = ec.edge_field(T)
    V = ec.values(T, X.shape[1], 1, special=False)  # finite: a count is the number of anchors whose step lies in the record
    for anchor in ec.ANCHORS:
        for L in ec.LAGS:
            assert eo.composites(X, V, L, anchor)["anchors"][0, :10].tolist() == ec.EDGE_ANCHORS[anchor], (anchor, L)
    on, end = eo.composites(X, V, 2, "onset")["count"][0], eo.composites(X, V, 2, "end")["count"][0]
    assert on[:, :10].T.tolist() == [[0] * 5, [1] * 5, [0, 1, 1, 1, 1], [2] * 5, [1] * 5, [0] * 5, [0] * 5, [1] * 5, [1] * 5, [1, 1, 1, 0, 0]]
    assert end[:, :10].T.tolist() == [[1] * 5, [0] * 5, [1, 1, 1, 1, 0], [2] * 5, [1] * 5, [0] * 5, [0] * 5, [1] * 5, [1] * 5, [0, 0, 1, 1, 1]]
    # T < 2 L + 1: the window of the one-step run at 5 leaves the record on both sides
    wide = eo.composites(X, V, 30, "onset")
    assert wide["count"][0, :, 4].tolist() == [0] * 25 + [1] * 12 + [0] * 24
    assert wide["sum"][0, 25:37, 4].tolist() == V[:, 4].astype(np.float64).tolist()
    # the two runs one step apart: lag 0 of the second anchor is lag +3 of the first
    r = eo.composites(X, V, 3, "onset")
    assert r["sum"][0, 3, 3] == float(V[4, 3]) + float(V[7, 3]) and r["sum"][0, 6, 3] == float(V[7, 3]) + float(V[10, 3])
    # a missing value is not counted, and nothing of it reaches the sums
    V2 = V.copy()
    V2[5, 4], V2[6, 4], V2[4, 4] = np.nan, np.inf, -np.inf
    r = eo.composites(X, V2, 1, "end")
    assert r["count"][0, :, 4].tolist() == [0, 0, 0] and r["sum"][0, :, 4].tolist() == [0.0] * 3 and r["anchors"][0, 4] == 1
    m, s, t = eo.derived(r["count"][0], r["sum"][0], r["sumsq"][0])
    assert np.isnan(m[:, 4]).all() and np.isnan(s[:, 4]).all() and np.isnan(t[:, 4]).all()


def test_derived_statistics():
    cnt = np.array([0, 1, 2, 3, 2], np.uint32)
    tot = np.array([0.0, 2.0, 4.0, 6.0, 4.0])
    sq = np.array([0.0, 4.0, 10.0, 14.0, 8.0])
    for fn in (eo.derived, mp.derived):
        m, s, t = fn(cnt, tot, sq)
        assert np.isnan(m[0]) and m[1:].tolist() == [2.0, 2.0, 2.0, 2.0]
        assert np.isnan(s[:2]).all() and s[2:].tolist() == [math.sqrt(2.0), 1.0, 0.0]
        assert np.isnan(t[:2]).all() and t[2] == 2.0 / (math.sqrt(2.0) / math.sqrt(2.0)) and t[3] == 2.0 / (1.0 / math.sqrt(3.0))
        assert np.isnan(t[4])  # no spread: no statistic


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
    v = np.zeros((3, 4, 5), np.float32)
    V, Cf = DataValidationError, ConfigurationError
    cases = [
        (dict(values=np.zeros((3, 4, 6), np.float32)), V, "field and values differ in shape"),
        (dict(values=np.zeros((4, 4, 5), np.float32)), V, "field and values differ in shape"),
        (dict(values=np.zeros((3, 20), np.float32)), V, "field and values differ in shape"),
        (dict(field=m[0, 0], values=v[0, 0]), V, r"field must be \(time, y, x\) or \(time, cells\)"),
        (dict(field=_da(m), values=_da(v, dims=("time", "y", "x"))), V, "field and values differ in their dimensions"),
        (dict(field=_da(m, dims=("time", "lon", "lat")), values=_da(v)), V, "field and values differ in their dimensions"),
        (dict(field=_da(m, _days(3)), values=_da(v, _days(3, "2001-01-02"))), V, "field and values differ in their time coordinate"),
        (dict(values=np.zeros((3, 4, 5), np.int32)), V, "values must be a floating-point field"),
        (dict(values=m), V, "values must be a floating-point field"),
        (dict(values=torch.zeros((3, 4, 5), dtype=torch.int64)), V, "values must be a floating-point field"),
        (dict(field=v), V, "field must be a mask .* or an integer ID field"),
        (dict(by="week"), Cf, "by must be one of"),
        (dict(by="season"), V, "by='season' needs a datetime time coordinate"),
        (dict(by=np.zeros(4, np.int32)), V, "by labels must be one integer per timestep"),
    ]
    cases += [(dict(max_lag=k), Cf, "max_lag must be an integer in 0 .. 30") for k in (-1, 31, 2.0, True, "3", None)]
    cases += [(dict(anchor=k), Cf, "anchor must be one of") for k in ("peak", "Onset", 0, None, ("onset",))]
    cases += [(dict(block_steps=b), Cf, "block_steps must be a positive number of timesteps, 'auto' or None") for b in (0, 2.5, "all")]
    for kw, cls, msg in cases:
        args = dict(field=m, values=v)
        args.update(kw)
        with pytest.raises(cls, match=msg):
            marex_amd.event_composites(**args)
    # the default names of the shared check keep their text
    with pytest.raises(V, match="dat_anomaly must be a floating-point field"):
        ms.plan_field(m, "local_intensity", np.zeros((3, 4, 5), np.int32))


def test_event_composites_is_public():
    assert "event_composites" in marex_amd.__all__ and marex_amd.event_composites is mp.event_composites
    assert "event_composites" in marex_amd.__doc__
    assert hasattr(marex_amd.tracker, "event_composites") and hasattr(HotPath, "event_composites")
    assert HotPath.COMPOSITES_MAX_LAG == 30 and HotPath.composites_rows(5, 9, 20, 0) == (4, 10)
    assert HotPath.composites_rows(5, 9, 20, 7) == (0, 16) and HotPath.composites_rows(0, 20, 20, 30) == (0, 20)
    from marex_amd import _lib
    from marex_amd.csrc import build

    assert "marex_event_composites_u8" in _lib.PROTOTYPES and "marex_composites" in build.UNITS
    doc = marex_amd.event_composites.__doc__
    for words in ("hobday_events", "two different IDs on adjacent steps", "censored", "composite_sum / n", "Out of scope", "peak"):
        assert words in doc, words
    assert mp.accumulator_bytes(4, 100, 10) == 4 * 100 * (4 + 20 * 21)


# ------------------------------------------------------------------ the public path on the host engine
@pytest.fixture
def host_engine(monkeypatch):
    import marex_amd.detect as det

    eng = HostEngine()
    monkeypatch.setattr(det, "get_engine", lambda device=0: eng)
    monkeypatch.setattr(ms, "_free_bytes", lambda e: 1 << 30)
    return eng


DTYPES = {"anchors": np.uint32, "anchors_by": np.uint32, "steps_by": np.int64}
for _k in ("count", "sum", "sumsq", "mean", "std", "t"):
    for _s in ("", "_by"):
        DTYPES[f"composite_{_k}{_s}"] = np.uint32 if _k == "count" else np.float64


def assert_equals_oracle(ds, exp, space):
    """Every variable the oracle has, and no other: dtype, shape (the oracle is flat in space), every byte."""
    assert sorted(ds.data_vars) == sorted(exp)
    for k, want in exp.items():
        got = np.asarray(ds[k].values)
        assert got.dtype == DTYPES[k] == want.dtype, (k, got.dtype)
        if k != "steps_by":
            assert got.shape[got.ndim - len(space):] == tuple(space), (k, got.shape)
            got = got.reshape(got.shape[:got.ndim - len(space)] + (-1,))
        assert got.shape == want.shape, (k, got.shape, want.shape)
        assert np.ascontiguousarray(got).tobytes() == want.tobytes(), k


def same(x, y):
    assert list(x.data_vars) == list(y.data_vars)
    for k in x.data_vars:
        assert np.asarray(x[k].values).tobytes() == np.asarray(y[k].values).tobytes(), k
        assert tuple(x[k].dims) == tuple(y[k].dims), k


@pytest.mark.parametrize("anchor", ec.ANCHORS)
@pytest.mark.parametrize("L", [0, 1, 10, 30])
def test_grid_on_the_host_engine(host_engine, anchor, L):
    T, ny, nx = 40, 3, 7
    X = ec.chain(T, ny * nx, 0.3, 7 + L, mean_run=3.0)
    X[:, :10] = ec.edge_field(T)[:, :10]
    V = ec.values(T, ny * nx, L)
    tv = _days(T, "2003-12-10")  # 22 days of December, 18 of January: two years, one season
    coords = {"time": ("time", tv), "lat": ("lat", np.linspace(-30, 30, ny)), "lon": ("lon", np.linspace(0, 100, nx))}
    dx, dv = (DataArray(a.reshape(T, ny, nx), dims=("time", "lat", "lon"), coords=coords) for a in (X, V))
    year, Gy, _, yvals = marex_amd.occurrence.group_labels("year", tv, T)
    season, Gs, _, _ = marex_amd.occurrence.group_labels("season", tv, T)
    assert Gy == 2 and yvals.tolist() == [2003, 2004] and Gs == 4
    labels = ec.labels(T, 5)
    for by, grp, G, gname in ((None, None, 1, None), ("year", year, 2, "year"), ("season", season, 4, "season"), (labels, labels, 5, "group")):
        exp = eo.variables(X, V, L, anchor, grp, G)
        host_engine.calls.clear()
        whole = marex_amd.event_composites(dx, dv, max_lag=L, anchor=anchor, by=by)
        assert_equals_oracle(whole, exp, (ny, nx))
        assert host_engine.calls == [("event_composites", "uint8", 0, T, 0, T)]
        sfx, lead = ("", ()) if by is None else ("_by", (gname,))
        assert tuple(whole["anchors"].dims) == ("lat", "lon") and tuple(whole["composite_sum" + sfx].dims) == lead + ("lag", "lat", "lon")
        assert np.asarray(whole["composite_t" + sfx].coords["lag"].values).tolist() == list(range(-L, L + 1))
        assert whole["composite_t" + sfx].coords["lag"].values.dtype == np.int64
        assert np.array_equal(whole["composite_mean" + sfx].coords["lat"].values, coords["lat"][1])
        assert whole["anchors"].values.reshape(-1)[:10].tolist() == ec.EDGE_ANCHORS[anchor]
        if by is not None:
            assert tuple(whole["anchors_by"].dims) == (gname, "lat", "lon") and "composite_mean" not in whole.data_vars
            assert int(whole["steps_by"].values.sum()) == T
        for bs in (1, 3, 7, "auto"):  # windows: the same bytes
            host_engine.calls.clear()
            same(whole, marex_amd.event_composites(dx, dv, max_lag=L, anchor=anchor, by=by, block_steps=bs))
            if bs == 7:
                H = max(L, 1)
                assert host_engine.calls == [("event_composites", "uint8", max(0, a - H), min(T, a + 7 + H) - max(0, a - H), a, min(T, a + 7))
                                             for a in range(0, T, 7)]


def test_meshes_containers_and_types_on_the_host_engine(host_engine):
    T, C, L = 23, 77, 3
    X = ec.edge_field(T, C, seed=11)
    V = ec.values(T, C, 2)
    ids = np.where(X, np.arange(1, T * C + 1).reshape(T, C) % 9 + 1, 0).astype(np.int32)  # the ID changes inside every run
    by = ec.labels(T, 3)
    for anchor in ec.ANCHORS:
        exp = eo.variables(X, V, L, anchor, by, 3)
        assert eo.variables(ids, V, L, anchor, by, 3)["composite_sum_by"].tobytes() == exp["composite_sum_by"].tobytes()
        fields = [X, X.astype(np.uint8) * 3, ids, ids.astype(np.int64), torch.from_numpy(X), torch.from_numpy(ids), torch.from_numpy(ids.astype(np.int64)),
                  DataArray(X, dims=("time", "ncells")),
                  Dataset({"extreme_events": DataArray(X, dims=("time", "ncells")), "thresholds": DataArray(np.zeros(C), dims=("ncells",))})]
        vals = [V, V.astype(np.float64), torch.from_numpy(V), DataArray(V, dims=("time", "ncells"))]
        for i, f in enumerate(fields):
            host_engine.calls.clear()
            ds = marex_amd.event_composites(f, vals[i % len(vals)], max_lag=L, anchor=anchor, by=by, block_steps=4)
            assert_equals_oracle(ds, exp, (C,))
            assert len(host_engine.calls) == 6 and all(c[1] == "uint8" for c in host_engine.calls)  # the kernel sees presence bytes only
        assert tuple(ds["anchors"].dims) == ("ncells",) and tuple(ds["composite_count_by"].dims) == ("group", "lag", "ncells")
    # float64 values are read as float32
    big = V.astype(np.float64) * (1 + 2.0 ** -40)
    same(marex_amd.event_composites(X, big), marex_amd.event_composites(X, big.astype(np.float32)))
    # a negative ID, in the first window or in a later one, on the host or in a tensor
    bad = ids.copy()
    bad[T - 1, 3] = -2
    for f in (bad, torch.from_numpy(bad), bad.astype(np.int64)):
        with pytest.raises(DataValidationError, match="Object IDs must be non-negative"):
            marex_amd.event_composites(f, V, block_steps=4)
    with pytest.raises(marex_amd.TrackingError, match=r"event_composites: needs .* GB of device memory, .* GB are free"):
        marex_amd.event_composites(np.zeros((2, 1 << 26), bool), np.zeros((2, 1 << 26), np.float32), max_lag=0)
    with pytest.raises(marex_amd.TrackingError, match="block_steps='auto'"):
        marex_amd.event_composites(np.zeros((2, 1 << 21), bool), np.zeros((2, 1 << 21), np.float32), max_lag=30, block_steps=1)


def test_empty_records_touch_no_device(monkeypatch):
    import marex_amd.detect as det

    monkeypatch.setattr(det, "get_engine", lambda *a, **k: (_ for _ in ()).throw(AssertionError("touched the engine")))
    ds = marex_amd.event_composites(np.zeros((0, 5), bool), np.zeros((0, 5), np.float32), max_lag=2)
    assert ds["anchors"].values.tolist() == [0] * 5 and ds["anchors"].values.dtype == np.uint32
    assert ds["composite_count"].values.shape == (5, 5) and not ds["composite_count"].values.any() and not ds["composite_sum"].values.any()
    for k in ("composite_mean", "composite_std", "composite_t"):
        assert ds[k].values.shape == (5, 5) and np.isnan(ds[k].values).all() and ds[k].values.dtype == np.float64
    ds = marex_amd.event_composites(np.zeros((0, 2, 3), np.int32), np.zeros((0, 2, 3)), max_lag=1, by=np.zeros(0, np.int32), anchor="end")
    assert ds["anchors_by"].values.shape == (1, 2, 3) and ds["composite_sumsq_by"].values.shape == (1, 3, 2, 3)
    assert np.isnan(ds["composite_t_by"].values).all() and ds["steps_by"].values.tolist() == [0]
    ds = marex_amd.event_composites(np.zeros((4, 0), bool), np.zeros((4, 0), np.float32), max_lag=30, by=np.array([0, 0, 1, 1]))
    assert ds["anchors"].values.shape == (0,) and ds["composite_mean_by"].values.shape == (2, 61, 0) and ds["steps_by"].values.tolist() == [2, 2]


def test_tracker_method_takes_the_id_field(monkeypatch):
    seen = {}
    monkeypatch.setattr(mp, "event_composites", lambda field, values, **kw: seen.update(field=field, values=values, **kw) or "ds")

    class T:  # the attribute the method reads
        device = 3

    ev = marex_amd.Dataset({"ID_field": DataArray(np.zeros((2, 5), np.int32), dims=("time", "ncells"))})
    flux = DataArray(np.zeros((2, 5), np.float32), dims=("time", "ncells"))
    assert marex_amd.tracker.event_composites(T(), ev, flux, max_lag=4, anchor="end") == "ds"
    assert seen["field"] is ev["ID_field"] and seen["values"] is flux and seen["device"] == 3 and seen["max_lag"] == 4 and seen["anchor"] == "end"
    seen.clear()
    mask = np.zeros((2, 5), bool)
    marex_amd.tracker.event_composites(T(), mask, flux, device=1, by="year")
    assert seen["field"] is mask and seen["device"] == 1 and seen["by"] == "year"


def test_tracker_method_on_the_host_engine(host_engine):
    T, C = 15, 12
    X = ec.edge_field(T, C)
    V = ec.values(T, C, 4)

    class Trk:
        device = 0

    ev = marex_amd.Dataset({"ID_field": DataArray(np.where(X, 7, 0).astype(np.int32), dims=("time", "ncells"))})
    ds = marex_amd.tracker.event_composites(Trk(), ev, DataArray(V, dims=("time", "ncells")), max_lag=2, block_steps=4)
    assert_equals_oracle(ds, eo.variables(X, V, 2), (C,))
