"""GPU parity: lagged composites (``marex_event_composites_u8`` through ``HotPath.call``, ``HotPath.event_composites`` and
``marex_amd.event_composites``) against the NumPy oracle of tests/event_composites_oracle.py.  The counts are integers and
the sums are float64 additions in a fixed order, so everything compares by its bytes: partial waves and several blocks,
record lengths around the unroll depth and around ``2 L + 1``, both anchors, the windows with their halo, step labels,
missing values, input types and residency, and the guards."""
import os
import sys

import numpy as np
import pytest
import torch

import marex_amd
from marex_amd.exceptions import DataValidationError, ProcessingError
from marex_amd.xr_compat import DataArray, Dataset

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import event_composites_cases as ec  # noqa: E402
import event_composites_oracle as eo  # noqa: E402

pytestmark = pytest.mark.gpu
FN = "marex_event_composites_u8"
CODE = {"onset": 0, "end": 1}


def to_dev(hot, a, dtype=np.uint8, misaligned=False):
    """A copy of ``a`` on the device; ``misaligned`` (bytes only): a contiguous view one byte past an aligned address."""
    a = np.ascontiguousarray(a).astype(dtype)
    if not misaligned:
        return torch.from_numpy(a).to(hot.device)
    buf = torch.zeros(a.size + 16, dtype=torch.uint8, device=hot.device)
    v = buf[1:1 + a.size].view(a.shape)
    v.copy_(torch.from_numpy(a))
    assert v.data_ptr() % 4 == 1 and v.is_contiguous()
    return v


def buffers(hot, C, L, G, grp):
    """Buffers of the test's own: zeroed accumulators with one spare plane behind each as a canary."""
    z = lambda shape, dt: torch.zeros(shape, dtype=dt, device=hot.device)  # noqa: E731
    W = 2 * L + 1
    return {"anchors": z((G + 1, C), torch.int32), "cnt": z((G + 1, C, W), torch.int32), "sum": z((G + 1, C, W), torch.float64),
            "sumsq": z((G + 1, C, W), torch.float64), "status": z((2,), torch.int64),
            "grp": None if grp is None else torch.from_numpy(np.asarray(grp, np.int32)).to(hot.device)}


def kernel(hot, x, v, r0, a, b, T, L, anchor, G, bufs):
    Tr, C = x.shape
    hot.call(FN, x, v, r0, Tr, a, b, T, C, L, CODE[anchor], bufs["grp"], G, bufs["anchors"], bufs["sum"], bufs["sumsq"], bufs["cnt"],
             bufs["status"])


def read(bufs):
    out = {k: bufs[k].cpu().numpy() for k in ("anchors", "cnt", "sum", "sumsq", "status")}
    for k in ("anchors", "cnt", "sum", "sumsq"):  # the canaries
        assert not out[k][-1].view(np.uint8).any(), k
    assert out["status"][1] == 0
    lags_first = lambda a: np.ascontiguousarray(a[:-1].transpose(0, 2, 1))  # noqa: E731
    return {"anchors": out["anchors"][:-1].view(np.uint32), "count": lags_first(out["cnt"]).view(np.uint32), "sum": lags_first(out["sum"]),
            "sumsq": lags_first(out["sumsq"]), "lost": int(out["status"][0])}


def run(hot, X, V, L, anchor="onset", grp=None, G=1, cuts=None, misaligned=False):
    """The kernel over the windows between ``cuts`` (None: one call), each with the rows of its halo and no others."""
    T, C = X.shape
    bufs = buffers(hot, C, L, G, grp)
    cuts = [0, T] if cuts is None else cuts
    H = max(L, 1)
    for a, b in zip(cuts[:-1], cuts[1:]):
        lo, hi = max(0, a - H), min(T, b + H)
        kernel(hot, to_dev(hot, X[lo:hi], np.uint8, misaligned), to_dev(hot, V[lo:hi], np.float32), lo, a, b, T, L, anchor, G, bufs)
    return read(bufs)


def check(hot, X, V, L, anchor="onset", grp=None, G=1, cuts=None, misaligned=False):
    """The kernel on ``X``, ``V`` against the oracle: every output byte for byte, the status word."""
    got = run(hot, X, V, L, anchor, grp, G, cuts, misaligned)
    want = eo.composites(X, V, L, anchor, grp, G)
    what = (X.shape, L, anchor, cuts)
    for k in ("anchors", "count", "sum", "sumsq"):
        assert got[k].dtype == want[k].dtype and got[k].shape == want[k].shape and got[k].tobytes() == want[k].tobytes(), (k, what)
    assert got["lost"] == want["lost"], what
    return got, want


@pytest.mark.parametrize("C", ec.CELLS)
def test_cells_and_times_equal_the_oracle(hot, C):
    """Partial waves, full ones and several blocks at every length around the unroll depth and around ``2 L + 1``, both
    anchors, with groups that change inside a batch of rows and without labels."""
    total = 0
    for T in ec.TIMES:
        X = ec.chain(T, C, 0.4, seed=T, mean_run=2.0)
        V = ec.values(T, C, T)
        for L in ec.LAGS:
            for anchor in ec.ANCHORS:
                grp, G = (ec.labels(T), 4) if (L + T) % 2 else (None, 1)
                got, _ = check(hot, X, V, L, anchor, grp, G)
                total += int(got["anchors"].sum())
                if T == 1:
                    assert not got["anchors"].any() and not got["count"].any()
    assert total > 0


@pytest.mark.parametrize("anchor", ec.ANCHORS)
@pytest.mark.parametrize("L,T", [(30, 72), (30, 12), (7, 26), (1, 12), (0, 12)])
def test_windows_do_not_matter(hot, L, T, anchor):
    """On the hand-made columns: every single cut, windows of one step, windows shorter than the lag -- the bytes of the one
    call.  The labels change at window edges and inside windows; the presence bytes once from a view one byte past an
    aligned address."""
    C = 1028
    X = ec.edge_field(T, C)
    V = ec.values(T, C, L + T)
    grp = ec.labels(T)
    whole, want = check(hot, X, V, L, anchor, grp, 4)
    assert whole["anchors"].sum(0)[:10].tolist() == ec.EDGE_ANCHORS[anchor]
    splits = [list(range(T + 1)), list(range(0, T, 3)) + [T], list(range(0, T, 7)) + [T]] + [[0, s, T] for s in range(1, T)]
    for i, cuts in enumerate(splits):
        got = run(hot, X, V, L, anchor, grp, 4, cuts=cuts, misaligned=i == 1)
        for k in ("anchors", "count", "sum", "sumsq"):
            assert got[k].tobytes() == whole[k].tobytes(), (k, cuts)
        assert got["lost"] == 0


def test_hand_made_columns_as_literals(hot):
    T, C = 12, 1028
    X = ec.edge_field(T, C)
    V = ec.values(T, C, 1, special=False)
    on, _ = check(hot, X, V, 2, "onset")
    end, _ = check(hot, X, V, 2, "end")
    assert on["anchors"][0, :10].tolist() == ec.EDGE_ANCHORS["onset"] and end["anchors"][0, :10].tolist() == ec.EDGE_ANCHORS["end"]
    assert on["count"][0][:, :10].T.tolist() == [[0] * 5, [1] * 5, [0, 1, 1, 1, 1], [2] * 5, [1] * 5, [0] * 5, [0] * 5, [1] * 5, [1] * 5,
                                                 [1, 1, 1, 0, 0]]
    assert end["count"][0][:, :10].T.tolist() == [[1] * 5, [0] * 5, [1, 1, 1, 1, 0], [2] * 5, [1] * 5, [0] * 5, [0] * 5, [1] * 5, [1] * 5,
                                                  [0, 0, 1, 1, 1]]
    wide, _ = check(hot, X, V, 30, "onset")  # T < 2 L + 1: the window leaves the record on both sides
    assert wide["count"][0, :, 4].tolist() == [0] * 25 + [1] * 12 + [0] * 24
    assert wide["sum"][0, 25:37, 4].tolist() == V[:, 4].astype(np.float64).tolist()


@pytest.mark.parametrize("cover", ec.COVERAGES)
def test_coverage(hot, cover):
    """Nothing present, a few per cent, half, everything (every run touches both edges: censored)."""
    T, C = 41, 1028
    X = ec.chain(T, C, cover, seed=1)
    V = ec.values(T, C, 9)
    for anchor in ec.ANCHORS:
        for L in (7, 30):
            got, _ = check(hot, X, V, L, anchor, ec.labels(T), 4)
            if cover in (0.0, 1.0):
                assert not got["anchors"].any() and not got["count"].any() and not got["sum"].view(np.uint8).any()
            else:
                assert got["anchors"].any()


def test_missing_values(hot):
    T, C = 23, 257
    X = ec.chain(T, C, 0.4, seed=3, mean_run=2.0)
    for fill in (np.nan, np.inf, -np.inf):
        got, want = check(hot, X, np.full((T, C), fill, np.float32), 7, "onset")
        assert got["anchors"].any() and not got["count"].any() and not got["sum"].view(np.uint8).any() and not got["sumsq"].view(np.uint8).any()
    V = np.full((T, C), np.nan, np.float32)
    V[::2] = -0.0  # signed zeros are values: counted, and 0.0 + -0.0 is +0.0
    got, _ = check(hot, X, V, 7, "end")
    assert got["count"].any() and not got["sum"].view(np.uint8).any()


def test_labels(hot):
    T, C = 19, 1027
    X = ec.chain(T, C, 0.4, seed=2, mean_run=2.0)
    V = ec.values(T, C, 2)
    every_row = np.arange(T, dtype=np.int32)
    for anchor in ec.ANCHORS:
        check(hot, X, V, 3, anchor, every_row, T)  # one group per step
        check(hot, X, V, 3, anchor, None, 1)       # NULL grp
        check(hot, X, V, 3, anchor, np.zeros(T, np.int32), 1)
        # labels outside the range address nothing (read() checks the spare planes) and are counted
        grp = np.array([0, 1, 2, 7, -1, 1, 3, 2] + [0] * (T - 8), np.int32)
        got, _ = check(hot, X, V, 7, anchor, grp, 3, cuts=[0, 4, 5, T])
        assert got["lost"] > 0
        with pytest.raises(ProcessingError, match=r"event_composites: \d+ anchors lie under a step label outside its range"):
            hot.event_composites(to_dev(hot, X), to_dev(hot, V, np.float32), 0, 0, T, T, max_lag=7, anchor=anchor, grp=grp, G=3)


def test_return_codes(hot):
    T, C, L = 9, 1028, 2
    X = ec.chain(T, C, 0.4, seed=6, mean_run=2.0)
    V = ec.values(T, C, 6)
    x, v = to_dev(hot, X), to_dev(hot, V, np.float32)
    grp = ec.labels(T)
    bufs = buffers(hot, C, L, 4, grp)
    names = ("x", "v", "r0", "Tr", "a", "b", "T", "C", "L", "anchor", "grp", "G", "anchors", "sum", "sumsq", "cnt", "status")
    ok = (x, v, 0, T, 0, T, T, C, L, 0, bufs["grp"], 4, bufs["anchors"], bufs["sum"], bufs["sumsq"], bufs["cnt"], bufs["status"])

    def with_(**kw):
        return tuple(kw.get(k, val) for k, val in zip(names, ok))

    odd = lambda t, k: t.data_ptr() + k  # noqa: E731  (an address that is not aligned to the element)
    cases = [(-4, with_(C=2**31 - 1)), (-4, with_(T=2**31 - 1)), (-4, with_(C=2**31))]
    cases += [(-1, with_(**{k: None})) for k in ("x", "v", "anchors", "sum", "sumsq", "cnt", "status")]
    cases += [(-1, with_(C=0)), (-1, with_(C=-1)), (-1, with_(G=0)), (-1, with_(G=-1)), (-1, with_(grp=None)), (-1, with_(L=-1)), (-1, with_(L=31)),
              (-1, with_(anchor=-1)), (-1, with_(anchor=2)), (-1, with_(r0=-1)), (-1, with_(Tr=T + 1)), (-1, with_(Tr=-1)), (-1, with_(r0=1)),
              (-1, with_(a=-1)), (-1, with_(a=5, b=4)), (-1, with_(b=T + 1)), (-1, with_(T=T - 1)),
              (-1, with_(Tr=T - 1)),                    # the last row is missing
              (-1, with_(r0=1, Tr=T - 1)),              # the first row is missing
              (-1, with_(r0=3, Tr=3, a=4, b=5)),        # L = 2: the rows 2 .. 6 are needed
              (-1, with_(r0=2, Tr=4, a=4, b=5)),
              (-1, with_(L=0, r0=4, Tr=2, a=4, b=5)),   # L = 0 still needs the neighbour rows 3 and 5
              (-1, with_(L=0, r0=3, Tr=2, a=4, b=5)),
              (-1, with_(v=odd(v, 2))), (-1, with_(grp=odd(bufs["grp"], 1))), (-1, with_(anchors=odd(bufs["anchors"], 2))),
              (-1, with_(cnt=odd(bufs["cnt"], 1))), (-1, with_(sum=odd(bufs["sum"], 4))), (-1, with_(sumsq=odd(bufs["sumsq"], 4))),
              (-1, with_(status=odd(bufs["status"], 4)))]
    for code, args in cases:  # refused by the library before any launch
        with pytest.raises(ProcessingError, match=rf"{FN} failed \(code {code}\)"):
            hot.call(FN, *args)
    hot.sync()
    assert not any(bufs[k].view(torch.uint8).any() for k in ("anchors", "cnt", "sum", "sumsq", "status"))
    assert np.array_equal(x.cpu().numpy(), X.astype(np.uint8)) and v.cpu().numpy().tobytes() == V.tobytes()
    for args in (with_(a=3, b=3), with_(a=3, b=3, r0=0, Tr=0), with_(a=0, b=0), with_(a=T, b=T)):  # a == b does nothing
        hot.call(FN, *args)
    hot.sync()
    assert not any(bufs[k].view(torch.uint8).any() for k in ("anchors", "cnt", "sum", "sumsq", "status"))
    # the valid variants run
    want = eo.composites(X, V, L, "onset", grp, 4)
    hot.call(FN, *ok)
    assert read(bufs)["sum"].tobytes() == want["sum"].tobytes()
    for kw, w in ((dict(grp=None, G=1), eo.composites(X, V, L, "end")), (dict(L=0, grp=None, G=1), eo.composites(X, V, 0, "end")),
                  (dict(L=0, r0=3, Tr=3, a=4, b=5), None), (dict(r0=2, Tr=5, a=4, b=5), None)):
        b2 = buffers(hot, C, kw.get("L", L), kw.get("G", 4), grp)
        b2["grp"] = bufs["grp"] if "grp" not in kw else None
        args = dict(zip(names, with_(anchor=1, **kw)))
        args.update(anchors=b2["anchors"], sum=b2["sum"], sumsq=b2["sumsq"], cnt=b2["cnt"], status=b2["status"], grp=b2["grp"])
        if "r0" in kw:  # one step's anchors from the rows of its halo alone
            args.update(x=to_dev(hot, X[kw["r0"]:kw["r0"] + kw["Tr"]]), v=to_dev(hot, V[kw["r0"]:kw["r0"] + kw["Tr"]], np.float32))
            w = eo.accumulate(eo.zeros(4, C, kw.get("L", L)), X, V, 0, 4, 5, T, kw.get("L", L), "end", grp, 4)
        hot.call(FN, *(args[k] for k in names))
        got = read(b2)
        for k in ("anchors", "count", "sum", "sumsq"):
            assert got[k].tobytes() == w[k].tobytes(), (k, kw)


def test_engine_contract(hot):
    """``HotPath.event_composites``: poisoned fresh buffers, windows through ``acc``, the deferred read, the refusals."""
    from marex_amd.engine import HotPath

    assert HotPath.POISON
    T, C, L = 23, 1028, 7
    X = ec.edge_field(T, C)
    V = ec.values(T, C, 4)
    grp = ec.labels(T)
    for anchor in ec.ANCHORS:
        want = eo.composites(X, V, L, anchor, grp, 4)
        acc = None
        for a in range(0, T, 5):
            b = min(T, a + 5)
            lo, hi = HotPath.composites_rows(a, b, T, L)
            r = hot.event_composites(to_dev(hot, X[lo:hi]).view(torch.bool) if a else to_dev(hot, X[lo:hi]), to_dev(hot, V[lo:hi], np.float32),
                                     lo, a, b, T, max_lag=L, anchor=anchor, grp=grp, G=4, acc=acc, finish=b == T)
            acc = r["acc"]
            assert (b == T) == ("sum" in r)
        for k in ("anchors", "count", "sum", "sumsq"):
            assert r[k].dtype == want[k].dtype and r[k].shape == want[k].shape and r[k].tobytes() == want[k].tobytes(), k
    x, v = to_dev(hot, X), to_dev(hot, V, np.float32)
    plain = hot.event_composites(x, v, 0, 0, T, T)
    assert plain["count"].shape == (1, 21, C) and plain["sum"].tobytes() == eo.composites(X, V, 10)["sum"].tobytes()
    ev = hot.event_composites
    for bad in (lambda: ev(x.to(torch.int32), v, 0, 0, T, T), lambda: ev(x, v.to(torch.float64), 0, 0, T, T), lambda: ev(x, v[:-1], 0, 0, T, T),
                lambda: ev(x.t(), v.t(), 0, 0, T, T), lambda: ev(x, v.cpu(), 0, 0, T, T), lambda: ev(x, v, -1, 0, T, T), lambda: ev(x, v, 0, 0, T, T - 1),
                lambda: ev(x, v, 0, 3, 3, T), lambda: ev(x, v, 0, 5, 4, T), lambda: ev(x, v, 0, 0, T + 1, T + 1), lambda: ev(x, v, 0, 0, T, T, G=2),
                lambda: ev(x, v, 0, 0, T, T, max_lag=31), lambda: ev(x, v, 0, 0, T, T, max_lag=-1), lambda: ev(x, v, 0, 0, T, T, max_lag=1.0),
                lambda: ev(x, v, 0, 0, T, T, anchor="peak"), lambda: ev(x, v, 0, 0, T, T, anchor=0), lambda: ev(x, v, 0, 0, T, T, grp=grp[:3], G=4),
                lambda: ev(x, v, 0, 0, T, T, grp=grp.astype(np.float32), G=4),
                lambda: ev(x[4:9], v[4:9].contiguous(), 4, 5, 8, T, max_lag=2),   # the halo starts at row 3
                lambda: ev(x[3:9], v[3:9].contiguous(), 3, 5, 8, T, max_lag=2),   # ... and ends after row 9
                lambda: ev(x[5:8], v[5:8].contiguous(), 5, 5, 8, T, max_lag=0),   # max_lag = 0 still needs the neighbour rows
                lambda: ev(x, v, 0, 0, T, T, max_lag=3, acc=ev(x, v, 0, 0, T, T, max_lag=2, finish=False)["acc"]),
                lambda: ev(x, v, 0, 0, T, T, anchor="end", acc=ev(x, v, 0, 0, T, T, finish=False)["acc"])):
        with pytest.raises(ProcessingError):
            bad()
    ok = ev(x[3:10], v[3:10].contiguous(), 3, 5, 8, T, max_lag=2)  # exactly the halo
    w = eo.accumulate(eo.zeros(1, C, 2), X, V, 0, 5, 8, T, 2)
    assert ok["sum"].tobytes() == w["sum"].tobytes() and ok["anchors"].tobytes() == w["anchors"].tobytes()


# ------------------------------------------------------------------ the public call
def same(x, y):
    assert list(x.data_vars) == list(y.data_vars)
    for k in x.data_vars:
        xv, yv = (np.asarray(d[k].values) for d in (x, y))
        assert xv.dtype == yv.dtype and xv.tobytes() == yv.tobytes(), k
        assert tuple(x[k].dims) == tuple(y[k].dims), k


def days(n, start="2003-11-20"):
    return (np.datetime64(start) + np.arange(n)).astype("datetime64[ns]")


def equals_oracle(ds, exp, nspace):
    assert sorted(ds.data_vars) == sorted(exp)
    for k, want in exp.items():
        got = np.asarray(ds[k].values)
        got = got if k == "steps_by" else got.reshape(got.shape[:got.ndim - nspace] + (-1,))
        assert got.dtype == want.dtype and got.shape == want.shape and np.ascontiguousarray(got).tobytes() == want.tobytes(), k


@pytest.mark.parametrize("anchor", ec.ANCHORS)
def test_public_call_on_a_grid(hot, anchor):
    """Host and resident fields in every mix, whole and in windows: one Dataset, equal to the oracle."""
    T, ny, nx, L = 97, 7, 12, 10
    X = ec.chain(T, ny * nx, 0.3, seed=ny, mean_run=3.0)
    X[:, :10] = ec.edge_field(T)[:, :10]
    V = ec.values(T, ny * nx, 8)
    tv = days(T)
    season, G, _, _ = marex_amd.occurrence.group_labels("season", tv, T)
    coords = {"time": ("time", tv), "lat": ("lat", np.linspace(-30, 30, ny)), "lon": ("lon", np.linspace(0, 100, nx))}
    da = lambda a: DataArray(a, dims=("time", "lat", "lon"), coords=coords)  # noqa: E731
    host = [da(a.reshape(T, ny, nx)) for a in (X, V)]
    dev = [da(torch.from_numpy(a.reshape(T, ny, nx)).to(hot.device)) for a in (X, V)]
    for by, grp in ((None, None), ("season", season)):
        kw = dict(max_lag=L, anchor=anchor, by=by)
        first = marex_amd.event_composites(host[0], host[1], **kw)
        equals_oracle(first, eo.variables(X, V, L, anchor, grp, G if by else 1), 2)
        assert first["anchors"].values.reshape(-1)[:10].tolist() == ec.EDGE_ANCHORS[anchor]
        for f, v in ((host[0], dev[1]), (dev[0], host[1]), (dev[0], dev[1]), (host[0], host[1])):
            for bs in (None, 1, 7, "auto"):
                same(first, marex_amd.event_composites(f, v, block_steps=bs, **kw))


def test_public_call_on_a_mesh_with_types_in_every_mix(hot):
    T, C, L = 41, 4100, 30
    X = ec.chain(T, C, 0.1, seed=9, mean_run=3.0)
    V = ec.values(T, C, 9)
    ids = np.where(X, (np.arange(T * C).reshape(T, C) % 9 + 1), 0).astype(np.int32)
    by = ec.labels(T, 3)
    exp = eo.variables(X, V, L, "end", by, 3)
    kw = dict(max_lag=L, anchor="end", by=by)
    first = marex_amd.event_composites(X, V, **kw)
    equals_oracle(first, exp, 1)
    t = lambda a: torch.from_numpy(a).to(hot.device)  # noqa: E731
    fields = [X.astype(np.uint8) * 7, ids, ids.astype(np.int64), t(X), t(X.astype(np.uint8) * 7), t(ids), t(ids.astype(np.int64)),
              Dataset({"extreme_events": DataArray(X, dims=("time", "cells"))})]
    vals = [V, t(V), V.astype(np.float64), t(V.astype(np.float64)), DataArray(V, dims=("time", "cells"))]
    for i, f in enumerate(fields):
        for bs in (None, 3):
            same(first, marex_amd.event_composites(f, vals[(i + (bs or 0)) % len(vals)], block_steps=bs, **kw))
    bad = ids.copy()
    bad[T - 1, C - 1] = -3
    for f in (bad, t(bad)):
        with pytest.raises(DataValidationError, match="Object IDs must be non-negative"):
            marex_amd.event_composites(f, V, block_steps=8)
    with pytest.raises(DataValidationError, match="field and values differ in shape"):
        marex_amd.event_composites(X, V[:, :-1])
