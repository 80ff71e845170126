"""GPU parity: compound events (``marex_compound_u8`` through ``HotPath.call``, ``HotPath.compound`` and
``marex_amd.compound_events``) against the NumPy oracle of tests/compound_oracle.py.  Every output is an integer count or
one float64 division of two of them, so everything compares with ``array_equal``: layouts, unroll edges, lags and
tolerances, the state carried across time windows, step labels and cell classes, input types and residency, the joint
mask, and the guards."""
import os
import sys

import numpy as np
import pytest
import torch

import marex_amd
from marex_amd.exceptions import DataValidationError, ProcessingError
from marex_amd.xr_compat import DataArray

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import compound_cases as cc  # noqa: E402
import compound_oracle as co  # noqa: E402

pytestmark = pytest.mark.gpu
S = 13  # rows of the carried state


def to_dev(hot, a, misaligned=False):
    """A uint8 copy of ``a`` on the device; ``misaligned``: a contiguous view that starts one byte past an aligned address."""
    a = np.ascontiguousarray(a).astype(np.uint8)
    if not misaligned:
        return torch.from_numpy(a).to(hot.device)
    buf = torch.zeros(a.size + 16, dtype=torch.uint8, device=hot.device)
    v = buf[1:1 + a.size].view(a.shape)
    v.copy_(torch.from_numpy(a))
    assert v.data_ptr() % 4 == 1 and v.is_contiguous()
    return v


def tab(hot, v):
    return None if v is None else torch.from_numpy(np.asarray(v, np.int32)).to(hot.device)


def buffers(hot, T, C, L, G, sgrp, G2, R, grp, cls, mask):
    """Buffers of the test's own: zeroed accumulators with one spare row (plane) behind each as a canary, the mask poisoned."""
    z = lambda shape, dt: torch.zeros(shape, dtype=dt, device=hot.device)  # noqa: E731
    return {"state": z((S + 1, C), torch.int32), "cell_cnt": z((3 * G + 1, C), torch.int32),
            "lag": z((2 * L + 2, C), torch.int32) if L else None,
            "sec_cnt": z((3 * G2 + 1, R), torch.int64) if sgrp is not None else None,
            "mask": torch.full((T + 1, C), 0xCD, dtype=torch.uint8, device=hot.device) if mask else None,
            "status": z(2, torch.int64), "grp": tab(hot, grp), "sgrp": tab(hot, sgrp), "cls": tab(hot, cls)}


def kernel(hot, a, b, t0, L, K, G, G2, R, bufs):
    Tb, C = a.shape
    hot.call("marex_compound_u8", a, b, t0, Tb, C, L, K, bufs["grp"], G, bufs["sgrp"], G2, bufs["cls"], R, bufs["state"],
             bufs["cell_cnt"], bufs["lag"], bufs["sec_cnt"], bufs["mask"], bufs["status"])


def read(bufs, G, G2):
    out = {k: (None if bufs[k] is None else bufs[k].cpu().numpy()) for k in ("state", "cell_cnt", "lag", "sec_cnt", "mask", "status")}
    for k in ("state", "cell_cnt", "lag", "sec_cnt"):  # the canaries
        assert out[k] is None or not out[k][-1].any(), k
    assert out["mask"] is None or (out["mask"][-1] == 0xCD).all()
    C = out["state"].shape[1]
    st = out["state"][:-1].view(np.uint32)
    return {"days": out["cell_cnt"][:-1].view(np.uint32).reshape(3, G, C), "runs": st[0:3], "co": st[7:11], "state": st,
            "lag_days": None if out["lag"] is None else out["lag"][:-1].view(np.uint32),
            "sec_cnt": None if out["sec_cnt"] is None else out["sec_cnt"][:-1].view(np.uint64).reshape(3, G2, -1),
            "mask": None if out["mask"] is None else out["mask"][:-1], "lost": int(out["status"][1])}


def run(hot, A, B, L=0, K=0, grp=None, G=1, sgrp=None, G2=0, cls=None, R=0, mask=True, misaligned=False, cuts=None):
    """The kernel over the windows between ``cuts`` (None: one call)."""
    T, C = A.shape
    bufs = buffers(hot, T, C, L, G, sgrp, G2, R, grp, cls, mask)
    cuts = [0, T] if cuts is None else cuts
    for lo, hi in zip(cuts[:-1], cuts[1:]):
        kernel(hot, to_dev(hot, A[lo:hi], misaligned), to_dev(hot, B[lo:hi], misaligned), lo, L, K, G, G2 if sgrp is not None else 0,
               R if sgrp is not None else 0, bufs)
    return read(bufs, G, G2)


def check(hot, A, B, L=0, K=0, grp=None, G=1, sgrp=None, G2=0, cls=None, R=0, mask=True, misaligned=False, cuts=None, want=None):
    """The kernel on ``A``, ``B`` against the oracle: every output, the joint mask byte for byte, the status word."""
    got = run(hot, A, B, L, K, grp, G, sgrp, G2, cls, R, mask, misaligned, cuts)
    want = co.compound(A, B, L, K, grp, G, sgrp, G2, cls, R) if want is None else want
    what = (A.shape, L, K, misaligned, cuts)
    for k in ("days", "runs", "co", "lag_days", "sec_cnt"):
        if want[k] is None:
            assert got[k] is None, (k, what)
        else:
            assert got[k].dtype == want[k].dtype and np.array_equal(got[k], want[k]), (k, what)
    if mask:
        assert np.array_equal(got["mask"], (A & B).astype(np.uint8)), what
    assert got["lost"] == co.lost(A, B, grp, G, sgrp, G2, cls, R), what
    return got, want


def labels(T, C):
    """Groups that change inside an unrolled batch, one section group per step, shuffled classes with -1 cells."""
    grp = (np.arange(T) // 3 % 4).astype(np.int32)
    R = 9 if C >= 64 else max(C - 1, 1)
    cls = cc.mesh_classes(C, R) if C >= 64 else (np.arange(C, dtype=np.int32) - 1)
    return dict(grp=grp, G=5, sgrp=np.arange(T, dtype=np.int32), G2=T, cls=cls, R=R)


@pytest.mark.parametrize("C", cc.CELLS)
def test_cells_and_times_equal_the_oracle(hot, C):
    """Every layout and block shape at every length around the unroll depth: all outputs at once (groups, sections, lags,
    tolerance, mask), then the plain instantiation without any of them."""
    for T in cc.TIMES:
        A, B = cc.pair(T, C, 0.4, seed=T)
        got, _ = check(hot, A, B, 7, 1, **labels(T, C))
        assert np.array_equal(got["lag_days"][7], got["days"][2].sum(0))
        check(hot, A, B, mask=False)


@pytest.mark.parametrize("L", cc.LAGS)
@pytest.mark.parametrize("K", cc.TOLERANCES)
def test_lags_and_tolerances(hot, L, K):
    """Every pair of lag and tolerance on independent and on shifted fields, on the hand-made edge columns, and on a record
    shorter than both."""
    for C in (65, 1028):
        for shift in (None, 3):
            A, B = cc.pair(97, C, 0.3, seed=L + K, shift=shift)
            got, _ = check(hot, A, B, L, K)
            if shift and L >= shift:
                assert np.array_equal(got["lag_days"][L + shift], A[:97 - shift].sum(0))
    T = 8 + 2 * max(K, L)
    A, B = cc.edge_pair(T, K, L)
    got, _ = check(hot, A, B, L, K)
    assert got["co"][:2, :4].tolist() == [[1, 1, 1, 1], [1, 0, 1, 0]]  # the last and the first step that meet the run
    assert got["co"][:2, 7].tolist() == [2, 2 if K >= 3 else 1 if K >= 1 else 0]
    assert got["co"][:, 8].tolist() == [1, int(K >= 1), 1, int(K >= 1)]  # the run open at the end is a run
    if L:
        assert got["lag_days"][2 * L, 4] == 1 and got["lag_days"][0, 5] == 1  # the largest lags, counted once
        assert got["lag_days"][:, 9].sum() == 0  # first and last step: further apart than any lag
    A, B = cc.pair(5, 1028, 0.5, seed=3)  # T < L: most lags reach outside the record
    got, _ = check(hot, A, B, L, K)
    if L == 30:
        assert not got["lag_days"][:L - 4].any() and not got["lag_days"][L + 5:].any()


@pytest.mark.parametrize("misaligned", [False, True], ids=["aligned", "misaligned"])
@pytest.mark.parametrize("L,K", [(30, 30), (7, 1), (0, 0)])
def test_windows_carry_the_state(hot, L, K, misaligned):
    """Windows of one step, windows shorter than the lag and the tolerance, and every single cut of the edge columns: the
    bytes of the one call -- state, counts, lags, sections, mask.  The labels change at window edges and inside windows."""
    T, C = 8 + 2 * max(K, L), 1028
    A, B = cc.edge_pair(T, K, L, C)
    lab = labels(T, C)
    whole, want = check(hot, A, B, L, K, misaligned=misaligned, **lab)
    splits = [list(range(T + 1)), list(range(0, T, 3)) + [T], list(range(0, T, 7)) + [T]] + [[0, s, T] for s in range(1, T, 5)]
    s0 = max(K, L) + 2
    splits += [[0, s0 + 1, T], [0, s0 + 3, T], [0, s0 + 2 + K, T], [0, s0 + 3, s0 + 2 + max(K, 1), T]]  # inside the run, after it, before b
    for cuts in splits:
        cuts = sorted(set(cuts))
        got = run(hot, A, B, L, K, misaligned=misaligned, cuts=cuts, **lab)
        for k in ("state", "days", "lag_days", "sec_cnt", "mask"):
            assert (got[k] is None and whole[k] is None) or got[k].tobytes() == whole[k].tobytes(), (k, cuts)
        assert got["lost"] == whole["lost"] == 0


def test_a_misaligned_view_falls_back_to_one_cell_per_lane(hot):
    A, B = cc.pair(17, 1028, 0.4, seed=8)
    lab = labels(17, 1028)
    a, _ = check(hot, A, B, 7, 2, **lab)
    m, _ = check(hot, A, B, 7, 2, misaligned=True, **lab)
    for k in ("state", "days", "lag_days", "sec_cnt", "mask"):
        assert a[k].tobytes() == m[k].tobytes(), k


@pytest.mark.parametrize("cover", cc.COVERAGES)
def test_coverage(hot, cover):
    """Nothing present (every lane skips every row), a few per cent, half, everything -- against each other too."""
    T, C = 41, 1028
    A, B = cc.pair(T, C, cover, seed=1)
    got, _ = check(hot, A, B, 7, 2, **labels(T, C))
    if cover == 0.0:
        assert not got["state"].any() and not got["mask"].any()
    if cover == 1.0:
        assert (got["runs"] == [[T], [1], [T]]).all() and (got["co"] == 1).all() and (got["lag_days"][0] == T - 7).all()
    other = cc.chain(T, C, 0.05, 77)
    check(hot, A, other, 30, 30)
    check(hot, other, A, 1, 0)


def test_labels_and_classes(hot):
    T, C = 19, 1027
    A, B = cc.pair(T, C, 0.4, seed=2)
    every_row = np.arange(T, dtype=np.int32)
    one = np.zeros(C, np.int32)
    check(hot, A, B, grp=every_row, G=T, sgrp=every_row % 2, G2=2, cls=one, R=1)          # a flush at every row; a single class
    check(hot, A, B, 3, 1, grp=None, G=1, sgrp=np.zeros(T, np.int32), G2=1, cls=np.arange(C, dtype=np.int32) % 64, R=64)  # 64 classes in a wave
    A4, B4 = cc.pair(T, 1028, 0.4, seed=12)  # the same with four cells per lane: each sub-cell sees 64 classes in a wave
    check(hot, A4, B4, 3, 1, sgrp=np.zeros(T, np.int32), G2=1, cls=(np.arange(1028, dtype=np.int32) // 4) % 64, R=64)
    check(hot, A, B, grp=(every_row >= 5).astype(np.int32), G=2, sgrp=every_row // 4, G2=5, cls=cc.mesh_classes(C, 70), R=70)
    # labels outside their range address nothing (read() checks the spare rows) and are counted
    grp = np.array([0, 1, 2, 7, -1, 1] + [0] * (T - 6), np.int32)
    sgrp = np.array([0, 5, 0, 0, -4, 0] + [0] * (T - 6), np.int32)
    got, _ = check(hot, A, B, 7, 0, grp=grp, G=3, sgrp=sgrp, G2=1, cls=cc.mesh_classes(C, 9), R=9)
    assert got["lost"] > 0
    with pytest.raises(ProcessingError, match="compound: .* present cells lie under a step label outside its range"):
        hot.compound(to_dev(hot, A), to_dev(hot, B), grp=grp, G=3)
    with pytest.raises(ProcessingError, match="compound: .* present cells lie under"):
        hot.compound(to_dev(hot, A), to_dev(hot, B), sgrp=sgrp, G2=1, cls=one, R=1)


def test_engine_contract(hot):
    """``HotPath.compound``: poisoned fresh buffers, windows through ``acc``, the deferred read, the refusals."""
    from marex_amd.engine import HotPath

    assert HotPath.POISON
    T, C, L, K = 23, 1028, 7, 2
    A, B = cc.pair(T, C, 0.4, seed=4)
    lab = labels(T, C)
    want = co.compound(A, B, L, K, **lab)
    mask = torch.full((T, C), 0xCD, dtype=torch.uint8, device=hot.device)
    acc = None
    for lo in range(0, T, 5):
        hi = min(T, lo + 5)
        r = hot.compound(to_dev(hot, A[lo:hi]).view(torch.bool), to_dev(hot, B[lo:hi]), t0=lo, max_lag=L, tolerance=K, mask=mask, acc=acc,
                         finish=hi == T, **lab)
        acc = r["acc"]
        assert (hi == T) == ("days" in r)
    for k in ("days", "runs", "co", "lag_days", "sec_cnt"):
        assert r[k].dtype == want[k].dtype and np.array_equal(r[k], want[k]), k
    assert np.array_equal(mask.cpu().numpy(), (A & B).astype(np.uint8))
    plain = hot.compound(to_dev(hot, A), to_dev(hot, B))
    assert plain["lag_days"] is None and plain["sec_cnt"] is None and np.array_equal(plain["days"], co.day_counts(A, B))
    a, b = to_dev(hot, A), to_dev(hot, B)
    for bad in (lambda: hot.compound(a, b.to(torch.int32)), lambda: hot.compound(a, b[:-1]), lambda: hot.compound(a.t(), b.t()),
                lambda: hot.compound(a, b, t0=-1), lambda: hot.compound(a, b, G=2), lambda: hot.compound(a, b, max_lag=31),
                lambda: hot.compound(a, b, tolerance=-1), lambda: hot.compound(a, b, max_lag=1.0),
                lambda: hot.compound(a, b, sgrp=lab["sgrp"], G2=T), lambda: hot.compound(a, b, grp=lab["grp"][:3], G=5),
                lambda: hot.compound(a, b, cls=lab["cls"][:-1], sgrp=lab["sgrp"], G2=T, R=9),
                lambda: hot.compound(a, b, mask=mask[:-1]), lambda: hot.compound(a, b, mask=mask.to(torch.int32)),
                lambda: hot.compound(a, b, max_lag=3, acc=hot.compound(a, b, max_lag=2, finish=False)["acc"])):
        with pytest.raises(ProcessingError):
            bad()


def test_return_codes(hot):
    fn = "marex_compound_u8"
    T, C = 6, 1028
    A, B = cc.pair(T, C, 0.4, seed=6)
    a, b = to_dev(hot, A), to_dev(hot, B)
    bufs = buffers(hot, T, C, 2, 1, np.zeros(T, np.int32), 1, 1, np.zeros(T, np.int32), np.zeros(C, np.int32), True)
    names = ("a", "b", "t0", "Tb", "C", "L", "K", "grp", "G", "sgrp", "G2", "cls", "R", "state", "cell_cnt", "lag", "sec_cnt", "mask", "status")
    ok = (a, b, 0, T, C, 2, 1, bufs["grp"], 1, bufs["sgrp"], 1, bufs["cls"], 1, bufs["state"], bufs["cell_cnt"], bufs["lag"],
          bufs["sec_cnt"], bufs["mask"], bufs["status"])

    def with_(**kw):
        return tuple(kw.get(k, v) for k, v in zip(names, ok))

    cases = [(-4, with_(C=2**31 - 1)), (-4, with_(Tb=2**31 - 1)), (-4, with_(t0=2**31 - 1 - T)), (-1, with_(Tb=0)), (-1, with_(C=0)),
             (-1, with_(t0=-1)), (-1, with_(G=0)), (-1, with_(grp=None, G=2)), (-1, with_(G2=0)), (-1, with_(R=0)), (-1, with_(sgrp=None)),
             (-1, with_(cls=None)), (-1, with_(sec_cnt=None)), (-1, with_(a=None)), (-1, with_(b=None)), (-1, with_(state=None)),
             (-1, with_(cell_cnt=None)), (-1, with_(status=None)), (-1, with_(L=31)), (-1, with_(L=-1)), (-1, with_(K=31)), (-1, with_(K=-1)),
             (-1, with_(lag=None)), (-1, with_(L=0))]
    for code, args in cases:  # refused by the library before any launch
        with pytest.raises(ProcessingError, match=rf"{fn} failed \(code {code}\)"):
            hot.call(fn, *args)
    hot.sync()
    assert not any(bufs[k].any() for k in ("state", "cell_cnt", "lag", "sec_cnt", "status")) and (bufs["mask"] == 0xCD).all()
    for args in (ok, with_(grp=None), with_(mask=None), with_(L=0, lag=None), with_(sgrp=None, cls=None, sec_cnt=None, G2=0, R=0)):
        hot.call(fn, *args)
    hot.sync()
    assert int(bufs["cell_cnt"][2].sum().item()) == 5 * int((A & B).sum()) and not bufs["status"].any()


# ------------------------------------------------------------------ the public call
def same(x, y):
    assert list(x.data_vars) == list(y.data_vars)
    for k in x.data_vars:
        xv, yv = (v.cpu().numpy() if torch.is_tensor(v) else np.asarray(v) for v in (x[k].data, y[k].data))
        assert xv.dtype == yv.dtype and xv.tobytes() == yv.tobytes(), k
        assert tuple(x[k].dims) == tuple(y[k].dims), k


def days(n, start="2003-11-20"):
    return (np.datetime64(start) + np.arange(n)).astype("datetime64[ns]")


@pytest.mark.parametrize("ny,nx", [(7, 12), (5, 13)])
def test_public_call_on_grids(hot, ny, nx):
    """Host and resident fields in every mix, whole and in windows: one Dataset, equal to the oracle; the joint mask goes on
    to ``event_occurrence``."""
    T, L, K = 97, 7, 2
    A, B = cc.pair(T, ny * nx, 0.3, seed=ny)
    tv = days(T)
    doy, G, _, _ = marex_amd.occurrence.group_labels("dayofyear", tv, T)
    months, G2, _, _ = marex_amd.occurrence.zonal_labels("month", tv, T)
    assert G == T and G2 == 4
    cls = np.repeat(np.arange(ny, dtype=np.int32), nx)
    exp = co.variables(A, B, L, K, doy, G, months, G2, cls, ny, np.full(ny, nx))
    coords = {"time": ("time", tv), "lat": ("lat", np.linspace(-30, 30, ny)), "lon": ("lon", np.linspace(0, 100, nx))}
    host = [DataArray(v.reshape(T, ny, nx), dims=("time", "lat", "lon"), coords=coords) for v in (A, B)]
    dev = [DataArray(torch.from_numpy(v.reshape(T, ny, nx)).to(hot.device), dims=("time", "lat", "lon"), coords=coords) for v in (A, B)]
    kw = dict(max_lag=L, tolerance=K, by="dayofyear", zonal=True, zonal_by="month")
    first = marex_amd.compound_events(host[0], host[1], **kw)
    for k, want in exp.items():
        got = np.asarray(first[k].values)
        got = got if k in ("steps_by", "cells_a", "cells_b", "cells_both", "share_both", "class_cells") else got.reshape(got.shape[:got.ndim - 2] + (-1,))
        assert got.dtype == want.dtype and np.array_equal(got, want, equal_nan=True), k
    assert sorted(first.data_vars) == sorted(exp)
    for fa, fb in ((host[0], dev[1]), (dev[0], host[1]), (dev[0], dev[1])):
        for bs in (None, 1, 7, "auto"):
            same(first, marex_amd.compound_events(fa, fb, block_steps=bs, **kw))
    for fa, resident in ((host[0], False), (dev[0], True)):
        ds = marex_amd.compound_events(fa, dev[1], return_mask=True, block_steps=10, **kw)
        m = ds["compound_events"]
        assert torch.is_tensor(m.data) == resident and (m.data.dtype == torch.bool if resident else m.data.dtype == np.bool_)
        assert np.array_equal(m.data.cpu().numpy() if resident else m.data, (A & B).reshape(T, ny, nx))
        occ = marex_amd.event_occurrence(m)
        for k, j in (("days_both", "occurrence"), ("n_runs", "n_runs"), ("longest_run", "longest_run"), ("mean_run", "mean_run")):
            assert np.asarray(ds[k].values).tobytes() == np.asarray(occ[j].values).tobytes(), k


def test_public_call_on_a_mesh_with_types_in_every_mix(hot):
    T, C, L, K = 41, 4100, 30, 30
    A, B = cc.pair(T, C, 0.05, seed=9)
    ids = np.where(B, (np.arange(T * C).reshape(T, C) % 9 + 1), 0).astype(np.int32)
    lat = np.random.default_rng(4).uniform(-12, 12, C)
    edges = np.arange(-10.0, 11.0, 2.0)
    cls, R, _ = marex_amd.occurrence.lat_classes(lat, edges, C)
    step = np.arange(T, dtype=np.int32)
    exp = co.variables(A, B, L, K, None, 1, step, T, cls, R, np.bincount(cls[cls >= 0], minlength=R))
    kw = dict(max_lag=L, tolerance=K, zonal=True, zonal_by="step", lat=lat, lat_bins=edges)
    first = marex_amd.compound_events(A, B, **kw)
    for k, want in exp.items():
        got = np.asarray(first[k].values)
        assert got.dtype == want.dtype and np.array_equal(got, want, equal_nan=True), k
    u8 = lambda v: torch.from_numpy(v.astype(np.uint8) * 7).to(hot.device)  # noqa: E731
    for fa, fb in ((u8(A), u8(B)), (A, ids), (torch.from_numpy(A).to(hot.device), torch.from_numpy(ids).to(hot.device)),
                   (A.astype(np.uint8), ids.astype(np.int64)), (u8(A), B)):
        for bs in (None, 3):
            same(first, marex_amd.compound_events(fa, fb, block_steps=bs, **kw))
    m = marex_amd.compound_events(u8(A), ids, return_mask=True)["compound_events"].data
    assert torch.is_tensor(m) and m.dtype == torch.uint8 and np.array_equal(m.cpu().numpy(), (A & B).astype(np.uint8))
    bad = ids.copy()
    bad[T - 1, C - 1] = -3
    for f in (bad, torch.from_numpy(bad).to(hot.device)):
        with pytest.raises(DataValidationError, match="Object IDs must be non-negative"):
            marex_amd.compound_events(A, f, block_steps=8)
    with pytest.raises(DataValidationError, match="field_a and field_b differ in shape"):
        marex_amd.compound_events(A, B[:, :-1])
