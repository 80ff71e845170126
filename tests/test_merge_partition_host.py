"""Host checks of the partition cases (tests/merge_partition_cases.py): no device.

* The oracle's vectorised partitions (merge_oracle.partition_nn / partition_centroid) equal a scalar, cell-by-cell
  restatement of the reference's algorithm on every case: the 3 x 3 walk over bucket indices taken modulo the bucket
  counts, a strict ``<`` across the parents in order, ``<=`` against max_distance, the centroid rule for a cell nothing
  reaches.  The restatement works on the batched tables the device gets (entries, shared parents, one flat bucket table
  with scanned starts), the oracle on one child at a time.
* The restatement takes a ``defect=``: one plausible kernel mistake each.  Every defect changes the result of at least one
  case, so a kernel with that mistake cannot pass the device test that runs the same cases.
* The coverage conditions of the case families hold (merge_partition_cases.check_coverage).
"""
import functools
import math
import os
import sys

import numpy as np
import pytest
import torch

from marex_amd.exceptions import ProcessingError

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import merge_partition_cases as mc  # noqa: E402
from test_engine_call_host import _engine  # noqa: E402

DEFECTS = {
    "tie_le": "<= instead of < between parents",
    "cap_lt": "< instead of <= against max_distance",
    "no_wrap": "dx never wrapped",
    "wrap_regional": "dx wrapped in regional mode",
    "clamp_buckets": "bucket indices clamped instead of taken modulo",
    "shared_first_entry": "a shared parent filed under its first entry only",
    "first_bucket_size": "the bucket size of the first entry used for all entries",
    "fallback_leftover": "the centroid search starts from the nearest candidate the bucket walk saw, beyond the cap or not",
    "squares": "squared distances compared instead of roots",
    "skip_high_cells": "cells with flat index >= 2 097 152 skipped",
    "scan_drops_tail": "an exclusive scan that drops the last, partial thread range",
}
SCAN_THREADS = 1024
INF = math.inf


def _distance(defect, nx, wrap):
    if defect == "no_wrap":
        wrap = False
    if defect == "wrap_regional":
        wrap = True

    def dist(dy, dx):
        if wrap:
            if dx > nx / 2:
                dx -= nx
            elif dx < -nx / 2:
                dx += nx
        q = dy * dy + dx * dx
        return q if defect == "squares" else math.sqrt(q)

    return dist


def _nearest_centroid(dist, y, x, c, lo, hi, bd, le):
    best = lo
    for j in range(lo, hi):
        d = dist(y - float(c.pcy[j]), x - float(c.pcx[j]))
        if d < bd or (le and d <= bd):
            bd, best = d, j
    return best


def restated(name, nn, defect=None):
    """The slice of case ``name`` after the partition, one cell at a time."""
    c = mc.get(name)
    ny, nx = c.ny, c.nx
    dist = _distance(defect, nx, c.wrap)
    le = defect == "tie_le"
    out = c.cur.copy()
    n_ent = len(c.lab)
    child_of = {int(k): i for i, k in enumerate(c.child_keys)}
    if nn:
        real = [max(2, int(m) // 4) for m in c.maxd]
        size = [real[0]] * n_ent if defect == "first_bucket_size" else real
        ngy = [(ny + g - 1) // g for g in real]
        ngx = [(nx + g - 1) // g for g in real]
        base = [0]
        for j in range(n_ent):
            base.append(base[-1] + ngy[j] * ngx[j])
        entries = {}
        for j, p in enumerate(c.parents.tolist()):
            entries.setdefault(p, []).append(j)
        buckets = {}
        for p, ent in entries.items():
            if defect == "shared_first_entry":
                ent = ent[:1]
            for y, x in zip(*(a.tolist() for a in np.nonzero(c.prev == p))):
                for j in ent:
                    b = base[j] + min(y // size[j], ngy[j] - 1) * ngx[j] + min(x // size[j], ngx[j] - 1)
                    buckets.setdefault(b, []).append((y, x))
        if defect == "scan_drops_tail":  # the thread whose range the table's end cuts short writes no bucket starts
            per = (base[-1] + SCAN_THREADS - 1) // SCAN_THREADS
            if base[-1] % per:
                for b in range(base[-1] - base[-1] % per, base[-1]):
                    buckets.pop(b, None)
        cap = [float(m) * float(m) if defect == "squares" else float(m) for m in c.maxd]
    for y, x in zip(*(a.tolist() for a in np.nonzero(np.isin(c.cur, c.child_keys)))):
        if defect == "skip_high_cells" and y * nx + x >= mc.LAUNCH_CELLS:
            continue
        k = child_of[int(c.cur[y, x])]
        lo, hi = int(c.off[k]), int(c.off[k + 1])
        best, bd, seen = -1, INF, INF
        if nn:
            for j in range(lo, hi):
                by, bx = min(y // size[j], ngy[j] - 1), min(x // size[j], ngx[j] - 1)
                m = INF
                for sy in (-1, 0, 1):
                    for sx in (-1, 0, 1):
                        if defect == "clamp_buckets":
                            cy, cx = min(max(by + sy, 0), ngy[j] - 1), min(max(bx + sx, 0), ngx[j] - 1)
                        else:
                            cy, cx = (by + sy) % ngy[j], (bx + sx) % ngx[j]
                        for py, px in buckets.get(base[j] + cy * ngx[j] + cx, ()):
                            d = dist(float(y - py), float(x - px))
                            seen = min(seen, d)
                            if (d < cap[j] if defect == "cap_lt" else d <= cap[j]) and d < m:
                                m = d
                if m < bd or (le and m <= bd and m < INF):
                    bd, best = m, j
        if best < 0:
            best = _nearest_centroid(dist, float(y), float(x), c, lo, hi, seen if defect == "fallback_leftover" else INF, le)
        out[y, x] = c.lab[best]
    return out


@functools.lru_cache(maxsize=None)
def _clean(name, nn):
    return restated(name, nn)


@pytest.mark.parametrize("name", mc.NAMES)
def test_the_oracle_equals_the_scalar_restatement(name):
    for nn in (False, True):
        want, _ = mc.expected(name, nn)
        assert np.array_equal(_clean(name, nn), want), (name, "nearest cell" if nn else "centroid")


@pytest.mark.parametrize("defect", list(DEFECTS))
def test_some_case_sees_the_defect(defect):
    for name in mc.NAMES:
        for nn in (True, False):
            if not np.array_equal(restated(name, nn, defect), _clean(name, nn)):
                return
    pytest.fail(f"no case notices: {DEFECTS[defect]}")


def test_the_defects_are_seen_by_the_families_built_for_them():
    """The families named in the cases' description do their own work (a defect seen only by accident elsewhere would
    leave the family's case pointless)."""
    for defect, names in (("tie_le", ["e-tie"]), ("cap_lt", ["e-cap"]), ("no_wrap", ["e-half"]), ("squares", ["e-roots"]),
                          ("fallback_leftover", ["d-wrap", "d-flat"]), ("skip_high_cells", ["g-1025x2048"]),
                          ("scan_drops_tail", ["f-1025", "f-3073"]), ("shared_first_entry", mc.FAMILIES["c"]),
                          ("first_bucket_size", mc.FAMILIES["c"])):
        for name in names:
            assert not np.array_equal(restated(name, True, defect), _clean(name, True)), (defect, name)
    for total in (1, 2, 1023, 1024, 2049):  # no partial thread range at these totals: the scan's other branch
        assert np.array_equal(restated(f"f-{total}", True, "scan_drops_tail"), _clean(f"f-{total}", True)), total


@pytest.mark.parametrize("name", mc.NAMES)
def test_the_case_meets_its_coverage_condition(name):
    mc.check_coverage(name)


def test_the_families_are_complete():
    assert [len(mc.FAMILIES[f]) for f in "abcdefg"] == [36, 18, 4, 2, 4, 7, 1]
    got = {(mc.get(n).ny, mc.get(n).nx, mc.get(n).wrap, int(mc.get(n).off[1]), mc.get(n).marks["gs"]) for n in mc.FAMILIES["a"]}
    assert {g[:4] for g in got} == {(ny, nx, w, k) for ny, nx in mc.A_SHAPES for w in (True, False) for k in (2, 3, 10)}
    for ny, nx in mc.A_SHAPES:  # every shape meets every bucket size, so also those that leave a partial last bucket
        assert {g[4] for g in got if g[:2] == (ny, nx)} == {2, 3, 10}
    for n in mc.FAMILIES["a"]:
        c = mc.get(n)
        xs = np.nonzero(c.cur == 5)[1]
        assert xs.min() == 0 and xs.max() == c.nx - 1 and 0 < np.nonzero(c.cur == 9)[1].min()
    assert {mc.bucket_counts(mc.get(n).ny, mc.get(n).nx, 40) for n in mc.FAMILIES["b"]} == {(a, b) for a in (1, 2, 3)
                                                                                             for b in (1, 2, 3)}
    assert sorted(int(n.split("-")[1]) for n in mc.FAMILIES["f"]) == [1, 2, 1023, 1024, 1025, 2049, 3 * 1024 + 1]
    g = mc.get("g-1025x2048")
    assert (g.ny, g.nx) == (1025, 2048) and set(np.nonzero(g.cur)[0].tolist()) <= {0, 1, 2, 1022, 1023, 1024}
    assert set(np.nonzero(g.prev)[0].tolist()) <= {0, 1, 2, 1022, 1023, 1024}


def test_relabel_cases_agree_with_a_plain_loop():
    cases = mc.relabel_cases()
    assert list(cases) == mc.RELABEL_NAMES
    for name, (ids, vals, keys, exp) in cases.items():
        if keys is not None:
            assert np.all(np.diff(keys.astype(np.int64)) > 0) and keys.size == vals.size, name
        table = {int(k): int(v) for k, v in zip(range(len(vals)) if keys is None else keys.tolist(), vals.tolist())}
        step = max(1, ids.size // 4096)  # the large cases are checked on a sample; the small ones in full
        for i in range(0, ids.size, step):
            v = int(ids[i])
            assert exp[i] == (table.get(v, v) if v > 0 else v), (name, i, v)
        assert exp.dtype == np.int32 and exp.shape == ids.shape
    sizes = sorted({c[0].size for c in cases.values()})
    assert {1, 255, 256, 257, 1025 * 2048} <= set(sizes)
    dense = cases["h-dense-only-the-edges"]
    assert dense[3][0] != 49 and dense[3][1] == 50 and dense[3][2] == 51  # n_keys - 1 is mapped, n_keys and n_keys + 1 stay


def test_the_engine_refuses_bad_tables_before_the_library():
    """The argument checks of HotPath.partition_centroid / partition_nn / relabel on an engine whose library is a recording
    stub: nothing is recorded for a refused call, and the accepted call passes the tables it was given."""
    hot, log = _engine()
    c = mc.get("a-7x64-wrap-k3")
    cur, prev = torch.from_numpy(c.cur.reshape(-1).copy()), torch.from_numpy(c.prev.reshape(-1).copy())
    ok = dict(ny=c.ny, nx=c.nx, child_keys=c.child_keys, off=c.off, parents=c.parents, pcy=c.pcy, pcx=c.pcx, lab=c.lab,
              maxd=c.maxd, cur=cur, prev=prev)

    def centroid(**kw):
        a = {**ok, **kw}
        hot.partition_centroid(a["cur"], a["ny"], a["nx"], a["child_keys"], a["off"], a["pcy"], a["pcx"], a["lab"], c.wrap)

    def nearest(**kw):
        a = {**ok, **kw}
        hot.partition_nn(a["cur"], a["prev"], a["ny"], a["nx"], a["child_keys"], a["off"], a["parents"], a["pcy"], a["pcx"],
                         a["lab"], a["maxd"], c.wrap)

    slices = {"an int64 slice": dict(cur=cur.to(torch.int64)), "a short slice": dict(cur=cur[:-1]),
              "a strided slice": dict(cur=torch.zeros(2 * cur.numel(), dtype=torch.int32)[::2]),
              "a slice of another device": dict(cur=torch.zeros(cur.numel(), dtype=torch.int32, device="meta"))}
    for what, kw in {**mc.bad_tables(c), **slices}.items():
        for fn in (centroid, nearest):
            with pytest.raises(ProcessingError):
                fn(**kw)
                pytest.fail(f"{fn.__name__}: {what} was accepted")
    for what, kw in {**mc.bad_nn_tables(c), "an int64 prev": dict(prev=prev.to(torch.int64)),
                     "a short prev": dict(prev=prev[1:])}.items():
        with pytest.raises(ProcessingError):
            nearest(**kw)
            pytest.fail(f"nearest: {what} was accepted")
    ids = torch.arange(-3, 40, dtype=torch.int32)
    for what, (vals, keys) in mc.bad_relabel_tables().items():
        with pytest.raises(ProcessingError):
            hot.relabel(ids, vals, keys)
            pytest.fail(f"relabel: {what} was accepted")
    assert log == []
    assert np.array_equal(cur.numpy(), c.cur.reshape(-1)) and np.array_equal(prev.numpy(), c.prev.reshape(-1))
    centroid()
    hot.relabel(ids, [7, 8], [2, 3])
    hot.relabel(ids, np.zeros(0, np.int32), np.zeros(0, np.int32))  # nothing to rename: no call
    calls = [e for e in log if e != "bind" and e[0] != "check"]
    assert [e[0] for e in calls] == ["marex_partition_centroid_i32", "marex_relabel_i32"]
    args = calls[0][1]
    assert args[1:4] == (cur.data_ptr(), c.ny, c.nx) and args[5] == len(c.child_keys) and args[-1] == 1
    assert calls[1][1][1:3] == (ids.data_ptr(), ids.numel()) and calls[1][1][-1] == 2
