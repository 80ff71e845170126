"""The object and overlap kernels (csrc/marex_objects.hip, csrc/marex_mesh_objects.hip) at the edges of their launch
geometry, through the C entry points on the test's own buffers: spans, moments and compaction per (timestep, ID), overlap
pairs, per-step ranks, row maxima and offsets, area per step.  The cases and plain references are
tests/object_kernel_cases.py: slices that end inside a 64-cell piece, objects across the 1024- and 4096-cell edges of a wave
and a workgroup, IDs living in slices t, t + 64, t + 128 of one workgroup's walk, ID tables ending around multiples of 16
and 4096, hash tables exactly full, one key too many, more pairs than the output holds, 65 535 rows and more.

Every output buffer is one row longer than needed and filled with -77: the spare row must survive and whatever the
contract says is written must equal the reference.  All comparisons are exact.  tests/test_object_kernel_cases_host.py
shows on the host that each of twenty plausible kernel mistakes changes the expected result of some case here.
"""
import os
import sys

import numpy as np
import pytest
import torch

from marex_amd.exceptions import ProcessingError
from marex_amd.track_mesh import mesh_moments_finish

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import object_kernel_cases as oc  # noqa: E402

pytestmark = pytest.mark.gpu

P = oc.POISON
TABLE_NAMES = [n for n in oc.FIELD_NAMES if n not in ("values-big-id",)]
ENGINE_NAMES = oc.FAMILIES["slice"] + oc.FAMILIES["cell"]


def dev(hot, a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(hot.device)


def poisoned(hot, shape, dtype):
    return torch.full(shape, P, dtype=dtype, device=hot.device)


def same(got, want, what):
    """Exact equality with the first difference in the message."""
    got, want = np.asarray(got), np.asarray(want)
    assert got.shape == want.shape, (what, got.shape, want.shape)
    bad = np.argwhere(got != want)
    assert bad.size == 0, (what, f"{len(bad)} differ, first at", bad[0].tolist(), "got", got[tuple(bad[0])].tolist(), "want",
                           want[tuple(bad[0])].tolist())


def spare(t, what):
    """The host copy without the spare last row, which must still hold the canary."""
    a = t.cpu().numpy()
    assert (a[-1] == P).all(), f"{what}: the element behind the output was written"
    return a[:-1]


def run_spans(hot, ids, T, C, max_id):
    nid = max_id + 1
    ntiles = (nid + oc.TILE - 1) // oc.TILE
    tmin, tmax = poisoned(hot, (nid + 1,), torch.int32), poisoned(hot, (nid + 1,), torch.int32)
    off, work = poisoned(hot, (nid + 1,), torch.int64), poisoned(hot, (2 * ntiles + 1,), torch.int64)
    total = poisoned(hot, (2,), torch.int64)
    hot.call("marex_object_spans_i32", ids, T, C, max_id, tmin, tmax, off, work, total)
    spare(work, "work")
    return tmin, tmax, off, int(spare(total, "total")[0])


def run_slots(hot, c, ids, tmin, off, n_slots, mesh, q=None):
    """Moments and compaction: the dense slots [n_slots, 5] and the compacted rows sorted by (t, id)."""
    acc = poisoned(hot, (n_slots + 1, 5), torch.int64)
    if mesh:
        hot.call("marex_mesh_object_moments_i64", ids, c.T, c.C, q, tmin, off, n_slots, acc)
    else:
        hot.call("marex_object_moments_i32", ids, c.T, c.ny, c.nx, tmin, off, n_slots, acc)
    n_out = poisoned(hot, (2,), torch.int64)
    tid, mom = poisoned(hot, (n_slots + 1, 2), torch.int32), poisoned(hot, (n_slots + 1, 5), torch.int64)
    hot.call("marex_object_compact", n_slots, c.max_id, tmin, off, acc, n_out, tid, mom)
    n = int(spare(n_out, "n_out")[0])
    assert 0 < n <= n_slots, (n, n_slots)
    tid_h, mom_h = spare(tid, "out_tid").astype(np.int64), spare(mom, "out_mom")
    assert (tid_h[n:] == P).all() and (mom_h[n:] == P).all(), "rows behind the compacted ones were written"
    order = np.argsort((tid_h[:n, 0] << 32) | tid_h[:n, 1])
    return spare(acc, "acc"), tid_h[:n][order], mom_h[:n][order]


def check_tables(hot, name, mesh):
    c, e = oc.get(name), oc.expected(name)
    ids = dev(hot, c.ids)
    tmin, tmax, off, total = run_spans(hot, ids, c.T, c.C, c.max_id)
    w_tmin, w_tmax, w_off, w_total = e.spans
    same(spare(tmin, "tmin"), w_tmin, f"{name} tmin")
    same(spare(tmax, "tmax"), w_tmax, f"{name} tmax")
    same(spare(off, "off"), w_off, f"{name} off")
    assert total == w_total, (name, total, w_total)
    assert np.array_equal(ids.cpu().numpy(), c.ids)
    if total == 0:
        return None
    w_tid, w_mom = e.mesh if mesh else e.grid
    acc, tid, mom = run_slots(hot, c, ids, tmin, off, total, mesh, dev(hot, c.q) if mesh else None)
    same(acc, oc.slots(w_tid, w_mom, e.spans), f"{name} slots")
    same(tid, w_tid, f"{name} compacted (t, id)")
    same(mom, w_mom, f"{name} compacted moments")
    return acc, tid, mom


@pytest.mark.parametrize("name", TABLE_NAMES)
def test_spans_moments_and_compaction_on_a_grid(hot, name):
    oc.check_coverage(name)
    check_tables(hot, name, mesh=False)


@pytest.mark.parametrize("name", TABLE_NAMES)
def test_spans_moments_and_compaction_on_a_mesh(hot, name):
    check_tables(hot, name, mesh=True)


def run_count(hot, ids, T, C):
    stats = poisoned(hot, (5,), torch.int64)
    hot.call("marex_overlap_count_i32", ids, T, C, stats)
    return spare(stats, "stats")


def run_pairs(hot, ids, T, C, cap, out_cap, q0=None):
    """``(stats, {(a, b): value}, raw rows)`` of the grid (q0 None) or the mesh pair table; the value of a mesh pair is
    sums[1] * 2^32 + sums[0] as a Python integer."""
    w = 1 if q0 is None else 2
    keys, vals = poisoned(hot, (cap + 1,), torch.int64), poisoned(hot, (cap + 1, w), torch.int64)
    stats = poisoned(hot, (5,), torch.int64)
    out_k, out_v = poisoned(hot, (out_cap + 1,), torch.int64), poisoned(hot, (out_cap + 1, w), torch.int64)
    if q0 is None:
        hot.call("marex_overlap_pairs_i32", ids, T, C, cap, keys, vals, stats, out_cap, out_k, out_v)
    else:
        hot.call("marex_mesh_overlap_pairs_i64", ids, T, C, q0, cap, keys, vals, stats, out_cap, out_k, out_v)
    spare(keys, "keys"), spare(vals, "table values")
    s = spare(stats, "stats")
    assert s[0] == P and s[1] == P, "stats[0..1] belong to the counting pass"
    k, v = spare(out_k, "out_keys"), spare(out_v, "out values").view(np.uint64)
    n = min(int(s[3]), out_cap)
    assert (k[n:] == P).all() and (out_v.cpu().numpy()[n:-1] == P).all(), "entries behind the pairs were written"
    order = np.argsort(k[:n], kind="stable")
    k, v = k[:n][order], v[:n][order]
    if q0 is None:
        got = {(int(x) >> 32, int(x) & oc.MASK32): int(y[0]) for x, y in zip(k, v)}
    else:
        got = {(int(x) >> 32, int(x) & oc.MASK32): (int(y[1]) << 32) + int(y[0]) for x, y in zip(k, v)}
    assert len(got) == n, "a key was emitted twice"
    return s, got, (k.tobytes(), v.tobytes())


def same_pairs(got, want, what):
    if got != want:
        for key in sorted(set(got) | set(want)):
            assert got.get(key) == want.get(key), (what, "first differing pair", key, "got", got.get(key), "want", want.get(key))


@pytest.mark.parametrize("name", oc.FIELD_NAMES)
def test_overlap_counts_and_pairs(hot, name):
    c, e = oc.get(name), oc.expected(name)
    ids = dev(hot, c.ids)
    s = run_count(hot, ids, c.T, c.C)
    assert s[0] == e.cells and s[1] >= len(e.overlaps) and s[2] == 0 and s[3] == 0, (name, s.tolist(), e.cells, len(e.overlaps))
    assert np.array_equal(run_count(hot, ids, c.T, c.C), s), "the counting pass is not repeatable"
    if c.T < 2 or s[1] == 0:
        assert not e.overlaps
        return
    runs = int(s[1])
    cap = oc.table_cap(runs)
    st, got, _ = run_pairs(hot, ids, c.T, c.C, cap, runs)
    assert st[2] == 0 and st[3] == len(e.overlaps), (name, st.tolist())
    same_pairs(got, e.overlaps, f"{name} grid pairs")
    st, got, _ = run_pairs(hot, ids, c.T, c.C, cap, runs, dev(hot, c.q[0]))
    assert st[2] == 0 and st[3] == len(e.overlaps), (name, st.tolist())
    same_pairs(got, e.mesh_overlaps, f"{name} mesh pairs")


@pytest.mark.parametrize("name", ["slice-T130-C4097-const", "cell-8193-alt", "cell-4097-one", "nx-130x1"])
def test_results_do_not_depend_on_the_order_of_arrival(hot, name):
    """Large objects: many waves add to one slot and one table entry.  Two runs give the same bytes once sorted."""
    c = oc.get(name)
    ids = dev(hot, c.ids)
    for mesh in (False, True):
        a, b = check_tables(hot, name, mesh), check_tables(hot, name, mesh)
        assert all(x.tobytes() == y.tobytes() for x, y in zip(a, b)), (name, mesh)
    runs = int(run_count(hot, ids, c.T, c.C)[1])
    for q0 in (None, dev(hot, c.q[0])):
        a, b = (run_pairs(hot, ids, c.T, c.C, oc.table_cap(runs), runs, q0) for _ in range(2))
        assert a[2] == b[2] and a[1] == b[1] and np.array_equal(a[0], b[0]), (name, q0 is None)


@pytest.mark.parametrize("name", oc.FIELD_NAMES)
def test_minmax_and_row_max_of_the_field_cases(hot, name):
    c, e = oc.get(name), oc.expected(name)
    ids = dev(hot, c.ids)
    mm = poisoned(hot, (3,), torch.int32)
    hot.call("marex_ids_minmax_i32", ids, c.ids.size, mm)
    assert tuple(spare(mm, "minmax").tolist()) == e.minmax, name
    rm = poisoned(hot, (c.T + 1,), torch.int32)
    hot.call("marex_ids_row_max_i32", ids, c.T, c.C, rm)
    same(spare(rm, "rowmax"), e.row_max, f"{name} row maxima")


@pytest.mark.parametrize("name", oc.MINMAX_NAMES)
def test_minmax_around_the_launch_width(hot, name):
    a = oc.minmax_case(name)
    mm = poisoned(hot, (3,), torch.int32)
    hot.call("marex_ids_minmax_i32", dev(hot, a), a.size, mm)
    assert tuple(spare(mm, "minmax").tolist()) == oc.minmax(a), name
    assert a.size == 1 or oc.minmax(a) == (oc.INT_MIN, oc.INT_MAX)


@pytest.mark.parametrize("mesh", [False, True], ids=["grid", "mesh"])
@pytest.mark.parametrize("name", oc.HASH_NAMES)
def test_the_hash_tables_keep_their_contract(hot, name, mesh):
    oc.check_hash_coverage(name)
    h = oc.hash_case(name)
    want = oc.mesh_overlaps(h.ids, h.q0) if mesh else oc.overlaps(h.ids)
    ids = dev(hot, h.ids)
    st, got, _ = run_pairs(hot, ids, h.T, h.C, h.cap, h.out_cap, dev(hot, h.q0) if mesh else None)
    if name == "hash-65-one-too-many":
        assert st[2] != 0 and st[3] == 64 and len(got) == 64, (st.tolist(), len(got))
        for key, v in got.items():  # whichever key found no entry, the stored ones are whole
            assert want.get(key) == v, (key, v, want.get(key))
    elif name == "hash-40-out-39":
        assert st[2] == 0 and st[3] == 40 and len(got) == 39, (st.tolist(), len(got))
        for key, v in got.items():
            assert want.get(key) == v, (key, v, want.get(key))
    else:
        assert st[2] == 0 and st[3] == 64, st.tolist()
        same_pairs(got, want, name)


@pytest.mark.parametrize("name", oc.RANK_NAMES)
def test_ranks_of_roots(hot, name):
    oc.check_rank_coverage(name)
    r = oc.rank_case(name)
    w_rank, w_nt, w_ids = oc.rank_roots(r.labels, r.T, r.C)
    n = r.T * r.C
    for in_place in (False, True):
        labels = poisoned(hot, (n + 1,), torch.int32)
        labels[:n] = dev(hot, r.labels)
        rank, n_t = poisoned(hot, (n + 1,), torch.int32), poisoned(hot, (r.T + 1,), torch.int32)
        ids = labels if in_place else poisoned(hot, (n + 1,), torch.int32)
        hot.call("marex_label_mesh_rank_i32", labels, r.T, r.C, rank, ids, n_t)
        same(spare(n_t, "n_t"), w_nt, f"{name} n_t")
        same(spare(rank, "rank"), w_rank, f"{name} rank (in place: {in_place})")
        same(spare(ids, "ids"), w_ids, f"{name} ids (in place: {in_place})")
        if not in_place:
            assert np.array_equal(spare(labels, "labels"), r.labels)


@pytest.mark.parametrize("name", oc.LONG_NAMES)
def test_row_maxima_and_offsets_of_long_and_wide_fields(hot, name):
    oc.check_long_coverage(name)
    c = oc.long_case(name)
    ids = poisoned(hot, (c.T + 1, c.C), torch.int32)
    ids[:c.T] = dev(hot, c.ids)
    rm = poisoned(hot, (c.T + 1,), torch.int32)
    hot.call("marex_ids_row_max_i32", ids, c.T, c.C, rm)
    same(spare(rm, "rowmax"), oc.row_max(c.ids), f"{name} row maxima")
    want = oc.add_row_offset(c.ids, c.off)
    off, out = dev(hot, c.off), poisoned(hot, (c.T + 1, c.C), torch.int32)
    hot.call("marex_ids_add_row_offset_i32", ids, c.T, c.C, off, out)
    same(spare(out, "out"), want, f"{name} offsets")
    assert np.array_equal(spare(ids, "ids"), c.ids)
    hot.call("marex_ids_add_row_offset_i32", ids, c.T, c.C, off, ids)
    same(spare(ids, "ids"), want, f"{name} offsets in place")


@pytest.mark.parametrize("name", oc.AREA_NAMES)
def test_area_per_step(hot, name):
    oc.check_long_coverage(name)
    c = oc.long_case(name)
    data = torch.full((c.T + 1, c.C), 255, dtype=torch.uint8, device=hot.device)  # a spare row of set cells: never read
    data[:c.T] = dev(hot, c.data)
    out = poisoned(hot, (c.T + 1,), torch.int64)
    hot.call("marex_mesh_area_i64", data, c.T, c.C, dev(hot, c.q0), out)
    same(spare(out, "area"), oc.mesh_area(c.data, c.q0), f"{name} area")


def test_the_entry_points_refuse_bad_arguments(hot):
    """One refusal each, naming the entry point, before anything is launched: the buffers keep their canaries."""
    i32, i64 = poisoned(hot, (64,), torch.int32), poisoned(hot, (640,), torch.int64)
    u8 = torch.zeros((64,), dtype=torch.uint8, device=hot.device)
    good = {
        "marex_ids_minmax_i32": [i32, 8, i32],
        "marex_object_spans_i32": [i32, 2, 4, 3, i32, i32, i64, i64, i64],
        "marex_object_moments_i32": [i32, 2, 2, 2, i32, i64, 4, i64],
        "marex_mesh_object_moments_i64": [i32, 2, 4, i64, i32, i64, 4, i64],
        "marex_object_compact": [4, 3, i32, i64, i64, i64, i32, i64],
        "marex_overlap_count_i32": [i32, 2, 4, i64],
        "marex_overlap_pairs_i32": [i32, 2, 4, 64, i64, i64, i64, 8, i64, i64],
        "marex_mesh_overlap_pairs_i64": [i32, 2, 4, i64, 64, i64, i64, i64, 8, i64, i64],
        "marex_label_mesh_rank_i32": [i32, 2, 4, i32, i32, i32],
        "marex_ids_row_max_i32": [i32, 2, 4, i32],
        "marex_ids_add_row_offset_i32": [i32, 2, 4, i32, i32],
        "marex_mesh_area_i64": [u8, 2, 4, i64, i64],
    }
    # (argument index, bad value): every pointer as NULL, then the sizes
    sizes = {
        "marex_ids_minmax_i32": [(1, 0)],
        "marex_object_spans_i32": [(1, 0), (2, 0), (1, -1), (3, -1)],
        "marex_object_moments_i32": [(1, 0), (2, 0), (3, 0), (6, 0)],
        "marex_mesh_object_moments_i64": [(1, 0), (2, 0), (6, 0)],
        "marex_object_compact": [(0, 0), (1, -1)],
        "marex_overlap_count_i32": [(1, 0), (2, 0)],
        "marex_overlap_pairs_i32": [(1, 1), (1, 0), (2, 0), (3, 32), (3, 96), (3, 0), (3, -64), (7, 0), (7, -1)],
        "marex_mesh_overlap_pairs_i64": [(1, 1), (1, 0), (2, 0), (4, 32), (4, 96), (4, 0), (4, -64), (8, 0), (8, -1)],
        "marex_label_mesh_rank_i32": [(1, 0), (2, 0)],
        "marex_ids_row_max_i32": [(1, 0), (2, 0)],
        "marex_ids_add_row_offset_i32": [(1, 0), (2, 0)],
        "marex_mesh_area_i64": [(1, 0), (2, 0)],
    }
    assert sorted(good) == sorted(sizes)
    n = 0
    for name, args in good.items():
        bad = [(k, None) for k, a in enumerate(args) if isinstance(a, torch.Tensor)] + sizes[name]
        for k, v in bad:
            trial = list(args)
            trial[k] = v
            with pytest.raises(ProcessingError, match=name):
                hot.call(name, *trial)
                pytest.fail(f"{name}: argument {k + 1} = {v} was accepted")
            n += 1
    hot.sync()
    assert n >= 90 and (i32.cpu().numpy() == P).all() and (i64.cpu().numpy() == P).all()


# ---------------------------------------------------------------------------------------------------------- through the engine
@pytest.mark.parametrize("name", ENGINE_NAMES)
def test_the_engine_agrees_on_a_grid(hot, name):
    """HotPath.object_moments / overlap_pairs: the host-side sort, division, seam correction and table sizing."""
    c, e = oc.get(name), oc.expected(name)
    ids = dev(hot, c.ids)
    got = hot.object_moments(ids, c.ny, c.nx, wrap=True)
    tid, mom = e.grid
    cnt, sy, sx, nr, fl = (mom[:, k] for k in range(5))
    c1 = sx / cnt
    shifted = (sx - c.nx * nr) / cnt
    c1 = np.where(fl == 3, np.where(shifted < 0, shifted + c.nx, shifted), c1)
    same(got["t"], tid[:, 0], f"{name} t")
    same(got["id"], tid[:, 1], f"{name} id")
    same(got["area"], cnt.astype(np.float64), f"{name} area")
    same(got["centroid"], np.stack([sy / cnt, c1]), f"{name} centroid")
    want = np.array([[a, b, n] for (a, b), n in sorted(e.overlaps.items())], np.int32).reshape(-1, 3)
    same(hot.overlap_pairs(ids), want, f"{name} overlap pairs")


@pytest.mark.parametrize("name", ENGINE_NAMES + ["values-pair-sum-above-64-bits", "values-q-big"])
def test_the_engine_agrees_on_a_mesh(hot, name):
    c, e = oc.get(name), oc.expected(name)
    ids, q, ex = dev(hot, c.ids), dev(hot, c.q), 20
    got = hot.mesh_object_moments(ids, q, ex)
    tid, mom = e.mesh
    area, centroid = mesh_moments_finish(mom, ex)
    for k, w in (("t", tid[:, 0]), ("id", tid[:, 1]), ("cells", mom[:, 0]), ("area", area), ("centroid", centroid)):
        same(got[k], w, f"{name} {k}")
    want = np.array([[np.float32(a), np.float32(b), np.float32(np.ldexp(float(s), -ex))]
                     for (a, b), s in sorted(e.mesh_overlaps.items())], np.float32).reshape(-1, 3)
    same(hot.mesh_overlap_pairs(ids, q, ex), want, f"{name} mesh overlap pairs")


@pytest.mark.parametrize("mesh", [False, True], ids=["grid", "mesh"])
def test_the_engine_reports_a_table_that_overflows(hot, monkeypatch, mesh):
    """65 pairs into a table the test shrinks to 64 entries on the way to the library."""
    h = oc.hash_case("hash-65-one-too-many")
    ids = dev(hot, h.ids)
    call = hot.call
    seen = []

    def shrunk(name, *args):
        args = list(args)
        if name in ("marex_overlap_pairs_i32", "marex_mesh_overlap_pairs_i64"):
            k = 3 if name == "marex_overlap_pairs_i32" else 4
            assert args[k] >= 128
            args[k] = 64
            seen.append(name)
        return call(name, *args)

    monkeypatch.setattr(hot, "call", shrunk)
    with pytest.raises(ProcessingError, match="hash table overflow"):
        if mesh:
            q = np.zeros((4, h.C), np.int64)
            q[0] = h.q0
            hot.mesh_overlap_pairs(ids, dev(hot, q), 20)
        else:
            hot.overlap_pairs(ids)
    assert len(seen) == 1
