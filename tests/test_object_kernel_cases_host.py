"""Host checks of the object-kernel cases (tests/object_kernel_cases.py): no device.

* Every vectorised reference equals a scalar restatement that walks the field cell by cell, the way the kernels are laid
  out: 64-cell pieces with a packed (lane | dy << 16) sum per group, a run of equal IDs carried by one wave over every 64th
  slice, spans scanned in tiles of 4096 IDs, pairs inserted into an open-addressing table, ranks scanned in chunks of 8192.
* The restatement takes a ``defect=``: one plausible kernel mistake each.  Every defect changes the result of the cases
  built for it, so a kernel with that mistake cannot pass tests/test_gpu_object_kernel_edges.py, which runs the same cases.
* The coverage conditions of all case families hold, and the engine's table sizing keeps its two properties.
"""
import functools
import os
import sys

import numpy as np
import pytest

from marex_amd.engine import pair_table_cap

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import object_kernel_cases as oc  # noqa: E402

DEFECTS = {
    "tail_next_row": "the last, partial piece of a slice reads on into the next slice",
    "skip_t64": "slices t >= 64 are skipped (no stride over the time axis)",
    "skip_last_pair": "the pair of the last two slices (T - 2, T - 1) is skipped",
    "moments_carry": "the moments' run is carried across slices instead of flushed per slice",
    "tmax_first": "tmax is taken from the first slice of a carried run",
    "dy8": "the dy field of the packed sum is 8 bits wide",
    "half_ge": "x >= nx // 2 instead of x > nx // 2",
    "band_left_le": "x <= 100 for the left band",
    "band_right_gt": "x > nx - 100 for the right band",
    "tile_off_dropped": "the tile offset is dropped for tiles >= 1 of the span scan",
    "tile_tail_dropped": "the last, partial 16-ID group of the ID table gets no offsets",
    "compact_first": "compaction gives a slot to the first ID with its offset instead of the last",
    "neg_ids": "negative values are counted as IDs",
    "key_swapped": "the pair key is built as b << 32 | a",
    "probe_no_wrap": "the probe sequence stops at the table's end instead of wrapping",
    "minmax_one_launch": "min / max ignore the elements past the first 2 097 152",
    "rows_one_launch": "row maxima, offsets and areas ignore the rows past the first 65 535",
    "rank_no_run": "the rank scan does not advance its running count between chunks",
    "rank_no_row": "a root is taken as labels == c + 1 without the slice's offset",
    "pair_sum_64": "the mesh pair sum is kept in one 64-bit word",
}
# the cases built for each defect of the field stages: every one of them must notice
SEEN_BY = {
    "tail_next_row": ["cell-1-tail", "cell-63-tail", "cell-65-tail", "cell-1023-tail", "cell-4097-tail", "cell-8193-tail"],
    "skip_t64": ["slice-T65-C70-const", "slice-T65-C70-midgap", "slice-T66-C4097-every64", "slice-T130-C70-change64"],
    "skip_last_pair": ["slice-T2-C70-lastpair", "slice-T64-C70-lastpair", "slice-T65-C4097-lastpair", "slice-T130-C70-lastpair"],
    "moments_carry": ["slice-T66-C70-every64", "slice-T130-C4097-every64", "slice-T129-C70-const", "slice-T130-C70-gap64"],
    "tmax_first": ["slice-T130-C70-gap64", "slice-T66-C4097-every64", "slice-T128-C70-const"],
    "dy8": ["nx-130x1", "nx-70x2", "nx-50x3"],
    "half_ge": ["seam-100", "seam-199", "seam-200", "seam-201"],
    "band_left_le": ["seam-199", "seam-200", "seam-201"],
    "band_right_gt": ["seam-100", "seam-199", "seam-200", "seam-201"],
    "tile_off_dropped": ["table-4096-b", "table-4097-a", "table-8192-b", f"table-{4096 * 1024 + 5}-a"],
    "tile_tail_dropped": ["table-16-a", "table-17-a", "table-4096-a", f"table-{4096 * 1024 + 5}-a"],
    "compact_first": ["table-17-a", "table-16-b", "table-4097-a", "table-8192-b"],
    "neg_ids": ["values-negative", "values-big-id"],
    "key_swapped": ["cell-65-each", "slice-T2-C70-lastpair", "cell-63-last"],
    "pair_sum_64": ["values-pair-sum-above-64-bits"],
}
R64 = lambda n: (n + 63) // 64 * 64  # noqa: E731


def cells_by_piece(c, defect, table_ids=True):
    """Per slice t: the pieces that hold an ID, ascending, as (piece, [(cell, id), ...]).  Values <= 0 are background."""
    flat = c.ids.reshape(-1).tolist()
    T, C = c.T, c.C
    width = R64(C) if defect == "tail_next_row" else C
    out = []
    for t in range(T):
        pieces = {}
        if not (defect == "skip_t64" and t >= oc.TSTRIDE):
            row = flat[t * C:t * C + width]
            for r, v in enumerate(row):
                if defect == "neg_ids" and v < 0 and (not table_ids or -v <= c.max_id):
                    v = -v
                if v > 0:
                    pieces.setdefault(r // oc.PIECE, []).append((r, v))
        out.append(sorted(pieces.items()))
    return out


def wave_walks(c, table):
    """The walks of one wave: (wave chunk, first slice) -> the (t, pieces of the chunk) it visits, every 64th slice."""
    chunks = (R64(c.C) + oc.WAVE_CELLS - 1) // oc.WAVE_CELLS
    per = oc.WAVE_CELLS // oc.PIECE
    for w in range(chunks):
        for ty in range(min(c.T, oc.TSTRIDE)):
            yield [(t, [(p, cells) for p, cells in table[t] if p // per == w]) for t in range(ty, c.T, oc.TSTRIDE)]


def s_spans(c, defect=None, table=None):
    nid = c.max_id + 1
    tmin, tmax = np.full(nid, oc.INT_MAX, np.int32), np.full(nid, -1, np.int32)
    table = cells_by_piece(c, defect) if table is None else table
    for walk in wave_walks(c, table):
        cur = first = last = 0
        for t, pieces in walk:
            for _, cells in pieces:
                for _, v in cells:
                    if v != cur:
                        if cur:
                            tmin[cur], tmax[cur] = min(tmin[cur], first), max(tmax[cur], last)
                        cur, first, last = v, t, t
                    elif defect != "tmax_first":
                        last = t
        if cur:
            tmin[cur], tmax[cur] = min(tmin[cur], first), max(tmax[cur], last)
    # the exclusive scan: present IDs in order, the empty spans between them take the next one's offset
    off = np.zeros(nid, np.int64)
    run, prev = 0, 0
    for k in np.nonzero(tmax >= 0)[0].tolist():
        off[prev:k + 1] = run
        run += int(tmax[k]) - int(tmin[k]) + 1
        prev = k + 1
    off[prev:] = run
    tile_start = off[::oc.TILE].copy()
    if defect == "tile_off_dropped":
        for tile in range(1, (nid + oc.TILE - 1) // oc.TILE):
            off[tile * oc.TILE:(tile + 1) * oc.TILE] -= tile_start[tile]
    if defect == "tile_tail_dropped" and nid % oc.PER_THREAD:
        off[nid - nid % oc.PER_THREAD:] = oc.POISON
    return tmin, tmax, off, run


def s_moments(c, mesh, defect=None, table=None):
    """{(t, id): [cells, four sums]} by the wave walk: per piece and group one packed sum, per run one flush."""
    ny, nx, q = c.ny, c.nx, [row.tolist() for row in c.q]
    out = {}
    table = cells_by_piece(c, defect) if table is None else table
    half = nx // 2

    def flush(t, cur, acc):
        if cur:
            have = out.setdefault((t, cur), [0, 0, 0, 0, 0])
            for k in range(4):
                have[k] += acc[k]
            have[4] = have[4] + acc[4] if mesh else have[4] | acc[4]

    for walk in wave_walks(c, table):
        cur, acc, t = 0, [0] * 5, 0
        for t, pieces in walk:
            for p, cells in pieces:
                groups = {}
                r0 = p * oc.PIECE
                y0, x0 = divmod(r0, nx)
                for r, v in cells:
                    g = groups.setdefault(v, [0] * 5)
                    g[0] += 1
                    if mesh:
                        for k in range(4):
                            g[k + 1] += q[k][r % c.C]
                    else:
                        y, x = divmod(r, nx)
                        g[1] += y - y0  # the dy field
                        g[2] += r - r0  # the lane field
                        g[3] += (x >= half) if defect == "half_ge" else (x > half)
                        left = x <= 100 if defect == "band_left_le" else x < 100
                        right = x > nx - 100 if defect == "band_right_gt" else x >= nx - 100
                        g[4] |= left + 2 * right
                for v, g in groups.items():  # dict order: by the group's first lane, as the wave's ballots go
                    if not mesh:
                        sdy = g[1] & 0xFF if defect == "dy8" else g[1]
                        g[1], g[2] = g[0] * y0 + sdy, g[0] * x0 + g[2] - nx * sdy
                    if v != cur:
                        flush(t, cur, acc)
                        cur, acc = v, [0] * 5
                    for k in range(4):
                        acc[k] += g[k]
                    acc[4] = acc[4] + g[4] if mesh else acc[4] | g[4]
            if defect != "moments_carry":
                flush(t, cur, acc)
                cur, acc = 0, [0] * 5
        flush(t, cur, acc)
    rows = sorted(out.items())
    tid = np.array([k for k, _ in rows], np.int64).reshape(-1, 2)
    return tid, np.array([v for _, v in rows], np.int64).reshape(-1, 5)


def s_compact(c, sp, tid, defect=None):
    """The (t, id) the compaction gives every filled slot: the owner is the last ID whose offset is <= the slot."""
    tmin, tmax, off, total = sp
    present = np.nonzero(tmax >= 0)[0].tolist()
    first_with = {}  # offset -> the first ID that has it
    prev = -1
    for k in present:
        first_with[int(off[k])] = prev + 1
        prev = k
    out = []
    for t, k in tid.tolist():
        slot = int(off[k]) + t - int(tmin[k])
        owner = k
        if defect == "compact_first":
            owner = first_with[int(off[k])]
        out.append((int(tmin[owner]) + slot - int(off[owner]), owner))
    return np.array(sorted(out), np.int64).reshape(-1, 2)


def s_overlaps(c, mesh, defect=None):
    flat = c.ids.reshape(-1).tolist()
    q0 = c.q[0].tolist()
    T, C = c.T, c.C
    width = R64(C) if defect == "tail_next_row" else C
    out = {}
    for t in range(T - 1 - (defect == "skip_last_pair")):
        if defect == "skip_t64" and t >= oc.TSTRIDE:
            continue
        ra, rb = flat[t * C:t * C + width], flat[(t + 1) * C:(t + 1) * C + width]
        for r, (a, b) in enumerate(zip(ra, rb)):
            if defect == "neg_ids":
                if a == 0 or b == 0:
                    continue
                a, b = a & oc.MASK32, b & oc.MASK32
            elif a <= 0 or b <= 0:
                continue
            key = (b, a) if defect == "key_swapped" else (a, b)
            out[key] = out.get(key, 0) + (q0[r % C] if mesh else 1)
    if mesh and defect == "pair_sum_64":
        out = {k: v % (1 << 64) for k, v in out.items()}
    return out


def s_table(pairs, cap, defect=None):
    """The keys an open-addressing table of ``cap`` entries holds after the pairs went in (any order gives the same set
    while nothing overflows), and whether a probe sequence found no entry."""
    table, lost = [None] * cap, False
    for a, b in sorted(pairs):
        h, placed = oc.splitmix64(a << 32 | b) & (cap - 1), False
        for _ in range(cap):
            if h >= cap:  # ran off the end
                break
            if table[h] in (None, (a, b)):
                table[h], placed = (a, b), True
                break
            h = h + 1 if defect == "probe_no_wrap" else (h + 1) & (cap - 1)
        lost = lost or not placed
    return {k for k in table if k is not None}, lost


def s_row_max(ids, defect=None):
    out = []
    for t, row in enumerate(ids.tolist()):
        m = row[0] if defect == "neg_ids" else 0
        for v in row:
            m = v if v > m else m
        out.append(0 if defect == "rows_one_launch" and t >= oc.ROW_CAP else m)
    return np.array(out, np.int32)


def s_rank(r, defect=None):
    lab = r.labels.tolist()
    rank, n_t = [oc.POISON] * (r.T * r.C), []
    for t in range(r.T):
        run = 0
        for base in range(0, r.C, oc.RANK_CHUNK):
            n = 0
            for cc in range(base, min(base + oc.RANK_CHUNK, r.C)):
                if lab[t * r.C + cc] == (cc + 1 if defect == "rank_no_row" else t * r.C + cc + 1):
                    n += 1
                    rank[t * r.C + cc] = run + n
            run = run if defect == "rank_no_run" else run + n
        n_t.append(run)
    ids = [rank[v - 1] if 0 < v <= len(lab) else 0 for v in lab]
    return np.array(rank, np.int32), np.array(n_t, np.int32), np.array(ids, np.int32)


def results(name, defect=None):
    """Everything the device test compares on a field case, from the scalar restatement."""
    c = oc.get(name)
    out = {"overlaps": s_overlaps(c, False, defect), "mesh_overlaps": s_overlaps(c, True, defect),
           "row_max": s_row_max(c.ids, defect).tolist()}
    if c.tables:
        table = cells_by_piece(c, defect)
        sp = s_spans(c, defect, table)
        out["spans"] = [a.tolist() for a in sp[:3]] + [sp[3]]
        for mesh in (False, True):
            tid, mom = s_moments(c, mesh, defect, table)
            out["mesh" if mesh else "grid"] = (tid.tolist(), mom.tolist())
        if defect in (None, "compact_first"):
            out["compact"] = s_compact(c, sp, np.array(out["grid"][0], np.int64).reshape(-1, 2), defect).tolist()
    return out


@functools.lru_cache(maxsize=None)
def _clean(name):
    return results(name)


@pytest.mark.parametrize("name", oc.FIELD_NAMES)
def test_the_references_equal_the_scalar_restatement(name):
    c, e, got = oc.get(name), oc.expected(name), _clean(name)
    assert got["overlaps"] == e.overlaps and got["mesh_overlaps"] == e.mesh_overlaps
    assert got["row_max"] == e.row_max.tolist()
    assert e.minmax == (min(c.ids.reshape(-1).tolist()), max(c.ids.reshape(-1).tolist()))
    if c.tables:
        assert got["spans"] == [a.tolist() for a in e.spans[:3]] + [e.spans[3]]
        assert got["grid"] == (e.grid[0].tolist(), e.grid[1].tolist())
        assert got["mesh"] == (e.mesh[0].tolist(), e.mesh[1].tolist())
        assert got["compact"] == e.grid[0].tolist()


@pytest.mark.parametrize("defect", list(SEEN_BY))
def test_the_cases_built_for_a_defect_see_it(defect):
    for name in SEEN_BY[defect]:
        assert results(name, defect) != _clean(name), f"{name} does not notice: {DEFECTS[defect]}"


@pytest.mark.parametrize("name", oc.ALL_NAMES)
def test_the_case_meets_its_coverage_condition(name):
    oc.check_coverage(name)


def test_the_families_are_complete():
    sizes = {k: len(v) for k, v in oc.FAMILIES.items()}
    assert sizes == {"cell": 66, "nx": 10, "slice": 108, "seam": 4, "table": 22, "values": 6}
    assert len(oc.MINMAX_NAMES) == 21 and len(oc.HASH_NAMES) == 4 and len(oc.RANK_NAMES) == 22 and len(oc.AREA_NAMES) == 17
    assert len(set(oc.ALL_NAMES)) == len(oc.ALL_NAMES)
    assert {oc.get(n).C for n in oc.FAMILIES["cell"]} == set(oc.CELL_C)
    assert {oc.get(n).T for n in oc.FAMILIES["slice"]} == set(oc.SLICE_T) and {oc.get(n).C for n in oc.FAMILIES["slice"]} == set(oc.SLICE_C)
    assert {oc.get(n).nx for n in oc.FAMILIES["nx"]} == {1, 2, 3, 63, 64, 65, 100, 199, 200, 201}
    assert {oc.get(n).max_id for n in oc.FAMILIES["table"]} == set(oc.TABLE_MAX_ID)


def test_every_defect_is_covered():
    """The defects of the field stages are in SEEN_BY; the others have a test of their own below."""
    own = {"probe_no_wrap", "minmax_one_launch", "rows_one_launch", "rank_no_run", "rank_no_row"}
    assert set(SEEN_BY) | own == set(DEFECTS) and not set(SEEN_BY) & own and len(DEFECTS) >= 14
    for names in SEEN_BY.values():
        assert set(names) <= set(oc.FIELD_NAMES)


@pytest.mark.parametrize("name", oc.HASH_NAMES)
def test_the_hash_cases(name):
    oc.check_hash_coverage(name)
    h = oc.hash_case(name)
    stored, lost = s_table(h.pairs, h.cap)
    assert lost == (name == "hash-65-one-too-many") and len(stored) == min(len(h.pairs), h.cap) and stored <= set(h.pairs)
    stored, lost = s_table(h.pairs, h.cap, "probe_no_wrap")
    if name == "hash-128-one-window":  # every key's home is in the last eight entries: all but eight run off the end
        assert lost and len(stored) == 8
    c = type("C", (), dict(ids=h.ids, T=h.T, C=h.C, q=h.q0[None, :], max_id=0))
    assert s_overlaps(c, False) == oc.overlaps(h.ids) and s_overlaps(c, True) == oc.mesh_overlaps(h.ids, h.q0)


@pytest.mark.parametrize("name", oc.MINMAX_NAMES)
def test_the_minmax_cases(name):
    a = oc.minmax_case(name)
    lst = a.tolist()
    assert oc.minmax(a) == (min(lst), max(lst))
    n = int(name.split("-")[1])
    assert a.size == n and a.dtype == np.int32
    if n > 1:
        assert oc.minmax(a) == (oc.INT_MIN, oc.INT_MAX) and lst.count(oc.INT_MIN) == 1 and lst.count(oc.INT_MAX) == 1
    if n > oc.LAUNCH and not name.endswith("middle"):  # the one element past the launch width holds an extreme
        cut = lst[:oc.LAUNCH]
        assert (min(cut), max(cut)) != oc.minmax(a), DEFECTS["minmax_one_launch"]
    where = [oc.minmax_case(f"minmax-{n}-{w}").tolist() for w in ("minlast", "maxlast", "middle")]
    if n >= 257:
        assert (where[0][-1], where[0][0]) == (oc.INT_MIN, oc.INT_MAX) and (where[1][0], where[1][-1]) == (oc.INT_MIN, oc.INT_MAX)
        mid = where[2].index(oc.INT_MIN)
        assert 64 <= mid < n - 64 and where[2][mid + 1] == oc.INT_MAX and mid // 64 == (mid + 1) // 64


@pytest.mark.parametrize("name", oc.RANK_NAMES)
def test_the_rank_cases(name):
    oc.check_rank_coverage(name)
    r = oc.rank_case(name)
    want = oc.rank_roots(r.labels, r.T, r.C)
    for got, w in zip(s_rank(r), want):
        assert np.array_equal(got, w)
    if r.C > oc.RANK_CHUNK:
        assert not np.array_equal(s_rank(r, "rank_no_run")[0], want[0]), DEFECTS["rank_no_run"]
    if r.T > 1:
        assert not np.array_equal(s_rank(r, "rank_no_row")[1], want[1]), DEFECTS["rank_no_row"]


@pytest.mark.parametrize("name", oc.AREA_NAMES)
def test_the_long_cases(name):
    oc.check_long_coverage(name)
    c = oc.long_case(name)
    rm = oc.row_max(c.ids)
    assert np.array_equal(s_row_max(c.ids), rm)
    step = max(1, c.T // 512)  # the long cases row by row on a sample that holds the rows around 65 535, the others in full
    rows = sorted(set(range(0, c.T, step)) | {t for t in range(65530, 65537) if t < c.T})
    add, area = oc.add_row_offset(c.ids, c.off), oc.mesh_area(c.data, c.q0)
    q0 = c.q0.tolist()
    for t in rows:
        o = int(c.off[t])
        assert add[t].tolist() == [v + o if v > 0 else 0 for v in c.ids[t].tolist()], (name, t)
        assert int(area[t]) == sum(w for w, d in zip(q0, c.data[t].tolist()) if d), (name, t)
    if c.T > oc.ROW_CAP:  # the rows a launch of 65 535 rows leaves to its stride differ from what an unwritten row would hold
        assert not np.array_equal(s_row_max(c.ids, "rows_one_launch"), rm), DEFECTS["rows_one_launch"]
        assert rm[oc.ROW_CAP:].min() > 0 and (add[oc.ROW_CAP:] != 0).any() and area[oc.ROW_CAP:].max() > 0


def test_the_table_sizing_of_the_engine():
    runs = {1, 31, 32, 33} | {(1 << k) + d for k in range(1, 31) for d in (-1, 0, 1)}
    for r in sorted(runs):
        cap = pair_table_cap(r)
        assert cap == oc.table_cap(r) and cap >= 64 and cap & (cap - 1) == 0 and cap >= 2 * r, (r, cap)
        assert cap == 64 or cap < 4 * r, (r, cap)  # and no larger than the next power of two needs
