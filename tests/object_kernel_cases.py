"""Hand-placed cases and plain references for the object and overlap kernels (csrc/marex_objects.hip,
csrc/marex_mesh_objects.hip): no device.

The references are NumPy / Python integers written from the kernels' documented contracts: which cells count (values > 0),
what a slot, a pair, a root and an area are.  They know nothing of pieces, waves, tiles or strides.  The cases sit where
that launch geometry has an edge: a slice ends inside a 64-cell piece, an object straddles cell 1023 | 1024 or
4095 | 4096, an ID lives in slices t, t + 64, t + 128 (one workgroup's walk), an ID table ends at a multiple of 16 or of
4096, a hash table is exactly full.  ``check_coverage(name)`` asserts the property a case exists for.

A field case is used by the grid and the mesh kernels alike: it has ``ids`` int32 [T, C], a factoring C = ny * nx, a
weight table ``q`` int64 [4, C] (q[0] >= 0, a slice's sum below 2^62) and the ``max_id`` the tables are built for.
"""
import functools
from types import SimpleNamespace

import numpy as np

INT_MAX = 2147483647
INT_MIN = -2147483648
PIECE, WAVE_CELLS, GROUP_CELLS = 64, 1024, 4096  # cells of a piece, of a wave's walk, of a workgroup's
TSTRIDE = 64                                       # a workgroup walks every 64th slice
TILE, PER_THREAD, SCAN_THREADS = 4096, 16, 1024    # IDs per tile of the span scan, per thread, threads of the tile scan
LAUNCH = 256 * 8192                                # elements the flat kernels cover before they stride
RANK_CHUNK, RANK_WAVE = 8192, 512
ROW_CAP, ROW_WIDTH = 65535, 1024 * 256
POISON = -77
MASK32 = 0xFFFFFFFF


# ---------------------------------------------------------------------------------------------------------- references
def spans(ids, max_id):
    """``tmin`` (INT_MAX where absent), ``tmax`` (-1), ``off`` (exclusive prefix of the span lengths tmax - tmin + 1, an
    absent ID has length 0) and ``total`` of the IDs 0..max_id of ``ids`` [T, C]; values <= 0 are background."""
    ids = np.asarray(ids)
    nid = int(max_id) + 1
    tmin, tmax = np.full(nid, INT_MAX, np.int32), np.full(nid, -1, np.int32)
    t, c = np.nonzero(ids > 0)
    v = ids[t, c]
    np.minimum.at(tmin, v, t.astype(np.int32))
    np.maximum.at(tmax, v, t.astype(np.int32))
    length = np.where(tmax >= tmin, tmax.astype(np.int64) - tmin + 1, 0)
    return tmin, tmax, np.cumsum(length) - length, int(length.sum())


def _by_slot(ids, cols):
    """Rows (t, id) in that order and the int64 sums of ``cols`` (each [n cells with an ID]) over every row's cells."""
    t, c = np.nonzero(ids > 0)
    key = (t.astype(np.int64) << 32) | ids[t, c].astype(np.int64)
    uk, inv = np.unique(key, return_inverse=True)
    mom = np.zeros((len(uk), len(cols)), np.int64)
    for k, col in enumerate(cols):
        np.add.at(mom[:, k], inv, col(t, c))
    return np.stack([uk >> 32, uk & MASK32], axis=1), mom, inv


def grid_moments(ids, ny, nx):
    """``tid`` int64 [n, 2] = (t, id) in that order and ``mom`` int64 [n, 5]: cells, sum y, sum x, cells with
    x > nx // 2, flags (1: a cell with x < 100; 2: a cell with x >= nx - 100)."""
    ids = np.asarray(ids)
    one = lambda t, c: np.ones(len(c), np.int64)  # noqa: E731
    tid, mom, inv = _by_slot(ids, [one, lambda t, c: c // nx, lambda t, c: c % nx,
                                   lambda t, c: (c % nx > nx // 2).astype(np.int64), lambda t, c: np.zeros(len(c), np.int64)])
    x = np.nonzero(ids > 0)[1] % nx
    left, right = np.zeros(len(tid), bool), np.zeros(len(tid), bool)
    np.logical_or.at(left, inv, x < 100)
    np.logical_or.at(right, inv, x >= nx - 100)
    mom[:, 4] = left + 2 * right.astype(np.int64)
    return tid, mom


def mesh_moments(ids, q):
    """``tid`` as above and ``mom`` int64 [n, 5]: cells and the exact signed sums of q[0..3] over the row's cells."""
    ids = np.asarray(ids)
    cols = [lambda t, c: np.ones(len(c), np.int64)] + [lambda t, c, k=k: q[k][c] for k in range(4)]
    tid, mom, _ = _by_slot(ids, cols)
    return tid, mom


def slots(tid, mom, sp):
    """The dense slot table [total, 5] of ``spans`` output ``sp``: slot = off[id] + t - tmin[id]; slots nobody fills stay 0."""
    tmin, _, off, total = sp
    acc = np.zeros((total, mom.shape[1]), np.int64)
    acc[off[tid[:, 1]] + tid[:, 0] - tmin[tid[:, 1]]] = mom
    return acc


def _pairs(ids):
    ids = np.asarray(ids)
    a, b = ids[:-1], ids[1:]
    t, c = np.nonzero((a > 0) & (b > 0))
    return (a[t, c].astype(np.int64) << 32) | b[t, c].astype(np.int64), c


def overlaps(ids):
    """{(a, b): cells} over all t < T - 1 with a = ids[t][c] > 0 and b = ids[t + 1][c] > 0."""
    key, _ = _pairs(ids)
    uk, n = np.unique(key, return_counts=True)
    return {(int(k) >> 32, int(k) & MASK32): int(v) for k, v in zip(uk, n)}


def mesh_overlaps(ids, q0):
    """{(a, b): sum of q0 over the shared cells}, an unbounded Python integer."""
    key, c = _pairs(ids)
    uk, inv = np.unique(key, return_inverse=True)
    lo, hi = np.zeros(len(uk), np.int64), np.zeros(len(uk), np.int64)  # each half stays far below 2^63
    np.add.at(lo, inv, q0[c] & MASK32)
    np.add.at(hi, inv, q0[c] >> 32)
    return {(int(k) >> 32, int(k) & MASK32): (int(h) << 32) + int(l) for k, l, h in zip(uk, lo, hi)}


def minmax(a):
    return int(np.min(a)), int(np.max(a))


def row_max(ids):
    return np.maximum(np.asarray(ids).max(axis=1), 0).astype(np.int32)


def add_row_offset(ids, off):
    ids = np.asarray(ids)
    return np.where(ids > 0, ids + np.asarray(off, np.int32)[:, None], 0).astype(np.int32)


def rank_roots(labels, T, C):
    """``rank`` int32 [T * C] (1 + the roots of the slice below the cell, at root cells; POISON elsewhere: not written),
    ``n_t`` int32 [T] and ``ids`` int32 [T * C] (the rank of the cell's root, 0 for background).  A root is
    labels[t * C + c] == t * C + c + 1."""
    lab = np.asarray(labels).reshape(T, C).astype(np.int64)
    root = lab == np.arange(T * C, dtype=np.int64).reshape(T, C) + 1
    r = np.cumsum(root, axis=1)
    rank = np.where(root, r, POISON).astype(np.int32).reshape(-1)
    flat = lab.reshape(-1)
    ids = np.where(flat > 0, rank[np.maximum(flat, 1) - 1], 0).astype(np.int32)
    return rank, root.sum(axis=1).astype(np.int32), ids


def mesh_area(data, q0):
    return ((np.asarray(data) != 0) * q0[None, :].astype(np.int64)).sum(axis=1)


def splitmix64(k):
    m = (1 << 64) - 1
    k ^= k >> 30
    k = k * 0xBF58476D1CE4E5B9 & m
    k ^= k >> 27
    k = k * 0x94D049BB133111EB & m
    return k ^ (k >> 31)


def table_cap(runs):
    """The engine's sizing of the pair table, restated: a power of two >= 64 and >= 2 * runs."""
    return max(64, 1 << (2 * runs - 1).bit_length())


# ---------------------------------------------------------------------------------------------------------- field cases
FACTORS = {1: (1, 1), 63: (9, 7), 64: (8, 8), 65: (5, 13), 70: (7, 10), 1023: (33, 31), 1024: (32, 32), 1025: (25, 41),
           4095: (63, 65), 4096: (64, 64), 4097: (17, 241), 8193: (3, 2731)}
CELL_C = [1, 63, 64, 65, 1023, 1024, 1025, 4095, 4096, 4097, 8193]
CELL_FIELDS = ["one", "alt", "each", "straddle", "last", "tail"]
NX_SHAPES = [(130, 1), (70, 2), (50, 3), (5, 63), (5, 64), (5, 65), (4, 100), (3, 199), (3, 200), (3, 201)]
SLICE_T = [1, 2, 63, 64, 65, 66, 128, 129, 130]
SLICE_C = [70, 4097]
SLICE_FIELDS = ["every64", "gap64", "change64", "const", "lastpair", "midgap"]
SEAM_NX = [100, 199, 200, 201]
TABLE_MAX_ID = [1, 15, 16, 17, 4095, 4096, 4097, 8191, 8192, 4096 * 1024 - 1, 4096 * 1024 + 5]
_BUILD = {}
FAMILIES = {}


def _case(family, name):
    def deco(fn):
        _BUILD[name] = (family, fn)
        FAMILIES.setdefault(family, []).append(name)
        return fn
    return deco


def weights(C, seed, bits=31):
    """q [4, C]: q[0] in [0, 2^bits), q[1..3] signed of the same size; a piece's 64-cell sum of q[0] needs the high word."""
    rng = np.random.default_rng(seed)
    q = rng.integers(-(1 << bits), 1 << bits, size=(4, C), dtype=np.int64)
    q[0] = np.abs(q[0])
    return q


def _field(ids, ny, nx, max_id=None, q=None, tables=True, **marks):
    ids = np.ascontiguousarray(ids, dtype=np.int32)
    T, C = ids.shape
    assert C == ny * nx
    q = weights(C, C + 7 * T) if q is None else np.ascontiguousarray(q, dtype=np.int64)
    assert q.shape == (4, C) and q[0].min() >= 0 and int(q[0].sum()) < 1 << 62
    if max_id is None:
        max_id = max(int(ids.max()), 0)
    assert not tables or int(ids.max()) <= max_id
    return SimpleNamespace(ids=ids, T=T, C=C, ny=ny, nx=nx, q=q, max_id=int(max_id), tables=tables, marks=marks)


def _edges(C):
    return [b for b in (PIECE, WAVE_CELLS, GROUP_CELLS, 2 * GROUP_CELLS) if b < C]


def _cell_field(C, kind):
    ny, nx = FACTORS[C]
    T = 3
    ids = np.zeros((T, C), np.int32)
    c = np.arange(C)
    if kind == "one":
        ids[:] = 3
    elif kind == "alt":
        ids[:] = 1 + (c % 2)
        ids[1] = 2 - (c % 2)
    elif kind == "each":
        for t in range(T):
            ids[t] = (c + t) % C + 1
    elif kind == "straddle":  # object k: the last cell before an edge and the first behind it
        for k, b in enumerate(_edges(C)):
            ids[:, b - 1:b + 1] = k + 1
        ids[1] = np.where(ids[1] > 0, ids[1] + 4, 0)
    elif kind == "last":
        ids[:, C - 1] = 2
        ids[2, C - 1] = 5
    else:  # tail: what lies behind the slice's end in memory (the next slice's first cells) differs from background
        ids[:, C - 1] = 2
        ids[1:, :min(C, PIECE)] = 5
        ids[2, :min(C, PIECE)] = 6
    return _field(ids, ny, nx, kind=kind)


for _C in CELL_C:
    for _k in CELL_FIELDS:
        _case("cell", f"cell-{_C}-{_k}")(functools.partial(_cell_field, _C, _k))


def _nx_field(ny, nx):
    rng = np.random.default_rng(ny * 1000 + nx)
    ids = rng.choice(np.array([0, 1, 1, 1, 1, 1, 2, 3], np.int32), size=(2, ny * nx))  # scattered over every piece, 1 the most
    return _field(ids, ny, nx, kind="nx")


for _ny, _nx in NX_SHAPES:
    _case("nx", f"nx-{_ny}x{_nx}")(functools.partial(_nx_field, _ny, _nx))


def slice_marks(T):
    t0 = min(1, T - 1)
    mid = T // 2 - 2 if T >= 5 else None
    return t0, mid


def _slice_field(T, C, kind):
    ny, nx = FACTORS[C]
    ids = np.zeros((T, C), np.int32)
    cells = [0, 1, C - 1]  # C = 4097: cell 4096 is the second workgroup's only cell
    t0, mid = slice_marks(T)
    vis = [t for t in (t0, t0 + TSTRIDE, t0 + 2 * TSTRIDE) if t < T]
    q = None
    if kind == "every64":
        for t in vis:
            ids[t, cells] = 1
    elif kind == "gap64":
        for t in vis[::2]:
            ids[t, cells] = 2
    elif kind == "change64":
        for k, t in enumerate(vis):
            ids[t, cells] = 3 + k % 2
    elif kind == "const":
        ids[:] = 7
    elif kind == "lastpair":
        if T >= 2:
            ids[T - 2, cells] = 5
            ids[T - 1, cells] = 6
    else:
        ids[:, cells] = 7
        ids[:, 2] = 9
        if mid is not None:
            ids[mid] = 0
    return _field(ids, ny, nx, q=q, kind=kind, t0=t0, mid=mid, vis=vis, cells=cells)


for _T in SLICE_T:
    for _C in SLICE_C:
        for _k in SLICE_FIELDS:
            _case("slice", f"slice-T{_T}-C{_C}-{_k}")(functools.partial(_slice_field, _T, _C, _k))


def _seam_field(nx):
    """Row k of a [8, nx] slice holds object k: 1 at x = 99, 2 at x = 100, 3 at x = nx - 100, 4 at x = nx - 101, 5 at
    x = 0 and x = nx - 1 (one cell each), 6 at x = nx // 2, 7 at x = nx // 2 + 1 (columns outside the slice: no object)."""
    ny = 8
    ids = np.zeros((2, ny, nx), np.int32)
    at = {1: [99], 2: [100], 3: [nx - 100], 4: [nx - 101], 5: [0, nx - 1], 6: [nx // 2], 7: [nx // 2 + 1]}
    for k, xs in at.items():
        for x in xs:
            if 0 <= x < nx:
                ids[:, k, x] = k
    return _field(ids.reshape(2, -1), ny, nx, kind="seam", at=at)


for _nx in SEAM_NX:
    _case("seam", f"seam-{_nx}")(functools.partial(_seam_field, _nx))


def table_present(max_id, variant):
    """The IDs present: variant a takes k * 16 - 1 and k * 4096 - 1 and leaves k * 16 and k * 4096 empty, b the reverse;
    both have 40 and 60 with nothing between (20 empty spans) and, where they fit, the table's last ID (a) or not (b)."""
    lows = [15, 31, 4095, 8191, 4096 * 1024 - 1]
    highs = [16, 32, 4096, 8192, 4096 * 1024]
    want = set(lows if variant == "a" else highs) | {1, 17 if variant == "a" else 14, 4097 if variant == "a" else 4094}
    want -= set(range(41, 60))
    want |= {40, 60}
    want = {k for k in want if 1 <= k <= max_id}
    want = want | {max_id} if variant == "a" else want - {max_id}
    return sorted(want) if want else ([1] if variant == "a" else [])


def _table_field(max_id, variant):
    T = 5
    present = table_present(max_id, variant)
    C = 2 * len(present) + 3
    ids = np.zeros((T, C), np.int32)
    for j, k in enumerate(present):
        rows = ([2], list(range(T)), [0, 4])[j % 3]  # a span of one step, of T steps, and one with three empty slots inside
        for t in rows:
            ids[t, 2 * j:2 * j + 2] = k
    return _field(ids, 1, C, max_id=max_id, kind="table", present=present)


for _m in TABLE_MAX_ID:
    for _v in "ab":
        _case("table", f"table-{_m}-{_v}")(functools.partial(_table_field, _m, _v))


@_case("values", "values-negative")
def _values_negative():
    rng = np.random.default_rng(5)
    ids = rng.choice(np.array([INT_MIN, -5, -1, 0, 1, 2, 3], np.int64), size=(4, 130)).astype(np.int32)
    ids[2] = np.where(ids[2] > 0, -ids[2], ids[2])  # a slice without a positive value
    ids[0, 0], ids[1, 0], ids[0, 1], ids[1, 1] = -1, 1, 2, INT_MIN
    return _field(ids, 10, 13, max_id=3, kind="negative")


@_case("values", "values-big-id")
def _values_big_id():
    ids = np.zeros((3, 70), np.int32)
    ids[:, 5:9] = INT_MAX - 1
    ids[1, 5] = 4
    ids[:, 69] = -3
    return _field(ids, 7, 10, tables=False, kind="big-id")


def _q_field(kind):
    rng = np.random.default_rng(11)
    C = 200
    ids = rng.integers(0, 4, size=(3, C)).astype(np.int32)
    if kind == "q-big":
        q = weights(C, 12, bits=40)
    elif kind == "q-zero":
        q = weights(C, 13)
        q[:, ids[0] == 1] = 0
        q[0, ::2] = 0
    else:
        q = weights(C, 14)
        q[1:] = -np.abs(q[1:]) - 1
    return _field(ids, 2, 100, q=q, kind=kind)


for _k in ("q-negative", "q-big", "q-zero"):
    _case("values", f"values-{_k}")(functools.partial(_q_field, _k))


@_case("values", "values-pair-sum-above-64-bits")
def _values_long_pair():
    q = np.zeros((4, 70), np.int64)
    q[0] = 1 << 55  # a slice: 70 * 2^55 < 2^62; the pair (7, 7) over 129 steps: more than 2^64
    return _field(np.full((130, 70), 7, np.int32), 7, 10, q=q, kind="long-pair")


FIELD_NAMES = list(_BUILD)


@functools.lru_cache(maxsize=None)
def get(name):
    return _BUILD[name][1]()


def family_of(name):
    return _BUILD[name][0]


@functools.lru_cache(maxsize=None)
def expected(name):
    """Every reference of a field case, computed once: do not modify."""
    c = get(name)
    out = SimpleNamespace(minmax=minmax(c.ids), row_max=row_max(c.ids), overlaps=overlaps(c.ids),
                          mesh_overlaps=mesh_overlaps(c.ids, c.q[0]))
    out.cells = sum(out.overlaps.values())
    if c.tables:
        out.spans = spans(c.ids, c.max_id)
        out.grid = grid_moments(c.ids, c.ny, c.nx)
        out.mesh = mesh_moments(c.ids, c.q)
    return out


def _run_cells(ids, v):
    """The flat cell indices of the runs of value v in a slice."""
    return np.nonzero(ids == v)[0]


def check_coverage(name):
    """The property the case exists for (any case of this module, by its name)."""
    for prefix, check in (("hash-", check_hash_coverage), ("rank-", check_rank_coverage), ("long-", check_long_coverage),
                          ("minmax-", check_minmax_coverage)):
        if name.startswith(prefix):
            return check(name)
    c, e, fam = get(name), expected(name), family_of(name)
    k = c.marks["kind"]
    ids, T, C = c.ids, c.T, c.C
    assert ids.size <= 600_000 and ids.dtype == np.int32
    if fam == "cell":
        assert T == 3 and C in CELL_C
        if k == "one":
            assert e.spans[3] == T and e.grid[1][:, 0].tolist() == [C] * T and e.overlaps == {(3, 3): 2 * C}
            for b in _edges(C):
                assert ids[0, b - 1] == ids[0, b]  # one run crosses every piece, wave and workgroup edge
        elif k == "alt":
            assert C == 1 or (ids[0, :-1] != ids[0, 1:]).all()
        elif k == "each":
            assert len(np.unique(ids[0])) == C and c.max_id == C and len(e.overlaps) == C
        elif k == "straddle":
            for j, b in enumerate(_edges(C)):
                assert _run_cells(ids[0], j + 1).tolist() == [b - 1, b]
            assert (ids > 0).sum() == 3 * 2 * len(_edges(C))
        elif k == "last":
            assert np.nonzero(ids[0])[0].tolist() == [C - 1] and e.overlaps == {(2, 2): 1, (2, 5): 1}
        else:
            flat = ids.reshape(-1)
            if C % PIECE:  # the cells behind slice 0 in memory hold an ID that slice 0 does not have
                assert flat[C] == 5 and 5 not in ids[0] and (C == 1 or ids[0, C - 1] == 2)
    elif fam == "nx":
        lane = np.arange(C) % PIECE
        dy = np.arange(C) // c.nx - (np.arange(C) - lane) // c.nx
        assert dy.max() >= (PIECE - 1) // c.nx and (c.nx > 3 or dy.max() >= 21)
        if c.nx <= 3:  # some group of one piece adds up more than 8 bits of dy
            piece = np.arange(C) // PIECE
            best = max(int(dy[(piece == p) & (ids[0] == v)].sum()) for p in range((C + 63) // 64) for v in (1, 2, 3))
            assert best >= 256
    elif fam == "slice":
        t0, mid, vis, cells = (c.marks[m] for m in ("t0", "mid", "vis", "cells"))
        assert T in SLICE_T and C in SLICE_C and cells[-1] == C - 1 and (C < GROUP_CELLS or cells[-1] // GROUP_CELLS == 1)
        present = sorted(set(np.nonzero((ids > 0).any(axis=1))[0].tolist()))
        if k == "every64":
            assert present == vis and all(b - a == TSTRIDE for a, b in zip(vis, vis[1:])) and (T < 66 or len(vis) >= 2)
        elif k == "gap64":
            assert present == vis[::2] and (T < 130 or (present == [1, 129] and e.spans[3] == 129 and not e.overlaps))
        elif k == "change64":
            assert [int(ids[t, 0]) for t in vis] == [3, 4, 3][:len(vis)]
        elif k == "const":
            assert e.spans[0][7] == 0 and e.spans[1][7] == T - 1 and (T == 1 or e.overlaps == {(7, 7): (T - 1) * C})
            if T >= 63:  # the pieces' low words add up to more than one word
                assert sum(int(c.q[0][p:p + PIECE].sum()) & MASK32 for p in range(0, C, PIECE)) * (T - 1) >= 1 << 32
        elif k == "lastpair":
            assert T < 2 or (e.overlaps == {(5, 6): 3} and present == [T - 2, T - 1])
        else:
            assert mid is None or (mid not in present and mid - 1 in present and mid + 1 in present and 0 < mid < T - 2)
            assert T < 63 or mid is not None
    elif fam == "seam":
        fl = {int(i): int(f) for (t, i), f in zip(e.grid[0], e.grid[1][:, 4]) if t == 0}
        nr = {int(i): int(f) for (t, i), f in zip(e.grid[0], e.grid[1][:, 3]) if t == 0}
        nx = c.nx
        assert fl[1] & 1 and fl[3] & 2 and fl[5] == 3 and e.grid[1][e.grid[0][:, 1] == 5][:, 0].tolist() == [2, 2]
        assert nx == 100 or not fl[2] & 1
        assert nx == 100 or not fl[4] & 2
        assert nr[6] == 0 and nr[7] == 1
    elif fam == "table":
        present, tmin, tmax, off, total = c.marks["present"], *e.spans
        nid = c.max_id + 1
        assert present == sorted(set(ids[ids > 0].tolist())) and (name[-1] == "b" or c.max_id in present)
        assert name[-1] == "a" or c.max_id not in present  # b: trailing empty spans
        length = np.where(tmax >= tmin, tmax - tmin + 1, 0)
        for edge in (PER_THREAD, TILE):
            for kk in range(edge, nid, edge):
                if kk in (16, 32, 4096, 8192, 4096 * 1024) and kk != c.max_id:
                    assert (length[kk - 1] > 0) != (length[kk] > 0) and (length[kk] > 0) == (name[-1] == "b")
        if c.max_id >= 60:
            assert not length[41:60].any() and length[40] and length[60]
        if len(present) >= 3:
            assert {1, 5} <= set(length[present].tolist()) and total > e.grid[0].shape[0]  # slots that stay empty
    elif k == "negative":
        assert INT_MIN in ids and (ids[2] <= 0).all() and (ids[2] < 0).any() and e.row_max[2] == 0 and e.minmax[0] == INT_MIN
        assert (ids[0, 0], ids[1, 0], ids[0, 1], ids[1, 1]) == (-1, 1, 2, INT_MIN) and all(a > 0 and b > 0 for a, b in e.overlaps)
    elif k == "big-id":
        assert e.minmax == (-3, INT_MAX - 1) and (INT_MAX - 1, INT_MAX - 1) in e.overlaps and (INT_MAX - 1, 4) in e.overlaps
    elif k == "q-negative":
        assert (c.q[1:] < 0).all() and (e.mesh[1][:, 2:] < 0).all()
    elif k == "q-big":
        assert np.abs(c.q).max() >= 1 << 39 and max(e.mesh_overlaps.values()) >= 1 << 40
    elif k == "q-zero":
        assert (e.mesh[1][e.mesh[0][:, 0] == 0][0, 1:] == 0).all() and (c.q[0] == 0).sum() >= 100
    elif k == "long-pair":
        assert e.mesh_overlaps[(7, 7)] >= 1 << 64
    else:
        raise AssertionError(name)


# ---------------------------------------------------------------------------------------------------------- min / max
MINMAX_N = [1, 255, 256, 257, LAUNCH - 1, LAUNCH, LAUNCH + 1]
MINMAX_NAMES = [f"minmax-{n}-{w}" for n in MINMAX_N for w in ("minlast", "maxlast", "middle")]


def minmax_case(name):
    """Values in -1000..1000 with INT_MIN and INT_MAX once each: the minimum in the last element and the maximum in the
    first, the reverse, or both in a wave in the middle (n = 1: the one random element is both)."""
    _, n, where = name.split("-")
    n = int(n)
    a = np.random.default_rng(n).integers(-1000, 1001, size=n).astype(np.int32)
    mid = n // 2 // 64 * 64
    lo, hi = {"minlast": (n - 1, 0), "maxlast": (0, n - 1), "middle": (min(mid + 5, n - 1), min(mid + 6, n - 1))}[where]
    if lo != hi:
        a[lo], a[hi] = INT_MIN, INT_MAX
    return a


def check_minmax_coverage(name):
    a, n = minmax_case(name), int(name.split("-")[1])
    assert a.size == n and a.dtype == np.int32
    if n > 1:
        lo, hi = int(np.argmin(a)), int(np.argmax(a))
        assert minmax(a) == (INT_MIN, INT_MAX) and (a == INT_MIN).sum() == 1 and (a == INT_MAX).sum() == 1
        want = {"minlast": (n - 1, 0), "maxlast": (0, n - 1)}.get(name.split("-")[2])
        assert (lo, hi) == want if want else (hi == lo + 1 and lo // 64 == hi // 64 and (n < 257 or 64 <= lo < n - 64))


# ---------------------------------------------------------------------------------------------------------- hash tables
HASH_NAMES = ["hash-64-full", "hash-65-one-too-many", "hash-40-out-39", "hash-128-one-window"]


@functools.lru_cache(maxsize=None)
def hash_case(name):
    """``ids`` [2, C] whose pairs are exactly the listed keys (pair j in 1 + j % 3 cells), the table's ``cap`` and the room
    ``out_cap`` of the output; ``q0`` for the mesh table."""
    n = {"hash-64-full": 64, "hash-65-one-too-many": 65, "hash-40-out-39": 40, "hash-128-one-window": 64}[name]
    cap = 128 if name == "hash-128-one-window" else 64
    out_cap = 39 if name == "hash-40-out-39" else n
    if cap == 128:  # homes 120..127: the probes run on past the table's end and wrap to its start
        pairs, a = [], 1
        while len(pairs) < n:
            for b in range(1, 40):
                if len(pairs) < n and splitmix64(a << 32 | b) & (cap - 1) >= cap - 8:
                    pairs.append((a, b))
            a += 1
    else:
        pairs = [(j + 1, 1000 - 3 * j) for j in range(n)]
    cols = [p for j, p in enumerate(pairs) for _ in range(1 + j % 3)]
    ids = np.array(cols, np.int32).T.copy()
    q0 = weights(ids.shape[1], n, bits=40)[0]
    return SimpleNamespace(ids=ids, T=2, C=ids.shape[1], q0=q0, pairs=pairs, cap=cap, out_cap=out_cap)


def check_hash_coverage(name):
    h = hash_case(name)
    want = overlaps(h.ids)
    assert sorted(want) == sorted(h.pairs) and len(set(h.pairs)) == len(h.pairs)
    assert {want[p] for p in h.pairs} == {1, 2, 3}
    if name == "hash-64-full":
        assert len(want) == h.cap == h.out_cap == 64
    elif name == "hash-65-one-too-many":
        assert len(want) == h.cap + 1
    elif name == "hash-40-out-39":
        assert len(want) == 40 == h.out_cap + 1 and len(want) <= h.cap // 2 + 8
    else:
        homes = [splitmix64(a << 32 | b) & 127 for a, b in h.pairs]
        assert min(homes) >= 120 and len(homes) == 64  # 64 keys from 8 homes: probes of up to 63 steps, most of them wrapped


# ---------------------------------------------------------------------------------------------------------- mesh rank
RANK_C = [1, 64, 511, 512, 513, 8191, 8192, 8193, 16384, 16385, 24577]
RANK_NAMES = [f"rank-T{T}-C{C}" for C in RANK_C for T in (1, 3)]
RANK_FORCED = [0, 511, 512, 8191, 8192, 16383, 16384]


@functools.lru_cache(maxsize=None)
def rank_case(name):
    """Labels of a random partition of every slice: about one cell in five is a root, the forced cells and C - 1 always;
    every other cell is background or carries the label of some root of its slice.  With T = 3 slice 1 has no root and
    slice 2 has only roots."""
    T, C = int(name.split("-")[1][1:]), int(name.split("-")[2][1:])
    rng = np.random.default_rng(T * 100003 + C)
    lab = np.zeros((T, C), np.int32)
    for t in range(T):
        if T == 3 and t == 1:
            continue
        root = rng.random(C) < 0.2 if not (T == 3 and t == 2) else np.ones(C, bool)
        root[[c for c in RANK_FORCED + [C - 1] if c < C]] = True
        rc = np.nonzero(root)[0]
        pick = rc[rng.integers(0, len(rc), size=C)]
        lab[t] = np.where(rng.random(C) < 0.3, 0, t * C + pick + 1)
        lab[t, rc] = t * C + rc + 1
    return SimpleNamespace(labels=lab.reshape(-1), T=T, C=C)


def check_rank_coverage(name):
    r = rank_case(name)
    rank, n_t, ids = rank_roots(r.labels, r.T, r.C)
    lab = r.labels.reshape(r.T, r.C)
    for t in ([0] if r.T == 1 else [0, 2]):
        for c in RANK_FORCED + [r.C - 1]:
            if c < r.C:
                assert lab[t, c] == t * r.C + c + 1
    if r.T == 3:
        assert n_t[1] == 0 and n_t[2] == r.C and (ids.reshape(3, -1)[2] == np.arange(1, r.C + 1)).all()
    # a third and a fourth chunk: both LDS buffers are reused
    assert (r.C - 1) // RANK_CHUNK == {16385: 2, 24577: 3}.get(r.C, (r.C - 1) // RANK_CHUNK)
    assert ids.max() == n_t.max() and ((rank == POISON) == (r.labels != np.arange(1, r.T * r.C + 1))).all()


# ---------------------------------------------------------------------------------------------------------- long rows
LONG_NAMES = ([f"long-T{T}-C{C}" for T in (65534, 65535, 65536, 65537) for C in (1, 3)]
              + [f"long-T2-C{C}" for C in (255, 256, 257, ROW_WIDTH - 1, ROW_WIDTH, ROW_WIDTH + 1)])
AREA_NAMES = LONG_NAMES + [f"long-T3-C{C}" for C in (4095, 4096, 4097)]


@functools.lru_cache(maxsize=4)
def long_case(name):
    """``ids`` [T, C] of small IDs, zeros and negatives whose rows 65 534, 65 535 and 65 536 (where they exist) have maxima
    found nowhere else, offsets of both signs, ``data`` uint8 of 0, 1, 2, 128 and 255 and weights ``q0``."""
    T, C = int(name.split("-")[1][1:]), int(name.split("-")[2][1:])
    rng = np.random.default_rng(T + 7 * C)
    ids = rng.integers(-3, 50, size=(T, C)).astype(np.int32)
    for k, t in enumerate((65534, 65535, 65536)):
        if t < T:
            ids[t, C - 1] = 1000 + k
    ids[0, C - 1] = 77  # the last cell of a row: behind the width cap at C = 262 145
    if T > 1:
        ids[1] = np.minimum(ids[1], 0)
    off = rng.integers(-40, 1000, size=T).astype(np.int32)
    off[0], off[T - 1] = -3, 5
    data = rng.choice(np.array([0, 0, 1, 2, 128, 255], np.uint8), size=(T, C))
    for t, v in ((65534, 0), (65535, 2), (65536, 0)):
        if t < T:
            data[t] = v
    data[T - 1, C - 1] = 255
    return SimpleNamespace(ids=ids, T=T, C=C, off=off, data=data, q0=weights(C, C, bits=40)[0])


def check_long_coverage(name):
    c = long_case(name)
    rm = row_max(c.ids)
    for k, t in enumerate((65534, 65535, 65536)):
        if t < c.T:
            assert rm[t] == 1000 + k and (rm == 1000 + k).sum() == 1
    assert (c.off < 0).any() and (c.off > 0).any() and rm[0] >= 77 and (c.T == 1 or rm[1] == 0)
    assert set(np.unique(c.data).tolist()) <= {0, 1, 2, 128, 255} and c.data[-1, -1] == 255 and c.ids.size <= 600_000
    a = mesh_area(c.data, c.q0)
    assert c.T <= 65535 or a[65535] == c.q0.sum() > 0
    assert c.T <= 65536 or (a[65534] == 0 and a[65536] == c.q0[-1] > 0)


ALL_NAMES = FIELD_NAMES + MINMAX_NAMES + HASH_NAMES + RANK_NAMES + AREA_NAMES
