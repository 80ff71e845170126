"""Hand-placed, seeded cases for the grid partition and relabel kernels of the merge tracker (k_mrg_part_centroid,
k_mrg_nn_buckets, k_mrg_scan, k_mrg_part_nn, k_mrg_relabel): plain NumPy, no device.  Not a test module.

A partition case is a namespace with the arguments of ``HotPath.partition_centroid`` / ``partition_nn``: ``ny, nx, wrap``,
the slices ``cur`` and ``prev`` (int32 ``[ny, nx]``), ``child_keys`` (ascending), ``off``, and per parent entry ``parents``,
``pcy``, ``pcx``, ``lab``, ``maxd`` (one ``max_distance`` per child, repeated over its entries, as the reference has it).
``marks`` names the cells a family is about.  ``expected(case, nn)`` is the slice the oracle of merge_oracle.py gives,
child by child.  Objects are small: child cells x parent cells stays far below 2e7 per case.

Families (``FAMILIES[name]`` lists the case names, ``get(name)`` builds one, cached):
  a  shape matrix: six shapes x wrap x k parents, bucket sizes 2, 3 and 10 rotated over them; one child across the x seam
     (bottom rows) and one in the interior (top rows, all rows on the low grids)
  b  1, 2 or 3 buckets along each axis (bucket size 10, larger than the grid for the 1s)
  c  two and three children that share one parent, each child with its own max_distance
  d  one long child: the near end takes the nearest-cell rule, the rest the centroid fallback
  e  an exact tie between two parents, the distance cap, |dx| = nx / 2 on an even nx, equal roots of unequal squares
  f  ny = 2 with exact bucket totals around the 1024 threads of the scan
  g  1025 x 2048 cells: more than the 8192 x 256 threads of one launch
Relabel cases (family h) come from ``relabel_cases()``.
"""
import functools
from types import SimpleNamespace

import numpy as np

import merge_oracle as mo

I32_MAX = 2 ** 31 - 1
#: cells one launch covers without looping: 8192 workgroups of 256 threads
LAUNCH_CELLS = 256 * 8192


def bucket_size(maxd):
    return max(2, int(maxd) // 4)


def bucket_counts(ny, nx, maxd):
    gs = bucket_size(maxd)
    return (ny + gs - 1) // gs, (nx + gs - 1) // gs


def total_buckets(case):
    """The documented size of the bucket table: ``ngy * ngx`` summed over the parent entries."""
    return sum(int(np.prod(bucket_counts(case.ny, case.nx, m))) for m in case.maxd)


class _Builder:
    def __init__(self, name, ny, nx, wrap):
        self.name, self.ny, self.nx, self.wrap = name, ny, nx, bool(wrap)
        self.cur = np.zeros((ny, nx), np.int32)
        self.prev = np.zeros((ny, nx), np.int32)
        self.child_keys, self.off = [], [0]
        self.parents, self.pcy, self.pcx, self.lab, self.maxd = [], [], [], [], []
        self.marks = {}
        self._next = 1000

    def rect(self, arr, val, y0, y1, x0, x1):
        """``val`` on rows y0..y1-1, columns x0..x1-1 taken modulo nx."""
        for x in range(x0, x1):
            arr[y0:y1, x % self.nx] = val

    def centroid(self, pid):
        """Mean cell of parent ``pid`` in ``prev`` (columns unwrapped when the object spans more than half the grid)."""
        ys, xs = np.nonzero(self.prev == pid)
        assert ys.size, (self.name, pid)
        xs = xs.astype(np.float64)
        if xs.max() - xs.min() > self.nx / 2:
            xs[xs < self.nx / 2] += self.nx
        return float(ys.mean()), float(xs.mean() % self.nx)

    def child(self, key, parents, maxd, centroids=None, keep_id=True):
        """Child ``key`` (painted in ``cur``) with its parents (painted in ``prev``), in this order; the first keeps the
        child's ID (unless ``keep_id`` is off), the others get fresh labels."""
        assert not self.child_keys or key > self.child_keys[-1], "children in ascending order"
        assert (self.cur == key).any(), (self.name, key)
        self.child_keys.append(key)
        for j, p in enumerate(parents):
            cy, cx = self.centroid(p) if centroids is None else centroids[j]
            self.parents.append(p)
            self.pcy.append(cy)
            self.pcx.append(cx)
            fresh = j > 0 or not keep_id
            self.lab.append(self._next if fresh else key)
            self._next += fresh
            self.maxd.append(int(maxd))
        self.off.append(len(self.parents))

    def done(self, family):
        return SimpleNamespace(name=self.name, family=family, ny=self.ny, nx=self.nx, wrap=self.wrap, cur=self.cur,
                               prev=self.prev, child_keys=np.array(self.child_keys, np.int32), off=np.array(self.off, np.int32),
                               parents=np.array(self.parents, np.int32), pcy=np.array(self.pcy, np.float64),
                               pcx=np.array(self.pcx, np.float64), lab=np.array(self.lab, np.int32),
                               maxd=np.array(self.maxd, np.int32), marks=self.marks,
                               gs_of=lambda j, m=tuple(self.maxd): bucket_size(m[j]))


def _scatter_parents(b, rng, first_id, k, y0, y1, x0, x1):
    """k parents ``first_id ..`` in ``prev``: parent j gets one free cell of rows y0..y1-1 in the j-th of k equal column
    ranges of x0..x1-1 (modulo nx), so that every parent is some cell's nearest, grown by its right neighbour when that
    is free."""
    picked = []
    for j in range(k):
        a, e = x0 + (x1 - x0) * j // k, x0 + (x1 - x0) * (j + 1) // k
        spots = [(y, x % b.nx) for y in range(max(y0, 0), min(y1, b.ny)) for x in range(a, e) if b.prev[y, x % b.nx] == 0]
        picked.append(spots[int(rng.integers(len(spots)))])
        b.prev[picked[-1]] = first_id + j
    for j, (y, x) in enumerate(picked):
        if b.prev[y, (x + 1) % b.nx] == 0 and rng.random() < 0.6:
            b.prev[y, (x + 1) % b.nx] = first_id + j
    return list(range(first_id, first_id + k))


# ------------------------------------------------------------------------------------------------------ a: shapes
A_SHAPES = [(1, 64), (7, 63), (7, 64), (7, 65), (50, 300), (33, 257)]
A_PARENTS = [2, 3, 10]
A_MAXD = [8, 12, 40]  # bucket sizes 2, 3 and 10


def _case_a(si, wrap, ki):
    ny, nx = A_SHAPES[si]
    k = A_PARENTS[ki]
    maxd = A_MAXD[(si + ki) % 3]
    rng = np.random.default_rng(1000 + 100 * si + 10 * ki + int(wrap))
    b = _Builder(f"a-{ny}x{nx}-{'wrap' if wrap else 'flat'}-k{k}", ny, nx, wrap)
    h = min(ny, 5)
    x0 = nx // 3 + 1
    hi = ny if ny <= 7 else h  # the interior child covers every row of a low grid: top cells see the bottom buckets
    b.rect(b.cur, 9, 0, hi, x0, x0 + 16)
    b.rect(b.cur, 5, ny - h, ny, nx - 8, nx + 8)  # across x = nx - 1 / 0, in the (partial) last bucket rows
    b.rect(b.cur, 3, 0, 1, x0 + 18, x0 + 21)  # objects that do not merge
    b.cur[ny - 1, 12] = 21
    b.rect(b.prev, 77, 0, 1, x0 + 3, x0 + 5)  # an object of the previous slice that is nobody's parent
    p5 = _scatter_parents(b, rng, 20, k, ny - h, ny, nx - 9, nx + 9)
    p9 = _scatter_parents(b, rng, 40, k, 0, hi, x0 - 1, x0 + 17)
    b.child(5, p5, maxd)
    b.child(9, p9, maxd)
    b.marks["gs"] = bucket_size(maxd)
    return b.done("a")


# ------------------------------------------------------------------------------------------------------ b: few buckets
B_NY = {1: 7, 2: 15, 3: 25}   # bucket size 10
B_NX = {1: 9, 2: 16, 3: 27}


def _case_b(gy, gx, wrap):
    ny, nx = B_NY[gy], B_NX[gx]
    rng = np.random.default_rng(2000 + 10 * gy + gx + 100 * int(wrap))
    b = _Builder(f"b-{gy}x{gx}-{'wrap' if wrap else 'flat'}", ny, nx, wrap)
    u = rng.random((ny, nx))
    b.cur[u < 0.35] = 5
    b.cur[(u >= 0.35) & (u < 0.6)] = 9
    b.cur[(u >= 0.6) & (u < 0.7)] = 3
    p5 = _scatter_parents(b, rng, 20, 3, 0, ny, 0, nx)
    p9 = _scatter_parents(b, rng, 40, 2, 0, ny, 0, nx)
    b.child(5, p5, 40)
    b.child(9, p9, 40)
    assert bucket_counts(ny, nx, 40) == (gy, gx)
    return b.done("b")


# ------------------------------------------------------------------------------------------------------ c: shared parent
C_SHARED = 30


def _case_c(n_children, wrap):
    ny, nx = 24, 64
    b = _Builder(f"c-{n_children}children-{'wrap' if wrap else 'flat'}", ny, nx, wrap)
    b.rect(b.prev, C_SHARED, 11, 13, 60, 60 + 40)  # the shared parent: a bar across the seam, x = 60 .. 35
    b.rect(b.cur, 5, 6, 12, 62, 62 + 10)           # child 5 above the bar's left end, across the seam
    b.rect(b.cur, 9, 12, 18, 10, 24)               # child 9 below its middle
    b.rect(b.prev, 21, 5, 6, 63, 63 + 6)
    b.rect(b.prev, 41, 18, 19, 12, 20)
    b.rect(b.prev, 42, 14, 16, 25, 27)
    b.rect(b.cur, C_SHARED, 20, 22, 40, 44)        # a non-merging object whose ID equals the shared parent's
    b.rect(b.cur, 21, 0, 1, 30, 33)
    b.child(5, [C_SHARED, 21], 40)                 # bucket size 10, the shared parent first
    b.child(9, [41, 42, C_SHARED], 8)              # bucket size 2, the shared parent last
    if n_children == 3:
        b.rect(b.cur, 13, 4, 11, 26, 34)           # child 13 above the bar's right end
        b.rect(b.prev, 61, 2, 4, 27, 30)
        b.rect(b.prev, 62, 6, 8, 35, 37)
        b.child(13, [61, C_SHARED, 62], 12)        # bucket size 3, the shared parent in the middle
    b.marks["shared_entries"] = [j for j, p in enumerate(b.parents) if p == C_SHARED]
    return b.done("c")


# ------------------------------------------------------------------------------------------------------ d: both rules
def _case_d(wrap):
    ny, nx = 9, 80
    b = _Builder(f"d-{'wrap' if wrap else 'flat'}", ny, nx, wrap)
    b.rect(b.cur, 5, 3, 6, 10, 50)  # the long child
    b.prev[4, 8] = 31               # parent 31 at the near end: the only one with cells within the cap of 3 ...
    b.prev[1, 10] = 31              # ... and with one cell in the 3 x 3 buckets of (3, 13) at sqrt(13), beyond the cap
    b.prev[8, 76] = 32              # parent 32: out of every child cell's reach
    b.prev[8, 77] = 32
    b.rect(b.cur, 3, 7, 9, 40, 44)
    # the nearest-cell rule can only choose parent 31 and takes the whole column x = 10; the centroids are 19 cells to the
    # left of that column and 20 to its right, so that every cell left to the centroid rule (x >= 11) goes to parent 32
    b.child(5, [31, 32], 3, centroids=[(4.0, 71.0 if wrap else -9.0), (4.0, 30.0)])
    b.marks["leftover"] = (3, 13)
    return b.done("d")


# ------------------------------------------------------------------------------------------------------ e: ties and the cap
def _case_e(which):
    if which == "tie":
        b = _Builder("e-tie", 11, 40, True)
        b.cur[5, 10] = 5   # two cells away from both parents: the first listed wins
        b.cur[5, 9] = 5    # nearer to 31
        b.cur[5, 11] = 5   # nearer to 32
        b.prev[5, 8] = 31
        b.prev[5, 12] = 32
        b.child(5, [31, 32], 8)
        b.marks["tie"] = (5, 10)
    elif which == "cap":
        b = _Builder("e-cap", 11, 40, True)
        b.cur[5, 30] = 5   # exactly max_distance = 3 from parent 32: taken
        b.cur[4, 30] = 5   # sqrt(10) from it, in the same buckets: not taken, the centroid rule gives it to 31
        b.cur[5, 33] = 5   # on the parent's cell
        b.prev[5, 33] = 32
        b.prev[9, 2] = 31  # out of everyone's reach
        b.child(5, [31, 32], 3, centroids=[(5.0, 28.0), (5.0, 37.0)])
        b.marks["cap"] = (5, 30)
        b.marks["beyond"] = (4, 30)
    elif which == "half":
        b = _Builder("e-half", 5, 16, True)
        b.cur[2, 0] = 5    # |dx| = 8 = nx / 2 to parent 31 (not wrapped), dx = -9 -> 7 to parent 32 (wrapped)
        b.cur[2, 1] = 5    # 7 to parent 31, 8 = nx / 2 to parent 32
        b.prev[2, 8] = 31
        b.prev[2, 9] = 32
        b.child(5, [31, 32], 40)
        b.marks["half"] = (2, 0)
    else:
        assert which == "roots"
        b = _Builder("e-roots", 5, 11, False)
        b.cur[0, 0] = 5    # 4 + 2^-50 and 4 have the same root 2.0: a tie of the distances, the first centroid wins
        b.cur[4, 10] = 5   # nearer to the second centroid
        b.prev[4, 3] = 31  # no parent cell within the cap of 1: both cells take the centroid rule
        b.prev[2, 6] = 32
        b.child(5, [31, 32], 1, centroids=[(-2.0 ** -25, 2.0), (0.0, 2.0)])
        b.marks["roots"] = (0, 0)
    return b.done("e")


# ------------------------------------------------------------------------------------------------------ f: scan widths
#: total -> (nx, entries of child 5 (max_distance 8, bucket size 2), entries of child 9, max_distance of child 9)
F_LAYOUT = {1: (2, 1, 0, 0), 2: (2, 2, 0, 0), 1023: (682, 3, 0, 0), 1024: (1024, 2, 0, 0), 1025: (788, 2, 3, 40),
            2049: (1366, 3, 0, 0), 3 * 1024 + 1: (1756, 2, 3, 16)}


def _case_f(total):
    nx, ka, kb, maxd_b = F_LAYOUT[total]
    rng = np.random.default_rng(6000 + total)
    b = _Builder(f"f-{total}", 2, nx, True)
    b.cur[0, :] = 5
    if kb:
        b.cur[1, :] = 9

    def place(pid, gs, row):
        ngx = (nx + gs - 1) // gs
        want = [0, ngx - 1] + rng.integers(0, ngx, 3).tolist()
        for bx in dict.fromkeys(want):
            free = [(y, x) for y in (row, 1 - row) for x in range(bx * gs, min(nx, bx * gs + gs)) if b.prev[y, x] == 0]
            assert free, (total, pid, bx)
            b.prev[free[0]] = pid

    for j in range(ka):
        place(20 + j, 2, 0)
    for j in range(kb):
        place(40 + j, bucket_size(maxd_b), 1)
    b.child(5, list(range(20, 20 + ka)), 8, keep_id=ka > 1)  # the only label of f-1 is a fresh one: the write shows
    if kb:
        b.child(9, list(range(40, 40 + kb)), maxd_b)
    case = b.done("f")
    assert total_buckets(case) == total, (total, total_buckets(case))
    return case


# ------------------------------------------------------------------------------------------------------ g: grid stride
def _case_g():
    ny, nx = 1025, 2048
    rng = np.random.default_rng(7000)
    b = _Builder("g-1025x2048", ny, nx, True)
    b.rect(b.cur, 5, 0, 3, 100, 140)
    b.rect(b.cur, 9, 1022, 1025, nx - 8, nx + 8)  # row 1024 starts at flat index 2 097 152
    b.rect(b.cur, 3, 1024, 1025, 500, 520)
    p5 = _scatter_parents(b, rng, 20, 3, 0, 3, 98, 142)
    p9 = _scatter_parents(b, rng, 40, 4, 1022, 1025, nx - 10, nx + 10)
    b.prev[1024, nx - 3] = p9[-1]  # a parent cell that only the second round of the bucket kernels' loop reaches
    b.child(5, p5, 40)
    b.child(9, p9, 40)
    assert ny * nx > LAUNCH_CELLS
    return b.done("g")


# ------------------------------------------------------------------------------------------------------ the registry
def _registry():
    reg = {}
    for si in range(len(A_SHAPES)):
        for wrap in (True, False):
            for ki in range(len(A_PARENTS)):
                ny, nx = A_SHAPES[si]
                reg[f"a-{ny}x{nx}-{'wrap' if wrap else 'flat'}-k{A_PARENTS[ki]}"] = ("a", functools.partial(_case_a, si, wrap, ki))
    for gy in (1, 2, 3):
        for gx in (1, 2, 3):
            for wrap in (True, False):
                reg[f"b-{gy}x{gx}-{'wrap' if wrap else 'flat'}"] = ("b", functools.partial(_case_b, gy, gx, wrap))
    for n in (2, 3):
        for wrap in (True, False):
            reg[f"c-{n}children-{'wrap' if wrap else 'flat'}"] = ("c", functools.partial(_case_c, n, wrap))
    for wrap in (True, False):
        reg[f"d-{'wrap' if wrap else 'flat'}"] = ("d", functools.partial(_case_d, wrap))
    for which in ("tie", "cap", "half", "roots"):
        reg[f"e-{which}"] = ("e", functools.partial(_case_e, which))
    for total in F_LAYOUT:
        reg[f"f-{total}"] = ("f", functools.partial(_case_f, total))
    reg["g-1025x2048"] = ("g", _case_g)
    return reg


_REG = _registry()
NAMES = list(_REG)
FAMILIES = {f: [n for n in NAMES if _REG[n][0] == f] for f in "abcdefg"}


@functools.lru_cache(maxsize=None)
def get(name):
    """The case ``name``; its arrays are shared between the tests and must not be written."""
    case = _REG[name][1]()
    assert case.name == name and case.family == _REG[name][0], (name, case.name)
    for a in (case.cur, case.prev, case.child_keys, case.off, case.parents, case.pcy, case.pcx, case.lab, case.maxd):
        a.setflags(write=False)
    return case


@functools.lru_cache(maxsize=None)
def expected(name, nn):
    """``(slice, fallback)``: the slice after the partition by the oracle, one child at a time, and with ``nn`` the mask
    of the child cells that no parent cell reaches and the centroid rule decides."""
    c = get(name)
    out = c.cur.copy()
    fallback = np.zeros(c.cur.shape, bool)
    for k, key in enumerate(c.child_keys.tolist()):
        ys, xs = np.nonzero(c.cur == key)
        sl = slice(int(c.off[k]), int(c.off[k + 1]))
        pc = np.stack([c.pcy[sl], c.pcx[sl]], axis=1)
        if nn:
            cells = [np.nonzero(c.prev == p) for p in c.parents[sl].tolist()]
            a = mo.partition_nn(ys, xs, cells, pc, c.ny, c.nx, int(c.maxd[sl][0]), c.wrap)
            # the fallback cells, from the oracle alone: with one more parent that has no cells and the only centroid
            # near the child, the oracle gives that parent exactly the cells it leaves to the centroid rule
            far = np.full_like(pc, 1e150)
            marker = mo.partition_nn(ys, xs, cells + [(np.zeros(0, np.int64), np.zeros(0, np.int64))],
                                     np.concatenate([far, [[ys.mean(), xs.mean()]]]), c.ny, c.nx, int(c.maxd[sl][0]), c.wrap)
            fallback[ys, xs] = marker == len(cells)
        else:
            a = mo.partition_centroid(ys, xs, pc, c.nx, c.wrap)
        out[ys, xs] = c.lab[sl][a]
    out.setflags(write=False)
    fallback.setflags(write=False)
    return out, fallback


def check_coverage(name):
    """The conditions a case exists for, from the oracle's results alone; a case that misses one is broken, not skipped."""
    c = get(name)
    cen, _ = expected(name, False)
    near, fallback = expected(name, True)
    child = np.isin(c.cur, c.child_keys)
    for what, out in (("centroid", cen), ("nearest cell", near)):
        assert np.array_equal(out[~child], c.cur[~child]), (name, what)
        for k, key in enumerate(c.child_keys.tolist()):
            got = np.unique(out[c.cur == key])
            assert set(got.tolist()) <= set(c.lab[c.off[k]:c.off[k + 1]].tolist()), (name, what, key)
            if c.off[k + 1] - c.off[k] > 1:
                assert got.size >= 2, f"{name}: child {key} is not split by the {what} rule"
            else:  # one bucket in all means one entry and one label (f-1): the label is fresh, so the write shows
                assert name == "f-1" and got.size == 1 and got[0] != key, (name, what, key)
    if c.family == "c":
        shared = [(np.searchsorted(c.off, j, side="right") - 1, j) for j in c.marks["shared_entries"]]
        assert len({int(c.gs_of(j)) for _, j in shared}) == len(shared), f"{name}: the shared parent's bucket sizes repeat"
        for what, out in (("centroid", cen), ("nearest cell", near)):
            won = sum(bool((out[c.cur == c.child_keys[k]] == c.lab[j]).any()) for k, j in shared)
            assert won >= 2, f"{name}: the shared parent wins cells in {won} children by the {what} rule"
        assert (c.cur == C_SHARED).any() and np.array_equal(near[c.cur == C_SHARED], c.cur[c.cur == C_SHARED])
    if c.family == "d":
        m = c.cur == 5
        assert (fallback & m).sum() > 0 and (~fallback & m).sum() > 0, name
        assert (near[m & ~fallback] == c.lab[0]).all() and (near[m & fallback] == c.lab[1]).all(), name
        assert fallback[c.marks["leftover"]]
    if c.family == "e":
        def d_to(cell, pid):
            ys, xs = np.nonzero(c.prev == pid)
            dx = xs - cell[1]
            dx = np.where(np.abs(dx) > c.nx / 2, c.nx - np.abs(dx), dx) if c.wrap else dx
            return np.sqrt(((ys - cell[0]) ** 2 + dx ** 2).astype(np.float64)).min()
        if "tie" in c.marks:
            cell = c.marks["tie"]
            assert c.cur[cell] == 5 and d_to(cell, 31) == d_to(cell, 32) <= c.maxd[0]
            assert near[cell] == c.lab[0] and not fallback[cell]
        if "cap" in c.marks:
            cell, far = c.marks["cap"], c.marks["beyond"]
            assert c.cur[cell] == 5 and d_to(cell, 32) == c.maxd[0] and d_to(cell, 31) > c.maxd[0]
            assert near[cell] == c.lab[1] and not fallback[cell]
            assert c.cur[far] == 5 and d_to(far, 32) == np.sqrt(float(c.maxd[0]) ** 2 + 1) and fallback[far]
            assert near[far] == c.lab[0]
        if "half" in c.marks:
            cell = c.marks["half"]
            assert c.wrap and c.nx % 2 == 0 and c.cur[cell] == 5
            assert abs(int(np.nonzero(c.prev == 31)[1][0]) - cell[1]) == c.nx // 2
            assert near[cell] == c.lab[1] and cen[cell] == c.lab[1]  # the wrapped 7 beats the unwrapped 8
        if "roots" in c.marks:
            y, x = c.marks["roots"]
            sq = (y - c.pcy) ** 2 + (x - c.pcx) ** 2
            assert sq[0] > sq[1] and np.sqrt(sq[0]) == np.sqrt(sq[1])
            assert fallback[y, x] and near[y, x] == c.lab[0] and cen[y, x] == c.lab[0]
    if c.family == "f":
        assert c.ny == 2 and total_buckets(c) == int(name.split("-")[1]), name
    if c.family == "g":
        flat = np.arange(c.ny * c.nx).reshape(c.ny, c.nx)
        for out in (cen, near):
            assert ((out != c.cur) & (flat >= LAUNCH_CELLS)).any(), name
        assert ((c.prev > 0) & (flat >= LAUNCH_CELLS)).any(), name


# ------------------------------------------------------------------------------------------------------ refused tables
def bad_tables(c):
    """``what -> keyword changes`` of a two-child case's partition arguments, each of which the engine has to refuse."""
    n = len(c.lab)
    keys, off = c.child_keys, c.off
    return {
        "no child": dict(child_keys=keys[:0], off=off[:1]),
        "children descending": dict(child_keys=keys[::-1].copy()),
        "a child twice": dict(child_keys=np.array([keys[0], keys[0]], np.int32)),
        "off does not start at 0": dict(off=off + 1),
        "off ends before len(lab)": dict(off=np.array([0, off[1], n - 1], np.int32)),
        "off ends after len(lab)": dict(off=np.array([0, off[1], n + 1], np.int32)),
        "off gives a child no entry": dict(off=np.array([0, 0, n], np.int32)),
        "off gives the last child no entry": dict(off=np.array([0, n, n], np.int32)),
        "off descends": dict(off=np.array([0, n + 2, n], np.int32)),
        "off too short": dict(off=off[:-1]),
        "off too long": dict(off=np.append(off, n).astype(np.int32)),
        "pcy short": dict(pcy=c.pcy[:-1]),
        "pcx long": dict(pcx=np.append(c.pcx, 1.0)),
        "lab short": dict(lab=c.lab[:-1]),
        "lab of floats": dict(lab=c.lab.astype(np.float64)),
        "ny too large": dict(ny=c.ny + 1),
        "nx too small": dict(nx=c.nx - 1),
        "ny zero": dict(ny=0),
    }


def bad_nn_tables(c):
    big = c.maxd.astype(np.int64)
    big[-1] = 2 ** 31
    zero, neg = c.maxd.copy(), c.maxd.copy()
    zero[0], neg[1] = 0, -8
    return {
        "parents short": dict(parents=c.parents[:-1]),
        "parents long": dict(parents=np.append(c.parents, 1).astype(np.int32)),
        "maxd short": dict(maxd=c.maxd[:-1]),
        "maxd zero": dict(maxd=zero),
        "maxd negative": dict(maxd=neg),
        "maxd above INT32_MAX": dict(maxd=big),
        "maxd of floats": dict(maxd=c.maxd.astype(np.float64)),
    }


def bad_relabel_tables():
    """``what -> (vals, keys)`` that ``HotPath.relabel`` has to refuse."""
    keys, vals = np.array([3, 7, 19], np.int32), np.array([1, 2, 3], np.int32)
    return {"keys descending": (vals, keys[::-1].copy()), "a key twice": (vals, np.array([3, 7, 7], np.int32)),
            "more keys than values": (vals[:2], keys), "more values than keys": (vals, keys[:2]),
            "keys without values": (vals[:0], keys), "a key above INT32_MAX": (vals, np.array([3, 7, 2 ** 31], np.int64)),
            "values of floats": (vals.astype(np.float32), keys), "a two-dimensional table": (vals.reshape(1, 3), None)}


# ------------------------------------------------------------------------------------------------------ h: relabel
def _relabel_expected(ids, vals, keys):
    ids64 = ids.astype(np.int64)
    if keys is None:
        hit = (ids64 > 0) & (ids64 < len(vals))
        return np.where(hit, vals[np.where(hit, ids64, 0)], ids).astype(np.int32)
    pos = np.minimum(np.searchsorted(keys, ids), len(keys) - 1)
    hit = (ids64 > 0) & (keys[pos] == ids)
    return np.where(hit, vals[pos], ids).astype(np.int32)


@functools.lru_cache(maxsize=None)
def relabel_cases():
    """``name -> (ids, vals, keys or None, expected)``, read-only arrays."""
    rng = np.random.default_rng(8000)
    out = {}
    edge = np.array([0, -1, -50, -I32_MAX - 1, 1, 48, 49, 50, 51, I32_MAX, I32_MAX - 1], np.int32)

    def ids_of(n, pool, mapped):
        if n == 1:
            return np.array([mapped], np.int32)
        x = rng.choice(pool, size=n).astype(np.int32)
        m = min(n - 1, edge.size)
        x[:m] = edge[:m]
        x[m] = mapped
        return x[rng.permutation(n)]

    dense = rng.integers(1, 1000, 50).astype(np.int32)  # n_keys = 50: 49 is mapped, 50 and 51 are not
    dense_pool = np.arange(-3, 60)
    for n in (1, 255, 256, 257, 1025 * 2048):
        out[f"h-dense-n{n}"] = (ids_of(n, dense_pool, 49), dense, None)
    out["h-dense-only-the-edges"] = (np.array([49, 50, 51, 49], np.int32), dense, None)
    out["h-dense-one-entry"] = (np.array([1, 0, 2, -1], np.int32), np.array([9], np.int32), None)  # vals[0] is never read
    many = np.unique(rng.integers(2, I32_MAX, 110_000))
    many = np.sort(rng.choice(many, size=100_000 - 2, replace=False))
    many = np.concatenate([[1], many, [I32_MAX]]).astype(np.int32)  # the smallest and the largest ID are keys
    assert many.size == 100_000 and np.all(np.diff(many.astype(np.int64)) > 0)
    many_vals = rng.integers(1, I32_MAX, many.size).astype(np.int32)
    many_pool = np.concatenate([many[::7], many[::7].astype(np.int64) + 1, many[::7].astype(np.int64) - 1, np.arange(-5, 5)])
    many_pool = np.clip(many_pool, -I32_MAX - 1, I32_MAX)
    for n in (1, 255, 256, 257, 1025 * 2048):
        out[f"h-sorted-100000-n{n}"] = (ids_of(n, many_pool, I32_MAX), many_vals, many)
    for key in (7, 1, I32_MAX):
        pool = np.clip(np.array([key - 1, key, int(key) + 1, 0, -key], np.int64), -I32_MAX - 1, I32_MAX)
        out[f"h-sorted-one-key-{key}"] = (ids_of(257, pool, key), np.array([123456], np.int32), np.array([key], np.int32))
    res = {}
    for name, (ids, vals, keys) in out.items():
        exp = _relabel_expected(ids, vals, keys)
        for a in (ids, vals, exp) + (() if keys is None else (keys,)):
            a.setflags(write=False)
        res[name] = (ids, vals, keys, exp)
    return res


RELABEL_NAMES = ([f"h-dense-n{n}" for n in (1, 255, 256, 257, 1025 * 2048)] + ["h-dense-only-the-edges", "h-dense-one-entry"]
                 + [f"h-sorted-100000-n{n}" for n in (1, 255, 256, 257, 1025 * 2048)]
                 + [f"h-sorted-one-key-{k}" for k in (7, 1, I32_MAX)])
