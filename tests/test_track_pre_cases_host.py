"""Host checks of the pre-processing cases (tests/track_pre_cases.py): no device.

* The restated launch geometry is the source's (the lines it restates are pinned), and every case lands on the edge of
  the launch it is named for: the second trip of k_morph_pack's word loop, its grid-stride, a last word of 64 cells and of
  one, half-widths up to 63, grids far narrower than the padding, several time blocks of k_time_closing16, the scalar
  kernel, windows wider than the series.
* The second references equal the oracle: the distance form of the fill on every fill case with R <= 31 and on one image
  at R = 63, the run-length rule of the time closing on every closing case.  A disagreement on the device cannot be an
  oracle quirk.
* No case is trivial: the expected results add cells and remove cells, the last words of the padded rows carry set bits,
  gaps are closed and gaps are left open.
"""
import os
import re
import sys

import numpy as np
import pytest

from oracle import marex_oracle as orc

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import track_pre_cases as tc  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FILL = {c.name: c for c in tc.fill_cases()}


def _geom(c):
    return tc.fill_geometry(c.T, c.ny, c.nx, c.R)


# ------------------------------------------------------------------------------------------------------------------------
# the restated geometry is the source's
# ------------------------------------------------------------------------------------------------------------------------
def test_geometry_is_the_one_in_the_source():
    """fill_geometry, closing_geometry and the limits restate these lines; when they change, the restatement (and the
    edges the cases are named for) must be looked at again."""
    src = re.sub(r"\s+", " ", open(os.path.join(ROOT, "marex_amd", "csrc", "marex_morphology.hip")).read())
    for line in (
        "const int Hp = ny + 4 * R, nxp = nx + 4 * R, Wp = (nxp + 63) / 64;",
        "for (long r = blockIdx.x; r < rows; r += gridDim.x) {",
        "for (int w0 = wave; w0 < Wp; w0 += 4 * 8) {",
        "const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;",
        "if (lane == 0 && w0 + 4 * u < Wp) packed[(size_t)r * Wp + w0 + 4 * u] = word;",
        "dim3((unsigned)((long)T * Hp < 1048576 ? (long)T * Hp : 1048576)), dim3(256)",
        "const int last_bits = nxp - 64 * (Wp - 1);",
        "if (w == Wp - 1 && last_bits < 64) acc &= (1ull << last_bits) - 1ull;",
        "while ((w + 1) * (w + 1) + dy * dy < R * R + 1) ++w;",
        'if (R < 0 || R > 63) return fail(ctx, -4, "marex_fill_holes_u8: R_fill must be in 0..63");',
        'if (R < 0 || R > 1024) return fail(ctx, -4, "marex_fill_holes_mesh_u8: R_fill must be in 0..1024");',
        "const int wide = (nx & 7) == 0 && (((uintptr_t)mask | (uintptr_t)out) & 7) == 0;",
        "#define TC_TBLOCK 32",
        "const long t0 = (long)blockIdx.y * TC_TBLOCK;",
        "if ((C & 15) == 0 && (((uintptr_t)data | (uintptr_t)out) & 15) == 0) {",
        "dim3 grid((unsigned)((C / 16 + 255) / 256), (unsigned)((T + TC_TBLOCK - 1) / TC_TBLOCK));",
        "hipLaunchKernelGGL(k_time_closing16, grid, dim3(256), 0, ctx->stream, data, (long)T, (long)C, T_fill / 2, out);",
    ):
        assert line in src, line
    assert (tc.R_MAX, tc.MESH_R_MAX, tc.PACK_GRID_CAP, tc.PACK_W0_STRIDE, tc.TC_TBLOCK) == (63, 1024, 1048576, 32, 32)
    # the restatement on shapes worked out by hand
    assert tc.fill_geometry(2, 3, 60, 1) == (7, 64, 1, 64, 14, (1, 0, 0, 0))
    assert tc.fill_geometry(5, 37, 70, 12) == (85, 118, 2, 54, 425, (1, 1, 0, 0))
    assert tc.closing_geometry(65, 4112, 4) == ("wide", 3, 2) and tc.closing_geometry(65, 4112, 4, aligned=False) == ("scalar", 1, 2)
    assert tc.closing_geometry(32, 17, 18) == ("scalar", 1, 9)


# ------------------------------------------------------------------------------------------------------------------------
# every fill case reaches its edge
# ------------------------------------------------------------------------------------------------------------------------
def test_fill_cases_are_the_listed_ones():
    kinds = {}
    for c in tc.fill_cases():
        kinds.setdefault(c.kind, []).append(c)
        assert 0 < c.R <= tc.R_MAX
    assert len(FILL) == len(tc.fill_cases())  # the names are ids
    assert {(c.nx + 4 * c.R, c.R, c.regional) for c in kinds["word"] if c.nx != 2300} == {
        (nxp, R, reg) for nxp in (64, 65, 128, 2048, 2049) for R in (1, 2) for reg in (False, True)}
    assert {(c.nx, c.R, c.regional) for c in kinds["word"] if c.nx == 2300} == {(2300, 1, False), (2300, 1, True)}
    assert all((c.T, c.ny) == (2, 3) for c in kinds["word"] + kinds["tail"])
    assert {(c.R, c.regional) for c in kinds["radius"]} == {(R, reg) for R in (12, 31, 62, 63) for reg in (False, True)}
    assert all(c.T == 2 and (c.ny, c.nx) == (6 * c.R + 11, 8 * c.R + 13) for c in kinds["radius"])
    assert {(c.ny, c.nx, c.R, c.regional) for c in kinds["narrow"]} == {
        (ny, nx, R, reg) for (ny, nx) in ((1, 1), (1, 7), (5, 3), (2, 64)) for R in (5, 31) for reg in (False, True)}
    assert [(c.T, c.ny, c.nx, c.R) for c in kinds["rows"]] == [(116509, 5, 8, 1)]


def test_word_cases_reach_the_word_and_trip_edges():
    seen = set()
    for c in tc.fill_cases():
        if c.kind != "word":
            continue
        Hp, nxp, Wp, last_bits, rows, trips = _geom(c)
        want = {64: (1, 64), 65: (2, 1), 128: (2, 64), 2048: (32, 64), 2049: (33, 1), 2304: (36, 64)}[nxp]
        assert (Wp, last_bits) == want, c.name
        assert trips == {32: (1, 1, 1, 1), 33: (2, 1, 1, 1), 36: (2, 2, 2, 2)}.get(Wp, trips), c.name
        assert max(trips) == (2 if Wp > 32 else 1)
        seen.add((Wp, last_bits, c.R, c.regional))
    for R in (1, 2):
        for reg in (False, True):
            assert {(32, 64, R, reg), (33, 1, R, reg), (1, 64, R, reg), (2, 1, R, reg)} <= seen
    assert {(36, 64, 1, False), (36, 64, 1, True)} <= seen
    # the tail-band cases: one cell and 36 cells in the last word
    assert {(_geom(c)[3], c.R, c.regional) for c in tc.fill_cases() if c.kind == "tail"} == {
        (b, R, reg) for b in (1, 36) for R in (1, 2) for reg in (False, True)}


@pytest.mark.parametrize("name", [c.name for c in tc.fill_cases() if c.kind in ("word", "tail")])
def test_word_cases_set_bits_in_the_last_words(name):
    """Input and result have set cells in the last word of a padded row that holds any: in the padded input that is word
    Wp - 1; the result is trimmed by 2R, its last cells lie in the word of padded column nx + 2R - 1.  On the wide rows
    the words past index 31 -- those of the pack loop's second trip -- are set in both as well."""
    c = FILL[name]
    x, mask = tc.fill_inputs(name)
    Hp, nxp, Wp, last_bits, rows, trips = _geom(c)
    p0, p = tc.fill_holes_distance(x, mask, c.R, c.regional, padded=True)
    assert p0.shape == (c.T, Hp, nxp)
    assert p0[:, :, 64 * (Wp - 1):].any(axis=(1, 2)).all()
    exp = tc.fill_holes_distance(x, mask, c.R, c.regional)
    w_last = (c.nx + 2 * c.R - 1) // 64                      # word of the last valid cell
    lo = max(64 * w_last - 2 * c.R, 0)                       # its first cell, in unpadded columns
    assert exp[:, :, lo:].any(axis=(1, 2)).all()
    assert not np.array_equal(exp, x & mask[None])
    if Wp > 32:
        assert p0[:, 2 * c.R:-2 * c.R, 64 * 32:].any(axis=(1, 2)).all()
        assert w_last >= 31 and exp[:, :, 64 * 32 - 2 * c.R:].any(axis=(1, 2)).all() == (w_last >= 32)
    if c.kind == "tail":  # the band is there and the opening removes it
        assert x[:, :, -c.R:].all() and not exp[:, :, -c.R:].any()


def test_row_stride_case_passes_the_grid_cap():
    c = FILL["rows-R1-periodic"]
    Hp, nxp, Wp, last_bits, rows, trips = _geom(c)
    assert rows == 1048581 > tc.PACK_GRID_CAP == 2 ** 20
    # the rows of the second trip of the grid-stride belong to the last timestep, the rows just below the cap to the last two
    assert (tc.PACK_GRID_CAP // Hp, (rows - 1) // Hp) == (c.T - 1, c.T - 1) and (tc.PACK_GRID_CAP - Hp) // Hp == c.T - 2
    x, mask = tc.fill_inputs(c.name)
    exp = orc.fill_holes(x, mask, c.R, c.regional)
    for t in (-2, -1):
        assert x[t].any() and exp[t].any() and not exp[t].all()
        for u in (0, 1):
            assert not np.array_equal(x[t], x[u]) and not np.array_equal(exp[t], exp[u])
    assert not np.array_equal(exp[-1], exp[-2])
    assert 2 * (c.T * Hp * Wp) * 8 < 20e6  # the device scratch stays small


def test_radius_cases_reach_the_half_widths():
    def hw(R):  # the host loop of marex_fill_holes_u8
        out = []
        for dy in range(R + 1):
            w = 0
            while (w + 1) * (w + 1) + dy * dy < R * R + 1:
                w += 1
            out.append(w)
        return out

    # half-widths up to 63: shifts by 64 - k down to 1; the widest rows of the disk reach the neighbour words only
    assert hw(63)[0] == 63 and hw(63)[63] == 0 and hw(62)[0] == 62 and min(hw(63)[:32]) > 48 and hw(1) == [1, 0]
    for c in tc.fill_cases():
        if c.kind == "radius":
            Hp, nxp, Wp, last_bits, rows, trips = _geom(c)
            assert Wp >= 3 and c.R in tc.STRUCTURED_R  # a word has both neighbours: hits from either side
    assert tc.STRUCTURED_R[-1] == tc.R_MAX


def test_narrow_cases_wrap_many_times():
    for c in tc.fill_cases():
        if c.kind == "narrow":
            assert (2 * c.R) // min(c.ny, c.nx) >= 3  # the padding of 2R holds the grid at least three times over
            x, mask = tc.fill_inputs(c.name)
            assert not x[0].any() and x[1].all() and all(0 < x[t].mean() < 1 or x[t].size == 1 for t in (2, 3, 4))


# ------------------------------------------------------------------------------------------------------------------------
# the distance form equals the oracle
# ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", [c.name for c in tc.fill_cases() if c.R <= 31])
def test_distance_form_equals_the_oracle(name):
    c = FILL[name]
    x, mask = tc.fill_inputs(name)
    assert np.array_equal(tc.fill_holes_distance(x, mask, c.R, c.regional), orc.fill_holes(x, mask, c.R, c.regional))


def test_distance_form_equals_the_oracle_at_the_largest_radius():
    """One 8 x 8 image, periodic: the padded image is 260 x 260 and the oracle's four passes with a 127 x 127 disk take
    most of this file's run time."""
    rng = np.random.default_rng(63)
    x = rng.random((1, 8, 8)) < 0.4
    mask = rng.random((8, 8)) < 0.9
    exp = orc.fill_holes(x, mask, 63, False)
    assert np.array_equal(tc.fill_holes_distance(x, mask, 63, False), exp)


def test_distance_form_small_radii_and_the_zero_radius():
    rng = np.random.default_rng(5)
    x = rng.random((3, 17, 23)) < 0.35
    mask = rng.random((17, 23)) < 0.8
    for R in (0, 1, 2, 3, 5, 8):
        for regional in (False, True):
            assert np.array_equal(tc.fill_holes_distance(x, mask, R, regional), orc.fill_holes(x, mask, R, regional)), (R, regional)


# ------------------------------------------------------------------------------------------------------------------------
# no fill case is trivial
# ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", [c.name for c in tc.fill_cases() if c.kind == "radius"])
def test_structured_cases_are_not_trivial(name):
    c = FILL[name]
    x, mask = tc.fill_inputs(name)
    exp = tc.fill_holes_distance(x, mask, c.R, c.regional)
    share = exp[:, mask].mean()
    assert 0.05 <= share <= 0.6, share
    assert (exp & ~x).sum() >= 10 and (x & ~exp).sum() >= 10
    assert not mask.all() and (x[:, :, 0].any(axis=1)).all()  # land; objects on the seam / the border
    for t in range(c.T):  # 60 pinholes and 4 specks a step would not change these counts by more
        assert abs(int(x[t].sum()) - int(x[0].sum())) < 0.2 * x[0].sum()
    assert not np.array_equal(x[0], x[1])


# ------------------------------------------------------------------------------------------------------------------------
# time closing
# ------------------------------------------------------------------------------------------------------------------------
def test_closing_cases_reach_both_kernels_and_several_time_blocks():
    assert set(tc.CLOSING_T) == {1, 31, 32, 33, 64, 65, 97}
    assert set(tc.CLOSING_C_WIDE) == {16, 4096, 4112} and set(tc.CLOSING_C_SCALAR) == {1, 15, 17, 4097}
    for T in tc.CLOSING_T:
        assert set(tc.closing_t_fills(T)) == {0, 2, 4, 16, 18, 2 * T}
    blocks = set()
    for (T, tf) in tc.closing_cases():
        for C in tc.CLOSING_C_WIDE:
            k, nb, c = tc.closing_geometry(T, C, tf)
            assert k == "wide" and nb == -(-T // 32) and c == tf // 2
            blocks.add(nb)
            assert tc.closing_geometry(T, C, tf, aligned=False)[0] == "scalar"  # the byte-offset view of the same field
        for C in tc.CLOSING_C_SCALAR:
            assert tc.closing_geometry(T, C, tf)[0] == "scalar"
    assert blocks == {1, 2, 3, 4}
    assert {T: -(-T // 32) for T in tc.CLOSING_T} == {1: 1, 31: 1, 32: 1, 33: 2, 64: 2, 65: 3, 97: 4}
    # 4 112 cells: 257 threads of 16 cells, i.e. a second workgroup with one active lane
    assert 4112 // 16 == 257 and 4096 // 16 == 256
    # windows wider than the series: c = T for T_fill = 2T (every step sees the whole series), c > T where T = 1; c > 8
    cs = {(T, tf // 2) for (T, tf) in tc.closing_cases()}
    assert all((T, T) in cs for T in tc.CLOSING_T)
    assert any(c > T for (T, c) in cs) and any(c > 8 and c < T for (T, c) in cs) and any(c > T and c > 8 for (T, c) in cs)


@pytest.mark.parametrize("T,T_fill", tc.closing_cases())
def test_run_length_rule_equals_the_oracle(T, T_fill):
    """On the distinct columns of the case (a column's closing depends on the column alone; every field of the case is
    made of these columns, asserted here for every width)."""
    base, names = tc.closing_columns(T, T_fill)
    n = base.shape[1]
    exp = orc.fill_time_gaps(base.reshape(T, 1, n), np.ones((1, n), dtype=bool), 0, T_fill).reshape(T, n)
    got = tc.time_closing_runs(base, T_fill)
    assert np.array_equal(got, exp)
    wide = tc.closing_field(T, tc.CLOSING_C_MAX, T_fill)
    cols = {base[:, j].tobytes() for j in range(n)}
    assert {wide[:, j].tobytes() for j in range(wide.shape[1])} == cols
    assert np.array_equal(wide[:, :n], base)
    for C in tc.CLOSING_C_WIDE + tc.CLOSING_C_SCALAR:
        f = tc.closing_field(T, C, T_fill)
        assert f.shape == (T, C) and f.flags.c_contiguous and np.array_equal(f, wide[:, :C])
        assert np.array_equal(tc.time_closing_runs(f, T_fill), tc.time_closing_runs(wide, T_fill)[:, :C])
    # nothing before the first or after the last True step of a cell; nothing but False steps change
    first = np.where(base.any(axis=0), base.argmax(axis=0), T)
    last = np.where(base.any(axis=0), T - 1 - base[::-1].argmax(axis=0), -1)
    t = np.arange(T)[:, None]
    assert not got[(t < first[None]) | (t > last[None])].any() and (got | ~base).all() and got[base].all()


@pytest.mark.parametrize("T,T_fill", tc.closing_cases())
def test_closing_cases_close_gaps_and_leave_gaps_open(T, T_fill):
    base, names = tc.closing_columns(T, T_fill)
    exp = tc.time_closing_runs(base, T_fill)
    closed = (exp & ~base).any(axis=0)
    still_open = (~exp).any(axis=0)
    col = {k: j for j, k in enumerate(names)}
    assert not exp[:, col["all_false"]].any() and exp[:, col["all_true"]].all()
    # what can close at all: a gap of 1..T_fill steps between two True steps needs T >= 3 and T_fill >= 1
    can_close = T >= 3 and T_fill >= 1
    for C in tc.CLOSING_C_WIDE + tc.CLOSING_C_SCALAR:
        present = np.zeros(len(names), dtype=bool)
        present[tc._closing_pick(len(names))[:C]] = True
        if C >= 15:
            assert (closed & present).any() == can_close, C
            if T >= 2:
                assert (still_open & present & base.any(axis=0)).any(), C   # open in a column that is not all False
    # the single column of C = 1
    if names[0] == "pair":        # one gap closed (T_fill > 0), one left open
        assert closed[0] == (T_fill > 0) and still_open[0] and (~exp[:, 0]).sum() == T_fill + 1
    elif names[0] == "ends_only":  # no room for the pair: the window is at least as wide as half the series
        assert closed[0] == (T - 2 <= T_fill) and T < 2 * T_fill + 4
    else:
        assert T <= 2
    if "ends_only" in col:
        assert exp[:, col["ends_only"]].all() == (T - 2 <= T_fill) and exp[:, col["first_only"]].sum() == 1
    if T_fill == 0:
        assert np.array_equal(exp, base)
    # the hand-built gaps: T_fill - 1 and T_fill close, T_fill + 1 stays, unless the gap touches an end of the series
    for j, k in enumerate(names):
        if k.startswith("gap"):
            g, place = k[3:].split("@")
            a, b = tc._gap(T, place, int(g))
            assert 0 <= a < b <= T and b - a == int(g) and not base[a:b, j].any() and base[:, j].sum() == T - int(g)
            inner = a > 0 and b < T
            assert exp[a:b, j].all() == (inner and int(g) <= T_fill), k
            assert exp[a:b, j].any() == (inner and int(g) <= T_fill), k
    # two time blocks of the wide kernel: the gaps at 31|32 and 63|64 lie on both sides of the block edge
    for edge in (32, 64):
        for g in (T_fill - 1, T_fill, T_fill + 1):
            ab = tc._gap(T, f"{edge - 1}|{edge}", g) if g >= 2 else None
            if ab is not None:
                assert ab[0] < edge < ab[1] and f"gap{g}@{edge - 1}|{edge}" in col
    if T in (33, 64, 65, 97) and T_fill in (2, 4):
        assert any(k.endswith("@31|32") for k in names) and (T <= 64 or any(k.endswith("@63|64") for k in names))


def test_chained_case():
    c = tc.CHAINED
    x, mask = tc.chained_field()
    assert x.shape == (65, 24, 32) and (c.R_fill, c.T_fill) == (4, 4)
    assert tc.closing_geometry(c.T, c.ny * c.nx, c.T_fill) == ("wide", 3, 2)
    closed = tc.time_closing_runs(x.reshape(c.T, -1), c.T_fill).reshape(x.shape)
    exp = orc.fill_time_gaps(x, mask, c.R_fill, c.T_fill)
    assert np.array_equal(tc.fill_holes_distance(closed, mask, c.R_fill // 2), exp)
    assert (closed & ~x).sum() > 100 and (exp & ~closed).sum() > 10 and (closed & ~exp).sum() > 10
    assert (~x.any(axis=(1, 2))).sum() >= 5  # whole steps missing


# ------------------------------------------------------------------------------------------------------------------------
# mesh
# ------------------------------------------------------------------------------------------------------------------------
def test_mesh_ring_is_what_it_claims():
    x, mask, nbr = tc.mesh_ring()
    C = tc.MESH_C
    assert nbr.shape == (3, C) and nbr.dtype == np.int32 and nbr.min() == -1 and nbr.max() < C
    i = np.arange(C)
    assert (nbr == i[None]).sum() == 3                                    # cells that list themselves
    listed = {(int(a), int(b)) for k in range(3) for a, b in zip(i, nbr[k]) if b >= 0 and a != b}
    assert sum((b, a) not in listed for (a, b) in listed) >= 8             # links listed from one end only
    assert (nbr[:, 240] == -1).all() and any(b == 240 for (_, b) in listed)
    assert x.shape == (5, C) and (~mask).sum() == 31 and not x[:, ~mask].any() and x.any(axis=1).all()
    assert tc.MESH_R == (0, 1, 40, 200, 1024)
    # the sweeps stop changing anything between R = 40 and R = 200: the larger radii lie beyond the mesh's diameter
    m = orc._mesh_dilation_matrix(nbr).astype(np.int32)
    v = np.eye(C, dtype=np.int32)
    steps = 0
    while True:
        w = (m @ v > 0).astype(np.int32)
        if np.array_equal(w, v):
            break
        v, steps = w, steps + 1
    assert 40 < steps < 200, steps
    outs = [orc.fill_holes_mesh(x, mask, nbr, R) for R in tc.MESH_R]
    assert not np.array_equal(outs[0], outs[1]) and not np.array_equal(outs[1], outs[2]) and np.array_equal(outs[3], outs[4])
    for o in outs:  # never one value throughout: an output left unwritten or written whole cannot pass
        assert 0 < o.mean() < 1
