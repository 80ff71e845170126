"""Seeded cases for the tracker's gridded pre-processing kernels (csrc/marex_morphology.hip: marex_fill_holes_u8 with
k_morph_pack, k_morph_pass, k_morph_unpack, k_mask_and; marex_time_closing_u8 with k_time_closing16, k_time_closing; the
sweeps of marex_fill_holes_mesh_u8): plain NumPy and SciPy, no device, no torch.  Not a test module.

* ``fill_geometry`` / ``closing_geometry`` restate the launch arithmetic of the two entry points, so that a case can say
  which edge of the launch it is there for (tests/test_track_pre_cases_host.py pins the restated lines to the source and
  proves every case reaches its edge).
* ``fill_holes_distance`` and ``time_closing_runs`` are second references that call no ``scipy.ndimage.binary_*``: the
  disk dilation as "squared integer distance to the nearest True cell <= R^2", the time closing as a rule on run lengths.
  The host test shows them bit-equal to the oracle; the distance form is also what makes R = 63 affordable.
* Every builder is a pure function of its arguments (fixed seeds).  tests/test_gpu_track_pre_edges.py runs the cases on
  the device.
"""
import functools
import zlib
from types import SimpleNamespace

import numpy as np

R_MAX = 63            # marex_fill_holes_u8 refuses a larger radius
MESH_R_MAX = 1024     # marex_fill_holes_mesh_u8
PACK_GRID_CAP = 1 << 20
PACK_W0_STRIDE = 4 * 8
TC_TBLOCK = 32


def _rng(*key):
    return np.random.default_rng(zlib.crc32(repr(key).encode()))


# ------------------------------------------------------------------------------------------------------------------------
# restated launch geometry
# ------------------------------------------------------------------------------------------------------------------------
def fill_geometry(T, ny, nx, R):
    """``(Hp, nxp, Wp, last_bits, rows, pack_trips_per_wave)`` of marex_fill_holes_u8 with ``R > 0``: the padded image is
    ``Hp x nxp`` cells, a padded row ``Wp`` 64-bit words whose last holds ``last_bits`` cells; k_morph_pack has ``rows``
    padded rows to pack (one workgroup each, the grid capped at ``PACK_GRID_CAP``), and wave ``w`` of its four makes
    ``pack_trips_per_wave[w]`` trips through ``for (w0 = wave; w0 < Wp; w0 += 32)``."""
    Hp, nxp = ny + 4 * R, nx + 4 * R
    Wp = (nxp + 63) // 64
    last_bits = nxp - 64 * (Wp - 1)
    trips = tuple(len(range(wave, Wp, PACK_W0_STRIDE)) for wave in range(4))
    return Hp, nxp, Wp, last_bits, T * Hp, trips


def closing_geometry(T, C, T_fill, aligned=True):
    """``(kernel, time_blocks, c)`` of marex_time_closing_u8: ``"wide"`` (k_time_closing16, 16 cells per thread,
    ``time_blocks`` values of blockIdx.y) when ``C`` is a multiple of 16 and both pointers are 16-byte aligned,
    ``"scalar"`` (k_time_closing, one launch dimension) otherwise; ``c`` is the half-width of the window."""
    wide = C % 16 == 0 and aligned
    return ("wide" if wide else "scalar"), ((T + TC_TBLOCK - 1) // TC_TBLOCK if wide else 1), T_fill // 2


# ------------------------------------------------------------------------------------------------------------------------
# second reference of the fill: distances, not structuring elements
# ------------------------------------------------------------------------------------------------------------------------
def dilate_distance(img, R):
    """Dilation of bool ``[T, H, W]`` per image with the disk ``x^2 + y^2 < R^2 + 1``, False outside the image: a cell is
    set exactly when the squared distance to the nearest True cell of its image, in integers, is ``<= R^2``.  The nearest
    cell comes from the feature transform of scipy's EDT (its indices, never its float distance); several images go
    through one call with the time axis stretched so far that no cell of another image can be nearer than one's own."""
    from scipy import ndimage as ndi

    img = np.asarray(img, dtype=bool)
    T, H, W = img.shape
    out = np.zeros_like(img)
    stretch = H + W  # stretch^2 > (H - 1)^2 + (W - 1)^2, the largest squared distance inside one image
    step = max(1, 2_000_000 // (H * W))
    yy = np.arange(H, dtype=np.int64)[None, :, None]
    xx = np.arange(W, dtype=np.int64)[None, None, :]
    for t0 in range(0, T, step):
        blk = img[t0:t0 + step]
        if not blk.any():
            continue
        it, iy, ix = ndi.distance_transform_edt(~blk, sampling=(stretch, 1, 1), return_distances=False, return_indices=True)
        own = it == np.arange(blk.shape[0])[:, None, None]  # an image without a True cell finds one elsewhere: never set
        d2 = (iy.astype(np.int64) - yy) ** 2 + (ix.astype(np.int64) - xx) ** 2
        out[t0:t0 + step] = own & (d2 <= R * R)
    return out


def erode_distance(img, R):
    """Erosion with the same disk and ``border_value = 0``: the complement of the dilation of the complement, the
    outside made part of that complement by a ring of ``R + 1`` False cells, removed again afterwards."""
    k = R + 1
    p = np.pad(np.asarray(img, dtype=bool), ((0, 0), (k, k), (k, k)), mode="constant", constant_values=False)
    return ~dilate_distance(~p, R)[:, k:-k, k:-k]


def fill_holes_distance(data_bin, mask, R, regional=False, padded=False):
    """The oracle's chain (pad by 2R with wrap / edge, close, open, trim, ``& mask``) on the two functions above.
    ``padded=True`` returns the padded input and the padded result before the trim instead (what the packed words hold
    before the first and after the last pass)."""
    x = np.asarray(data_bin, dtype=bool)
    mask = np.asarray(mask, dtype=bool)
    R = int(R)
    if R == 0:
        return (x, x) if padded else x & mask[None]
    d = 2 * R
    p0 = np.pad(x, ((0, 0), (d, d), (d, d)), mode="edge" if regional else "wrap")
    p = erode_distance(dilate_distance(p0, R), R)
    p = dilate_distance(erode_distance(p, R), R)
    if padded:
        return p0, p
    return p[:, d:-d, d:-d] & mask[None]


# ------------------------------------------------------------------------------------------------------------------------
# second reference of the time closing: run lengths
# ------------------------------------------------------------------------------------------------------------------------
def time_closing_runs(x, T_fill):
    """Closing of bool ``[T, C]`` along time with ``T_fill + 1`` ones, False outside the series, as a rule: a False step
    becomes True exactly when it lies in a run of at most ``T_fill`` False steps with a True step on both sides."""
    x = np.asarray(x, dtype=bool)
    T = x.shape[0]
    t = np.arange(T, dtype=np.int64).reshape((T,) + (1,) * (x.ndim - 1))
    prev = np.maximum.accumulate(np.where(x, t, -1), axis=0)                       # last True step at or before t
    nxt = np.minimum.accumulate(np.where(x, t, T)[::-1], axis=0)[::-1]             # first True step at or after t
    return x | ((prev >= 0) & (nxt < T) & (nxt - prev - 1 <= int(T_fill)))


# ------------------------------------------------------------------------------------------------------------------------
# fill cases
# ------------------------------------------------------------------------------------------------------------------------
def structured_field(R, T=2):
    """A field that stays interesting at every radius (random blobs close into one sheet at R = 63): on a grid of
    ``(6R + 11) x (8R + 13)`` two discs of radius 1.5R and 1.3R, each with an off-centre hole of radius 0.45R that the
    closing fills; a striped bar on the first columns, i.e. on the periodic seam and on the regional border; per step 4
    single-cell specks and 60 pinholes (counts, not densities: a density joins up under a large closing); a strip of
    land across the second disc.  Later steps move the discs a little.  Returns ``(x [T, ny, nx], mask [ny, nx])``."""
    rng = _rng("structured", R)
    ny, nx = 6 * R + 11, 8 * R + 13
    yy, xx = np.mgrid[0:ny, 0:nx]
    x = np.zeros((T, ny, nx), dtype=bool)
    mask = np.ones((ny, nx), dtype=bool)
    cxb = int(5.9 * R) + 8
    mask[:, cxb + R // 3:cxb + R // 3 + max(1, R // 4)] = False
    bar_w, stripe = max(2, R // 2), max(1, R // 3)
    for t in range(T):
        for (cy, cx, rad) in ((1.8 * R + 4 + t, 2.4 * R + 8 + 2 * t, 1.5 * R), (4.2 * R + 6 - t, 5.9 * R + 8 - t, 1.3 * R)):
            disc = (yy - cy) ** 2 + (xx - cx) ** 2 <= rad * rad
            hole = (yy - (cy + 0.5 * R)) ** 2 + (xx - (cx - 0.4 * R)) ** 2 <= (0.45 * R) ** 2
            x[t] |= disc & ~hole
        x[t, :, :bar_w] |= (((yy[:, :bar_w] + t) // stripe) % 2 == 0)
        on = np.flatnonzero(x[t])
        x[t].reshape(-1)[rng.choice(on, 60, replace=False)] = False                   # pinholes
        off = np.flatnonzero(~x[t])
        x[t].reshape(-1)[rng.choice(off, 4, replace=False)] = True                    # specks
    return x & mask[None], mask


def word_edge_field(nx, R):
    """T = 2, ny = 3: random at 30 % plus a solid block over the last 70 columns (the last quarter of a row narrower than
    140 cells), so that the last words of a padded row -- those past word 31 on the wide rows -- carry set bits in the
    input and in the result.  One cell in ten is land."""
    rng = _rng("word", nx, R)
    x = rng.random((2, 3, nx)) < 0.3
    x[:, :, -(70 if nx > 140 else nx // 4):] = True
    return x, rng.random((3, nx)) < 0.9


def tail_band_field(nx, R):
    """What makes the bits past the row end matter to the trimmed result: a solid band on the last R columns behind a moat
    of 3R False columns (wider than a closing bridges), and on the first 2R columns, so that under either padding the band
    runs on to the right border of the padded image, 3R cells wide.  The closing takes R cells off it at the border (False outside), the opening then
    removes what is left, 2R wide, entirely; if the dilation's spill into the unused bits of the last word were kept, the
    erosion would read it as image, take nothing off, and the band would survive.  Random at 30 % elsewhere."""
    rng = _rng("tail", nx, R)
    x = rng.random((2, 3, nx)) < 0.3
    x[:, :, nx - 4 * R:nx - R] = False
    x[:, :, nx - R:] = True
    x[:, :, :2 * R] = True
    return x, np.ones((3, nx), dtype=bool)


ROW_STRIDE_SHAPE =(116509, 5, 8, 1)  # (T, ny, nx, R): T * Hp = 1 048 581 padded rows, five more than the grid cap


def row_stride_field():
    """Random 5 x 8 images at 45 %; the last two steps, whose padded rows are the ones past the grid cap, are set by hand:
    not empty, not what the first two steps hold."""
    T, ny, nx, _ = ROW_STRIDE_SHAPE
    rng = _rng("rows")
    x = rng.random((T, ny, nx)) < 0.45
    x[-2] = False
    x[-2, 0:4, :] = True
    x[-2, 1, 3] = False
    x[-1] = False
    x[-1, 1:5, 2:7] = True
    x[-1, 4, 0] = True
    mask = np.ones((ny, nx), dtype=bool)
    mask[2, 5] = False
    return x, mask


NARROW_DENSITIES = (0.0, 1.0, 0.2, 0.5, 0.8)  # one timestep each


def narrow_field(ny, nx):
    """Grids far narrower than 2R: np.pad's "wrap" repeats them many times.  Steps: all False, all True, three densities."""
    rng = _rng("narrow", ny, nx)
    x = np.stack([rng.random((ny, nx)) < d for d in NARROW_DENSITIES])
    mask = rng.random((ny, nx)) < 0.85
    mask.reshape(-1)[0] = True
    return x, mask


WORD_EDGE_NXP = (64, 65, 128, 2048, 2049)
TAIL_BAND_NXP = (65, 100, 2049)  # 1, 36 and 1 cells in the last word: 63, 28 and 63 bits past the row end
STRUCTURED_R = (12, 31, 62, 63)
NARROW_GRIDS = ((1, 1), (1, 7), (5, 3), (2, 64))


@functools.lru_cache(maxsize=None)
def fill_cases():
    """Every fill case: ``name`` (its id), ``kind``, the shape ``T, ny, nx``, ``R``, ``regional`` and ``build`` (a
    function of nothing that returns ``(x, mask)``)."""
    cases = []

    def add(kind, name, T, ny, nx, R, regional, build):
        mode = "regional" if regional else "periodic"
        cases.append(SimpleNamespace(kind=kind, name=f"{name}-R{R}-{mode}", T=T, ny=ny, nx=nx, R=R, regional=regional, build=build))

    for regional in (False, True):
        for R in (1, 2):
            for nxp in WORD_EDGE_NXP:
                nx = nxp - 4 * R
                add("word", f"nxp{nxp}", 2, 3, nx, R, regional, functools.partial(word_edge_field, nx, R))
        add("word", "nx2300", 2, 3, 2300, 1, regional, functools.partial(word_edge_field, 2300, 1))
        for R in (1, 2):
            for nxp in TAIL_BAND_NXP:
                add("tail", f"band-nxp{nxp}", 2, 3, nxp - 4 * R, R, regional, functools.partial(tail_band_field, nxp - 4 * R, R))
        for R in STRUCTURED_R:
            add("radius", "structured", 2, 6 * R + 11, 8 * R + 13, R, regional, functools.partial(structured_field, R))
        for (ny, nx) in NARROW_GRIDS:
            for R in (5, 31):
                add("narrow", f"{ny}x{nx}", len(NARROW_DENSITIES), ny, nx, R, regional, functools.partial(narrow_field, ny, nx))
    T, ny, nx, R = ROW_STRIDE_SHAPE
    add("rows", "rows", T, ny, nx, R, False, row_stride_field)
    return tuple(cases)


def fill_case(name):
    return next(c for c in fill_cases() if c.name == name)


@functools.lru_cache(maxsize=None)
def fill_inputs(name):
    """``(x, mask)`` of the named case; shared, so leave them unchanged."""
    c = fill_case(name)
    x, mask = c.build()
    assert x.shape == (c.T, c.ny, c.nx) and mask.shape == (c.ny, c.nx)
    x.setflags(write=False)
    mask.setflags(write=False)
    return x, mask


# ------------------------------------------------------------------------------------------------------------------------
# time closing cases
# ------------------------------------------------------------------------------------------------------------------------
CLOSING_T = (1, 31, 32, 33, 64, 65, 97)
CLOSING_C_WIDE = (16, 4096, 4112)   # 4 112 = two workgroups of the wide kernel, the second with one active lane
CLOSING_C_SCALAR = (1, 15, 17, 4097)
CLOSING_C_MAX = 4112
GAP_PLACES = ("31|32", "63|64", "start", "after_first", "end", "before_last")


def closing_t_fills(T):
    return tuple(sorted({0, 2, 4, 16, 18, 2 * T}))


def _gap(T, place, g):
    """Steps ``[a, b)`` of a gap of ``g`` False steps at ``place``; None where the series has no room for it."""
    if place in ("31|32", "63|64"):
        edge = 32 if place == "31|32" else 64
        if edge >= T:
            return None
        a = edge - (g + 1) // 2  # g >= 2: steps edge - 1 and edge are both in the gap; g = 1: step edge - 1
    else:
        a = {"start": 0, "after_first": 1, "end": T - g, "before_last": T - 1 - g}[place]
    return (a, a + g) if a >= 0 and a + g <= T else None


@functools.lru_cache(maxsize=None)
def closing_columns(T, T_fill):
    """The distinct columns of the closing fields of one ``(T, T_fill)``: bool ``[T, n]`` and a name per column.

    * ``pair``: True, a gap of ``T_fill`` steps (closed), True, a gap of ``T_fill + 1`` (left open), True -- where T has
      room for it, so that the single column of C = 1 carries both outcomes.
    * ``ends_only``: True at the first and at the last step, a gap of T - 2 (closed by the windows as wide as the series);
      ``first_only``: True at the first step, nothing to close.  All False, all True.
    * ``gap<g>@<place>``: all True but for one gap of ``g`` in ``T_fill - 1, T_fill, T_fill + 1`` steps that straddles
      steps 31|32 or 63|64 (two time blocks of the wide kernel), starts the series (nothing to its left: stays open),
      follows the first step, ends the series, or precedes the last step -- where the series has room for it.
    * 24 random columns at 50 % and 10 % from which whole steps are removed, in turn with the gap columns.
    """
    rng = _rng("closing", T, T_fill)
    cols, names = [], []
    if T >= 2 * T_fill + 4:
        v = np.ones(T, dtype=bool)
        v[1:1 + T_fill] = False
        v[2 + T_fill:3 + 2 * T_fill] = False
        cols.append(v)
        names.append("pair")
    if T >= 3:
        v = np.zeros(T, dtype=bool)
        v[[0, T - 1]] = True
        cols.append(v)
        names.append("ends_only")
    if T >= 2:
        v = np.zeros(T, dtype=bool)
        v[0] = True
        cols.append(v)
        names.append("first_only")
    cols += [np.zeros(T, dtype=bool), np.ones(T, dtype=bool)]
    names += ["all_false", "all_true"]
    gaps = []
    for g in (T_fill - 1, T_fill, T_fill + 1):
        for place in GAP_PLACES:
            ab = _gap(T, place, g) if g >= 1 else None
            if ab is not None:
                v = np.ones(T, dtype=bool)
                v[ab[0]:ab[1]] = False
                gaps.append((f"gap{g}@{place}", v))
    r = np.concatenate([rng.random((T, 12)) < 0.5, rng.random((T, 12)) < 0.1], axis=1)
    r[rng.random(T) < 0.3] = False
    r = r[:, rng.permutation(24)]
    rand = [(f"random{j}", r[:, j]) for j in range(24)]
    while gaps or rand:
        for src in (gaps, rand):
            if src:
                k, v = src.pop(0)
                names.append(k)
                cols.append(v)
    out = np.stack(cols, axis=1)
    out.setflags(write=False)
    return out, tuple(names)


@functools.lru_cache(maxsize=None)
def _closing_pick(n):
    """Which distinct column stands at each of the CLOSING_C_MAX positions: every one once, then a seeded draw."""
    return np.concatenate([np.arange(n), _rng("pick", n).integers(0, n, CLOSING_C_MAX)])[:CLOSING_C_MAX]


def closing_field(T, C, T_fill):
    """bool ``[T, C]``: the leading C columns of one field per ``(T, T_fill)`` made of the distinct columns above, so that
    the references need only be compared on those (a column's closing depends on nothing but the column)."""
    base, _ = closing_columns(T, T_fill)
    return np.ascontiguousarray(base[:, _closing_pick(base.shape[1])[:C]])


def closing_cases():
    """``(T, T_fill)`` pairs; each is run at every width of CLOSING_C_WIDE and CLOSING_C_SCALAR."""
    return tuple((T, tf) for T in CLOSING_T for tf in closing_t_fills(T))


CHAINED = SimpleNamespace(T=65, ny=24, nx=32, R_fill=4, T_fill=4)


def chained_field():
    """fill_time_gaps end to end: coarse random blobs, specks, whole steps missing; C = 768 takes the wide kernel in
    three time blocks."""
    c = CHAINED
    rng = _rng("chained")
    x = np.kron(rng.random((c.T, c.ny // 4, c.nx // 4)) < 0.3, np.ones((1, 4, 4), dtype=bool))
    x ^= rng.random(x.shape) < 0.02
    x[rng.random(c.T) < 0.3] = False
    mask = np.ones((c.ny, c.nx), dtype=bool)
    mask[5:9, 10:13] = False
    return x & mask[None], mask


# ------------------------------------------------------------------------------------------------------------------------
# mesh cases
# ------------------------------------------------------------------------------------------------------------------------
MESH_C = 257
MESH_R = (0, 1, 40, 200, 1024)  # from R = 129 a dilation has gone round the ring, chords or not


def mesh_ring():
    """A ring of 257 cells with chords: ``(x [5, C], mask [C], nbr int32 [3, C])``.  Some cells list themselves, some
    links are listed from one end only, cell 240 lists nobody (its ring neighbours still list it), cells 100..130 are
    land.  Steps: two clusters with a hole, scattered cells, a single cell, the whole ocean, the ocean less two cells (at
    the larger radii the first three come out empty, the last two full)."""
    C = MESH_C
    i = np.arange(C)
    nbr = np.full((3, C), -1, dtype=np.int32)
    nbr[0] = (i + 1) % C
    nbr[1] = (i - 1) % C
    for a, b, both in ((3, 120, True), (40, 200, False), (77, 210, True), (150, 30, False), (222, 90, False)):
        nbr[2, a] = b
        if both:
            nbr[2, b] = a
    nbr[2, [10, 60, 130]] = [10, 60, 130]
    nbr[1, [20, 21, 95, 180]] = -1
    nbr[:, 240] = -1
    mask = np.ones(C, dtype=bool)
    mask[100:131] = False
    x = np.zeros((5, C), dtype=bool)
    x[0, 50:61] = True
    x[0, 55] = False
    x[0, 160:176] = True
    x[0, 166:168] = False
    x[1] = _rng("mesh").random(C) < 0.08
    x[2, 5] = True
    x[3:] = True
    x[4, [50, 200]] = False
    return x & mask[None], mask, nbr
