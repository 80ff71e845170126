"""The shared cases of the regional series tests: fields, region maps, areas, anomalies and thresholds at the edges of the
kernel's layout, and the comparison of an engine result with the oracle.  Not collected by pytest."""
import numpy as np

import regional_series_oracle as ro

F = np.float32
NAN, INF = np.nan, np.inf
from marex_amd.csrc import build as _build
from marex_amd.engine import HotPath

_build.build(verbose=False)  # hipcc cross-compiles without a GPU
# the layout the kernels of marex_regional_series_* were compiled with, from the library itself (marex_regional_layout):
# cells of a 64-lane piece, a wave and a workgroup per row at four cells per lane (uint8 without thresholds, C % 4 == 0,
# aligned) and at one; rows between two of a workgroup's
PIECE = {4: 256, 1: 64}
WAVE = {v: HotPath.regional_layout(v)[0] for v in (4, 1)}
WG = {v: HotPath.regional_layout(v)[1] for v in (4, 1)}
ROW_STRIDE = HotPath.regional_layout(1)[2]
assert HotPath.regional_layout(4)[2] == ROW_STRIDE and all(WAVE[v] % PIECE[v] == 0 and WG[v] == 4 * WAVE[v] for v in (4, 1))
POISON = 0xCD


def layout_edges():
    """Row lengths one below, at and above a wave pass and a workgroup of both layouts, and -- for the layout of four cells
    per lane, which needs ``C % 4 == 0`` -- one vector of four below and above them."""
    out = set()
    for v in (4, 1):
        for n in (WAVE[v], WG[v]):
            out.update((n - 1, n, n + 1))
    for n in (WAVE[4], WG[4]):
        out.update((n - 4, n + 4))
    return sorted(out)


def layout_cuts(C):
    """The cell indices below ``C`` at which a piece, a wave pass or a workgroup of either layout begins."""
    return sorted({p for v in (4, 1) for step in (PIECE[v], WAVE[v], WG[v]) for p in range(step, C, step)})


def dyadic_anomalies(rng, shape):
    """Multiples of 2^-10 below 64 in magnitude: with the weights below every partial sum of w a is exact in float64."""
    return (rng.integers(-(2**16) + 1, 2**16, shape) / 1024.0).astype(F)


def dyadic_weights(rng, C):
    """Multiples of 2^-8 below 2^10."""
    return (rng.integers(0, 2**18, C) / 256.0).astype(F)


def mask_field(rng, T, C, cover=0.35):
    x = (rng.random((T, C)) < cover).astype(np.uint8)
    x[:, 0] = 1  # a cell present throughout
    return x


def id_field(rng, T, C, cover=0.4, n_ids=5):
    return np.where(rng.random((T, C)) < cover, rng.integers(1, n_ids + 1, (T, C)), 0).astype(np.int32)


def edge_regions(C):
    """Regions whose edges lie exactly at and one cell past every piece, wave and workgroup boundary of both layouts below
    ``C``, a region without cells, and cells whose index lies at ``R``, above it and below 0: ``(reg int32 [C], R)``."""
    cuts = set()
    for p in layout_cuts(C):
        cuts.update((p, p + 1))
    cuts = np.array(sorted(c for c in cuts if c < C), np.int64)
    reg = np.searchsorted(cuts, np.arange(C), side="right").astype(np.int32)
    reg[reg >= 3] += 1  # region 3 holds no cell
    R = int(reg.max()) + 1
    reg[5::97] = R
    reg[11::89] = R + 1000
    reg[17::83] = -1
    reg[23::79] = -(2**31)
    return reg, R


def region_map(name, C):
    c = np.arange(C)
    if name == "one":
        return np.zeros(C, np.int32), 1
    if name == "holes":
        return np.where(c % 7 == 3, -1, 0).astype(np.int32), 1
    if name == "own":
        return c.astype(np.int32), C
    if name == "mod3":
        return (c % 3).astype(np.int32), 3
    if name == "edges":
        return edge_regions(C)
    raise KeyError(name)


def thresholds(rng, n_doy, C):
    thr = rng.uniform(0.3, 1.5, (n_doy, C)).astype(F)
    thr[:, 1 % C] = NAN  # class 5
    thr[0, 2 % C], thr[n_doy - 1, 3 % C] = 0.0, -1.0
    return thr


def spoil(rng, anom, x):
    """NaN and both infinities under present cells."""
    p = np.argwhere(x > 0)
    pick = p[rng.permutation(len(p))[:max(3, len(p) // 10)]]
    for n, (t, c) in enumerate(pick):
        anom[t, c] = (NAN, INF, -INF)[n % 3]
    return anom


def near_2_61(rng, C):
    """Areas whose fixed-point table sums to just under 2^61: ``(e, q, wf)``."""
    from marex_amd.regional import area_weight_table

    a = rng.uniform(0.5, 1.0, C)
    a *= 1024.0 * (1 - 1e-12) / a.sum()
    while float(a.sum()) > 1024.0:
        a *= 1 - 1e-15
    e, q = area_weight_table(a)
    total = sum(int(v) for v in q)
    assert 2**61 - 2**40 < total <= 2**61 + C, total
    return e, q, a.astype(F)


def device_field(hot, x, offset=0):
    """``x`` on the engine's device, its first byte ``offset`` bytes past an aligned address."""
    import torch

    t = torch.from_numpy(np.ascontiguousarray(x))
    if not offset:
        return t.to(hot.device)
    assert x.dtype == np.uint8
    buf = torch.empty(x.size + offset, dtype=torch.uint8, device=hot.device)
    assert buf.data_ptr() % 16 == 0
    v = buf[offset:].view(x.shape)
    v.copy_(t)
    return v


def run_engine(hot, x, reg, R, q=None, wf=None, anom=None, thr=None, doy=None, match=0, cuts=None, offset=0):
    """``HotPath.regional_series`` over the windows between ``cuts`` (one call by default); the spare row of every slot
    buffer must still hold the poison of a fresh buffer."""
    import torch

    T = x.shape[0]
    xt = device_field(hot, x, offset)
    at = None if anom is None else torch.from_numpy(np.ascontiguousarray(anom, dtype=F)).to(hot.device)
    tt = None if thr is None else torch.from_numpy(np.ascontiguousarray(thr, dtype=F)).to(hot.device)
    cuts = sorted(set(cuts or (0, T)))
    acc = r = None
    for a, b in zip(cuts[:-1], cuts[1:]):
        r = hot.regional_series(xt[a:b], reg, R, T, t0=a, q=q, wf=wf, anom=None if at is None else at[a:b], thr=tt, doy=doy,
                                match=match, acc=acc, finish=b == T)
        acc = r["acc"]
    assert hot.POISON
    for k in ("area", "cnt", "sums", "vmax", "cat_cnt", "cat_area"):
        if acc[k] is not None:
            spare = acc[k][T].cpu().numpy().view(np.uint8)
            assert spare.size and (spare == POISON).all(), k
    return r


def oracle(x, reg, R, q=None, wf=None, anom=None, thr=None, doy=None, match=0):
    return ro.finish(ro.accumulate(x, reg, R, x.shape[0], 0, q, wf, anom, thr, doy, match))


def assert_same(r, exp, float_bytes=True):
    """Integers equal; the maximum equal; the float64 sums byte for byte (``float_bytes``: dyadic inputs)."""
    for k in ("area", "cnt", "cat_cnt", "cat_area"):
        assert (r[k] is None) == (exp[k] is None), k
        if exp[k] is not None:
            assert r[k].dtype == np.int64 and r[k].shape == exp[k].shape, (k, r[k].dtype, r[k].shape)
            assert np.array_equal(r[k], exp[k]), (k, np.argwhere(r[k] != exp[k])[:5])
    assert (r["vmax"] is None) == (exp["vmax"] is None)
    if exp["vmax"] is not None:
        assert r["vmax"].dtype == np.float32 and np.array_equal(r["vmax"], exp["vmax"], equal_nan=True)
        assert np.array_equal(np.signbit(r["vmax"]), np.signbit(exp["vmax"]))
        if float_bytes:
            assert r["sums"].dtype == np.float64 and r["sums"].tobytes() == exp["sums"].tobytes()


def assert_within_bound(r, x, reg, R, wf, anom, match=0):
    """The two sums against ``math.fsum`` of the exact terms: within 2 n u sum|term|."""
    W, S, A, n = ro.exact_sums(x, reg, R, wf, anom, match)
    Wabs = W  # the weights are not negative
    dW, dS = np.abs(r["sums"][..., 0] - W), np.abs(r["sums"][..., 1] - S)
    print("largest error of sum w: %.3e of bound %.3e; of sum w a: %.3e of bound %.3e"
          % (dW.max(), (2 * n * ro.U * Wabs).max(), dS.max(), (2 * n * ro.U * A).max()))
    assert (dW <= 2 * n * ro.U * Wabs).all()
    assert (dS <= 2 * n * ro.U * A).all()
    assert np.array_equal(r["cnt"][..., 0], n)
