"""NumPy oracle of ``marex_amd.cell_trends`` and of the two entry points behind it (``marex_trend_stats_f64``,
``marex_trend_select_f64``), written the slow, obvious way: per cell the sort of all pairwise slopes, ``np.unique`` for the
ties, explicit sequential loops over the steps for the sums.  ``stats`` / ``select`` / ``cell_trends`` are the same
definitions vectorised over the cells (one sort of a ``[P, C]`` table), for a few thousand cells; the host tests hold the
two against each other.  Not collected by pytest."""
import math
from statistics import NormalDist

import numpy as np


# ------------------------------------------------------------------------------------------------ one cell at a time
def cell_slopes(y, x):
    """The sorted slopes ``((y_j - y_i) / (x_j - x_i)) + 0.0`` of the pairs ``i < j`` of finite samples of one cell."""
    ok = np.isfinite(y)
    yv, xv = np.asarray(y, np.float64)[ok], np.asarray(x, np.float64)[ok]
    out = []
    with np.errstate(all="ignore"):
        for i in range(yv.size):
            for j in range(i + 1, yv.size):
                out.append((yv[j] - yv[i]) / (xv[j] - xv[i]) + 0.0)
    return np.sort(np.array(out, np.float64))


def cell_stats(y, x):
    """``n, s, ties, med_y, med_x, (xbar, ybar, sxx, sxy, syy)`` of one cell."""
    ok = np.isfinite(y)
    yv, xv = np.asarray(y, np.float64)[ok], np.asarray(x, np.float64)[ok]
    n = int(yv.size)
    s = 0
    for i in range(n):
        for j in range(i + 1, n):
            s += int(yv[j] > yv[i]) - int(yv[j] < yv[i])
    _, t = np.unique(yv, return_counts=True)  # -0.0 and +0.0 are one value
    ties = int((t * (t - 1) * (2 * t + 5)).sum())

    def median(v):
        if v.size == 0:
            return np.nan
        w = np.sort(v)
        return 0.5 * (w[(v.size - 1) // 2] + w[v.size // 2]) + 0.0

    sx = sy = 0.0
    for k in range(n):
        sx = sx + xv[k]
        sy = sy + yv[k]
    with np.errstate(all="ignore"):
        xbar, ybar = np.float64(sx) / np.float64(n), np.float64(sy) / np.float64(n)
        sxx = sxy = syy = np.float64(0.0)
        for k in range(n):
            dx, dy = xv[k] - xbar, yv[k] - ybar
            sxx = sxx + dx * dx
            sxy = sxy + dx * dy
            syy = syy + dy * dy
    return n, s, ties, median(yv), median(xv), (xbar, ybar, sxx, sxy, syy)


def ranks_of(n, ties, alpha):
    """``((P - 1) // 2, P // 2, Rl, Ru)`` of one cell, in Python integers."""
    P = n * (n - 1) // 2
    v18 = n * (n - 1) * (2 * n + 5) - ties
    z = NormalDist().inv_cdf(alpha / 2.0)
    sigma = math.sqrt(v18 / 18.0)
    rl = max(int(np.round((P + z * sigma) / 2.0)) - 1, 0)
    ru = min(int(np.round((P - z * sigma) / 2.0)), P - 1)
    return (P - 1) // 2, P // 2, rl, ru


def cell_trend(y, x, alpha=0.05):
    """Every output of ``cell_trends`` for one cell, as a dict of scalars."""
    n, s, ties, med_y, med_x, (xbar, ybar, sxx, sxy, syy) = cell_stats(y, x)
    sl = cell_slopes(y, x)
    P = sl.size
    v18 = n * (n - 1) * (2 * n + 5) - ties
    var = v18 / 18.0
    pick = [sl[r] if 0 <= r < P else np.nan for r in ranks_of(n, ties, alpha)]
    if n < 2:
        z = p = np.nan
    else:
        z = 0.0 if s == 0 or var == 0.0 else (s - 1) / math.sqrt(var) if s > 0 else (s + 1) / math.sqrt(var)
        p = math.erfc(abs(z) / math.sqrt(2.0))
    sen = 0.5 * (pick[0] + pick[1])
    with np.errstate(all="ignore"):
        ols = sxy / sxx
        rad = (syy - sxy * sxy / sxx) / np.float64(n - 2) / sxx
        stderr = np.nan if n < 3 else math.sqrt(0.0 if rad < 0 else rad)
    return {"n": n, "mk_s": s, "mk_var": var, "mk_z": z, "mk_p": p, "significant": bool(p < alpha), "sen_slope": sen,
            "sen_slope_lo": pick[2], "sen_slope_hi": pick[3], "sen_intercept": med_y - sen * med_x, "ols_slope": ols,
            "ols_intercept": ybar - ols * xbar, "ols_stderr": stderr}


# ------------------------------------------------------------------------------------------------ all cells at once
def _samples(y):
    y = np.asarray(y, np.float64)
    return np.where(np.isfinite(y), y, np.nan)


def stats(y, x):
    """``marex_trend_stats_f64`` for ``y [G, C]``: ``n``, ``s``, ``ties`` int32 ``[C]``, ``med`` ``[2, C]``, ``sums`` ``[5, C]``."""
    yy, x = _samples(y), np.asarray(x, np.float64)
    G, C = yy.shape
    ok = yy == yy
    n = ok.sum(axis=0).astype(np.int32)
    s, ties = np.zeros(C, np.int64), np.zeros(C, np.int64)
    with np.errstate(all="ignore"):
        for i in range(G):
            d = yy[i + 1:] - yy[i]
            s += (d > 0).sum(axis=0) - (d < 0).sum(axis=0)
            t = (yy == yy[i]).sum(axis=0)  # the sample's tie group, itself included; 0 where it is missing
            ties += np.where(ok[i], (t - 1) * (2 * t + 5), 0)

        def median(v):  # NaN sorts last
            w = np.sort(v, axis=0)
            lo = np.take_along_axis(w, np.maximum((n[None, :] - 1) // 2, 0), axis=0)[0]
            up = np.take_along_axis(w, np.minimum(n[None, :] // 2, G - 1), axis=0)[0]
            return np.where(n > 0, 0.5 * (lo + up) + 0.0, np.nan)

        med = np.stack([median(yy), median(np.where(ok, x[:, None], np.nan))])
        sx, sy = np.zeros(C), np.zeros(C)
        for k in range(G):  # sequential, ascending steps
            sx = np.where(ok[k], sx + x[k], sx)
            sy = np.where(ok[k], sy + yy[k], sy)
        xbar, ybar = sx / n.astype(np.float64), sy / n.astype(np.float64)
        sxx, sxy, syy = np.zeros(C), np.zeros(C), np.zeros(C)
        for k in range(G):
            dx, dy = x[k] - xbar, yy[k] - ybar
            sxx = np.where(ok[k], sxx + dx * dx, sxx)
            sxy = np.where(ok[k], sxy + dx * dy, sxy)
            syy = np.where(ok[k], syy + dy * dy, syy)
    return {"n": n, "s": s.astype(np.int32), "ties": ties.astype(np.int32), "med": med,
            "sums": np.stack([xbar, ybar, sxx, sxy, syy])}


def sorted_slopes(y, x):
    """``[G (G - 1) / 2, C]``: every cell's slopes sorted, NaN (a pair with a missing sample) last."""
    yy, x = _samples(y), np.asarray(x, np.float64)
    iu, ju = np.triu_indices(yy.shape[0], 1)
    with np.errstate(all="ignore"):
        sl = (yy[ju] - yy[iu]) / (x[ju] - x[iu])[:, None] + 0.0
    return np.sort(sl, axis=0)


def select(y, x, ranks, slopes=None):
    """``marex_trend_select_f64``: float64 ``[K, C]``, NaN for a rank outside ``0 .. P - 1``."""
    sl = sorted_slopes(y, x) if slopes is None else slopes
    r = np.asarray(ranks).astype(np.int64)
    n = np.isfinite(np.asarray(y, np.float64)).sum(axis=0).astype(np.int64)
    P = n * (n - 1) // 2
    got = np.take_along_axis(sl, np.clip(r, 0, sl.shape[0] - 1), axis=0)
    return np.where((r >= 0) & (r < P[None, :]), got, np.nan)


def cell_trends(y, x, alpha=0.05):
    """Every output of ``marex_amd.cell_trends`` for ``y [G, C]``, as a dict of ``[C]`` arrays; built on ``stats`` and
    ``select`` and on the per-cell rank and test rules above, never on the package."""
    st = stats(y, x)
    n, s, ties = st["n"], st["s"], st["ties"]
    C = n.size
    ranks = np.array([ranks_of(int(n[c]), int(ties[c]), alpha) for c in range(C)], np.int64).T.reshape(4, C)
    sel = select(y, x, ranks)
    n64 = n.astype(np.int64)
    v18 = n64 * (n64 - 1) * (2 * n64 + 5) - ties
    var = v18 / 18.0
    z, p = np.full(C, np.nan), np.full(C, np.nan)
    for c in range(C):
        if n[c] >= 2:
            S = int(s[c])
            z[c] = 0.0 if S == 0 or var[c] == 0.0 else (S - 1) / math.sqrt(var[c]) if S > 0 else (S + 1) / math.sqrt(var[c])
            p[c] = math.erfc(abs(z[c]) / math.sqrt(2.0))
    xbar, ybar, sxx, sxy, syy = st["sums"]
    with np.errstate(all="ignore"):
        sen = 0.5 * (sel[0] + sel[1])
        ols = sxy / sxx
        rad = (syy - sxy * sxy / sxx) / (n - 2) / sxx
        stderr = np.where(n < 3, np.nan, np.sqrt(np.where(rad < 0, 0.0, rad)))
        return {"n": n, "mk_s": s, "mk_var": var, "mk_z": z, "mk_p": p, "significant": p < alpha, "sen_slope": sen,
                "sen_slope_lo": sel[2], "sen_slope_hi": sel[3], "sen_intercept": st["med"][0] - sen * st["med"][1],
                "ols_slope": ols, "ols_intercept": ybar - ols * xbar, "ols_stderr": stderr}
