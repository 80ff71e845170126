"""NumPy restatements of the heat stress statistics (``marex_group_mean_f32``, ``marex_heat_stress_f32``), two of each:

* ``walk`` / ``group_walk``: row loops that carry the state as the kernels do -- the running sum S of every cell, updated as
  ``S += h[t]; S -= h[t - window]`` with the leaving step recomputed from its sample, and the accumulators of every
  (group, cell) -- taking windows with their history rows and ``t0``;
* ``direct`` / ``group_direct_counts``: the definitions -- ``math.fsum`` over each window of each cell, the class and the
  maxima from it; the counts of the climatology (its sums have an order, which only the row loop states).

Not collected by pytest."""
import math

import numpy as np

F = np.float32


def hotspot(x, m, hmin):
    """``(d, valid, h)`` of the samples ``x [.., C]`` against ``m [C]``: the float32 difference, the validity of the step
    and the counted HotSpot."""
    x, m = np.asarray(x, F), np.asarray(m, F)
    with np.errstate(invalid="ignore", over="ignore"):
        d = (x - m).astype(F)
        valid = np.isfinite(x) & np.isfinite(m) & (np.abs(d) < F(1024))
        h = np.where(valid & (d >= F(hmin)), d, F(0)).astype(F)
    return d, valid, h


def alert_class(d, valid, w, hmin, lev):
    with np.errstate(invalid="ignore"):
        n = np.zeros(np.shape(d), np.int64)
        for v in np.asarray(lev, F):
            n += w >= v
        return np.where(~valid, 255, np.where(d <= 0, 0, np.where(d < F(hmin), 1, 2 + n))).astype(np.uint8)


def new_state(C, G, L):
    return {"S": np.zeros(C, np.float64), "dhw_max": np.full((G, C), np.nan, F), "tmax": np.full((G, C), -1, np.int32),
            "hotspot_max": np.full((G, C), np.nan, F), "alert_steps": np.zeros((G, 3 + L, C), np.uint32),
            "invalid": np.zeros((G, C), np.uint32), "onset": np.full((G, L, C), -1, np.int32), "status": 0}


def walk(x, m, t0=0, lead=0, window=84, hmin=1.0, spw=7.0, lev=(4.0, 8.0), grp=None, G=1, dhw=None, alert=None, state=None):
    """The rows ``t0 .. t0 + Tb - 1``: ``x [lead + Tb, C]`` begins ``lead = min(window, t0)`` rows before them.  ``dhw`` /
    ``alert``: the whole outputs, written at the global step.  Returns the state, continued from ``state``."""
    x, m, lev = np.asarray(x, F), np.asarray(m, F), np.asarray(lev, F).reshape(-1)
    assert lead == min(window, t0) and x.ndim == 2
    Tb, C, L = x.shape[0] - lead, x.shape[1], lev.size
    st = new_state(C, G, L) if state is None else state
    mok = np.isfinite(m)
    for r in range(Tb):
        t = t0 + r
        d, valid, h = hotspot(x[lead + r], m, hmin)
        st["S"] += h.astype(np.float64)
        if t >= window:
            st["S"] -= hotspot(x[lead + r - window], m, hmin)[2].astype(np.float64)
        w = np.where(mok, (st["S"] / np.float64(spw)).astype(F), F(np.nan))
        a = alert_class(d, valid, w, hmin, lev)
        if dhw is not None:
            dhw[t] = w
        if alert is not None:
            alert[t] = a
        g = 0 if grp is None else int(grp[t])
        if not 0 <= g < G:
            st["status"] += C
            continue
        with np.errstate(invalid="ignore"):
            up = mok & (np.isnan(st["dhw_max"][g]) | (w > st["dhw_max"][g]))
            st["dhw_max"][g][up], st["tmax"][g][up] = w[up], t
            up = valid & (np.isnan(st["hotspot_max"][g]) | (d > st["hotspot_max"][g]))
            st["hotspot_max"][g][up] = d[up]
            st["invalid"][g] += a == 255
            for q in range(3 + L):
                st["alert_steps"][g, q] += a == q
            for j in range(L):
                first = (st["onset"][g, j] < 0) & (w >= lev[j])
                st["onset"][g, j][first] = t
    return st


def window_sums_int(h, window):
    """The exact window sums of the counted HotSpots ``h [T, C]`` in integers: every ``h`` is a multiple of 2^-33 below 2^10,
    so ``h * 2^33`` is an int64 below 2^43, its prefix sums stay below 2^63 for T < 2^20, and a window's sum, below 2^52,
    converts to float64 without rounding.  For fields too large for ``math.fsum`` in a Python loop."""
    q = np.ldexp(h.astype(np.float64), 33)
    assert h.shape[0] < 2**20 and (q == np.rint(q)).all() and (q < 2**43).all()
    cs = np.concatenate([np.zeros((1,) + h.shape[1:], np.int64), np.cumsum(q.astype(np.int64), axis=0)])
    t = np.arange(h.shape[0])
    return np.ldexp((cs[t + 1] - cs[np.maximum(t - window + 1, 0)]).astype(np.float64), -33)


def direct(x, m, window=84, hmin=1.0, spw=7.0, lev=(4.0, 8.0), grp=None, G=1, integers=False):
    """The definition on the whole field ``x [T, C]``: ``dhw``, ``alert`` and the per-(group, cell) variables.  The window
    sums by ``math.fsum``, or -- ``integers`` -- by :func:`window_sums_int`."""
    x, m, lev = np.asarray(x, F), np.asarray(m, F), np.asarray(lev, F).reshape(-1)
    T, C = x.shape
    L = lev.size
    d, valid, h = hotspot(x, m, hmin)
    dhw = np.full((T, C), np.nan, F)
    if integers:
        dhw = np.where(np.isfinite(m)[None, :], (window_sums_int(h, window) / np.float64(spw)).astype(F), F(np.nan))
    for c in range(C):
        if integers or not np.isfinite(m[c]):
            continue
        col = [float(v) for v in h[:, c]]
        for t in range(T):
            dhw[t, c] = F(math.fsum(col[max(0, t - window + 1):t + 1]) / float(spw))
    alert = alert_class(d, valid, dhw, hmin, lev)
    out = new_state(C, G, L)
    del out["S"], out["status"]
    lab = np.zeros(T, np.int64) if grp is None else np.asarray(grp)
    for g in range(G):
        ts = np.flatnonzero(lab == g)
        if ts.size == 0:
            continue
        w, dd, ok, al, mok = dhw[ts], d[ts], valid[ts], alert[ts], np.isfinite(m)  # the group's steps, all cells at once
        with np.errstate(invalid="ignore"):
            out["dhw_max"][g] = np.where(mok, w.max(axis=0), F(np.nan))  # a cell with m has no NaN in w
            out["tmax"][g] = np.where(mok, ts[np.argmax(np.where(mok[None, :], w, F(0)), axis=0)], -1)  # argmax: the first
            out["hotspot_max"][g] = np.where(ok.any(axis=0), np.where(ok, dd, F(-np.inf)).max(axis=0), F(np.nan))
            out["invalid"][g] = (al == 255).sum(axis=0)
            for q in range(3 + L):
                out["alert_steps"][g, q] = (al == q).sum(axis=0)
            for j in range(L):
                hit = w >= lev[j]
                out["onset"][g, j] = np.where(hit.any(axis=0), ts[np.argmax(hit, axis=0)], -1)
    out.update(dhw=dhw, alert=alert)
    return out


SUMMARY = ("dhw_max", "tmax", "hotspot_max", "alert_steps", "invalid", "onset")


def group_walk(x, t0, lab, G, state=None):
    """The rows ``t0 ..`` of ``x [Tb, C]`` under the labels ``lab [T]`` (-1: skipped): ``sum`` float64 and ``cnt`` uint32
    ``[G, C]``, one addition per finite sample in ascending step."""
    x = np.asarray(x, F)
    C = x.shape[1]
    st = {"sum": np.zeros((G, C), np.float64), "cnt": np.zeros((G, C), np.uint32), "status": 0} if state is None else state
    for r in range(x.shape[0]):
        g = int(lab[t0 + r])
        if g == -1:
            continue
        if not 0 <= g < G:
            st["status"] += C
            continue
        ok = np.isfinite(x[r])
        st["sum"][g][ok] += x[r][ok].astype(np.float64)
        st["cnt"][g] += ok
    return st


def group_direct_counts(x, lab, G):
    x, lab = np.asarray(x, F), np.asarray(lab)
    return np.stack([np.isfinite(x[lab == g]).sum(axis=0) for g in range(G)]).astype(np.uint32)


def climatology(total, cnt):
    """``(monthly_mean, mmm, mmm_month)`` from the sums and counts, cell by cell."""
    G, C = total.shape
    mean = np.full((G, C), np.nan)
    mmm, month = np.full(C, np.nan, F), np.zeros(C, np.uint8)
    for c in range(C):
        best = None
        for g in range(G):
            if cnt[g, c]:
                mean[g, c] = total[g, c] / float(cnt[g, c])
                if best is None or mean[g, c] > mean[best, c]:
                    best = g
        if best is not None:
            mmm[c], month[c] = F(mean[best, c]), best + 1
    return mean, mmm, month
