"""NumPy oracle of the regional series (``marex_regional_series_u8`` / ``marex_regional_series_i32``,
``marex_amd.regional_series``): integer ``np.add.at`` for every count, Python integers for every area (no width to
overflow), float64 products added by ``np.add.at`` for the two sums -- exact, and so equal to any order of summation, on
dyadic inputs -- and ``math.fsum`` for the exact sums and the bound on anything else.  The NaN rule is the kernel's: with
anomalies ``area`` and ``cnt[0]`` count the present cells whose anomaly is finite, without anomalies all present cells; a
present cell with a NaN or infinite anomaly adds to ``cnt[1]`` alone.  Not collected by pytest."""
import math

import numpy as np

from marex_amd._keys import float_key, key_float

from local_intensity_oracle import classes, present, ratio

NCAT = 6
U = 2.0 ** -53


def new_state(T, R, anomalies=False, cats=False, areas=False):
    return {"area": np.zeros((T, R), object), "cnt": np.zeros((T, R, 2), np.int64),
            "sums": np.zeros((T, R, 2), np.float64) if anomalies else None,
            "key": np.zeros((T, R), np.uint32) if anomalies else None,
            "cat_cnt": np.zeros((T, R, NCAT), np.int64) if cats else None,
            "cat_area": np.zeros((T, R, NCAT), object) if cats and areas else None, "status": [0, 0]}


def accumulate(x, reg, R, T, t0=0, q=None, wf=None, anom=None, thr=None, doy=None, match=0, state=None):
    """The rows ``t0 .. t0 + Tb - 1`` added to ``state`` (a fresh one by default), exactly as the kernel defines it; ``doy`` is
    indexed by the global step."""
    x = np.asarray(x)
    Tb, C = x.shape
    an, cats = anom is not None, thr is not None
    s = new_state(T, R, an, cats, q is not None) if state is None else state
    reg = np.asarray(reg).astype(np.int64)
    inside = (reg >= 0) & (reg < R)
    qq = np.ones(C, object) if q is None else np.asarray(q).astype(object)
    w64 = np.ones(C) if wf is None else np.asarray(wf, np.float32).astype(np.float64)
    s["status"][0] += int((x.astype(np.int64) < 0).sum()) if x.dtype != bool else 0
    p_all = present(x, match) & inside[None, :]
    for r in range(Tb):
        t = t0 + r
        p = p_all[r]
        if cats and not 0 <= int(doy[t]) < np.asarray(thr).shape[0]:
            s["status"][1] += int(p.sum())  # the step addresses nothing
            continue
        if not an:
            np.add.at(s["cnt"][t, :, 0], reg[p], 1)
            np.add.at(s["area"][t], reg[p], qq[p])
            continue
        a = np.asarray(anom, np.float32)[r]
        ok = p & np.isfinite(a)
        np.add.at(s["cnt"][t, :, 0], reg[ok], 1)
        np.add.at(s["cnt"][t, :, 1], reg[p & ~ok], 1)
        np.add.at(s["area"][t], reg[ok], qq[ok])
        np.add.at(s["sums"][t, :, 0], reg[ok], w64[ok])
        np.add.at(s["sums"][t, :, 1], reg[ok], w64[ok] * a[ok].astype(np.float64))
        np.maximum.at(s["key"][t], reg[ok], float_key(a)[ok])
        if cats:
            c = classes(a, np.asarray(thr, np.float32)[int(doy[t])])
            np.add.at(s["cat_cnt"][t], (reg[ok], c[ok]), 1)
            if s["cat_area"] is not None:
                np.add.at(s["cat_area"][t], (reg[ok], c[ok]), qq[ok])
    return s


def finish(s):
    """The host view of a state, as ``HotPath.regional_series`` returns it: int64 areas (every sum fits: asserted) and
    ``vmax`` float32 with NaN for none."""
    out = {"cnt": s["cnt"], "sums": s["sums"], "cat_cnt": s["cat_cnt"], "status": s["status"]}
    for k in ("area", "cat_area"):
        v = s[k]
        if v is not None:
            assert all(0 <= int(e) < 2**63 for e in v.reshape(-1))
            v = v.astype(np.int64)
        out[k] = v
    out["vmax"] = None if s["key"] is None else \
        np.where(s["key"] != 0, key_float(s["key"]), np.float32(np.nan)).astype(np.float32)
    return out


def exact_sums(x, reg, R, wf, anom, match=0):
    """Per slot ``(fsum of w, fsum of w a, fsum of |w a|, finite cells)``: the correctly rounded sums of the exact terms."""
    x, a = np.asarray(x), np.asarray(anom, np.float32)
    T, C = x.shape
    reg = np.asarray(reg).astype(np.int64)
    w64 = np.ones(C) if wf is None else np.asarray(wf, np.float32).astype(np.float64)
    ok = present(x, match) & ((reg >= 0) & (reg < R))[None, :] & np.isfinite(a)
    W, S, A, n = np.zeros((T, R)), np.zeros((T, R)), np.zeros((T, R)), np.zeros((T, R), np.int64)
    for t in range(T):
        for r in range(R):
            sel = ok[t] & (reg == r)
            terms = (w64[sel] * a[t, sel].astype(np.float64)).tolist()  # float32 x float32 in float64: exact
            W[t, r], S[t, r], A[t, r], n[t, r] = math.fsum(w64[sel].tolist()), math.fsum(terms), math.fsum(map(abs, terms)), int(sel.sum())
    return W, S, A, n


def regional_series(x, regions=None, cell_areas=None, anom=None, thr=None, doy=None, mask=None, grp=None, G=1, match=0):
    """The variables of ``marex_amd.regional_series`` over ``[T, C]`` fields, flat in space; ``regions`` int ``[C]`` as the
    user gives them, ``thr`` ``[n_doy, C]``, ``grp`` the label of every step."""
    from marex_amd.regional import area_weight_table

    x = np.asarray(x)
    T, C = x.shape
    regions = np.zeros(C, np.int64) if regions is None else np.asarray(regions).astype(np.int64)
    rvals = np.unique(regions[regions >= 0])
    rank = np.where(regions >= 0, np.searchsorted(rvals, regions), -1)
    if mask is not None:
        rank = np.where(np.asarray(mask) != 0, rank, -1)
    R = max(rvals.size, 1)
    e, q, wf = 0, None, None
    if cell_areas is not None:
        e, q = area_weight_table(np.asarray(cell_areas).reshape(-1))
        wf = np.asarray(cell_areas, np.float32).reshape(-1)
    s = finish(accumulate(x, rank, R, T, 0, q, wf if anom is not None else None, anom, thr, doy, match))

    def to_area(S):
        return np.ldexp(np.asarray(S).astype(np.float64), -e)

    ok = rank >= 0
    region_cells = np.bincount(rank[ok], minlength=R).astype(np.int64)
    rq = np.zeros(R, np.int64)
    np.add.at(rq, rank[ok], 1 if q is None else q[ok])
    region_area = to_area(rq)
    cells = s["cnt"][..., 0]
    out = {"cells": cells, "area": to_area(s["area"]), "area_share": ratio(to_area(s["area"]), region_area[None]),
           "cells_share": ratio(cells, region_cells[None]), "region_cells": region_cells, "region_area": region_area}
    if anom is not None:
        W, SA = s["sums"][..., 0], s["sums"][..., 1]
        out["intensity_mean"] = np.where(cells > 0, ratio(SA, W), np.nan)
        out["intensity_max"] = s["vmax"]
        out["intensity_integral"] = np.where(cells > 0, SA, np.nan)
        out["invalid_cells"] = s["cnt"][..., 1]
    if thr is not None:
        ca = s["cat_cnt"] if s["cat_area"] is None else s["cat_area"]
        out["category_cells"] = s["cat_cnt"]
        out["category_area"] = to_area(ca)
        out["category_share"] = ratio(to_area(ca), region_area[None, :, None])
    if grp is not None:
        grp = np.asarray(grp)
        steps = np.bincount(grp, minlength=G).astype(np.int64)

        def by(v, dt):
            o = np.zeros((G,) + v.shape[1:], dt)
            for t in range(T):  # ascending time
                o[grp[t]] += v[t].astype(dt)
            return o

        out["steps_by"] = steps
        out["cell_steps_by"] = by(cells, np.int64)
        out["area_steps_by"] = by(out["area"], np.float64)
        out["share_by"] = ratio(out["area_steps_by"], steps[:, None] * region_area[None])
        if anom is not None:
            vm = np.full((G, R), np.nan, np.float32)
            for t in range(T):
                vm[grp[t]] = np.fmax(vm[grp[t]], s["vmax"][t])
            out["intensity_max_by"] = vm
        if thr is not None:
            out["category_cell_steps_by"] = by(s["cat_cnt"], np.int64)
            out["category_area_steps_by"] = by(out["category_area"], np.float64)
    return out
