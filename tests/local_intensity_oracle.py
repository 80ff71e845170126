"""NumPy oracle of the per-cell intensity (``marex_local_intensity_u8`` / ``marex_local_intensity_i32``,
``marex_amd.local_intensity``): a Python loop over the rows, vectorised over the cells -- the sums add one row after the
other in float64, the category compares are float32 against the three float32 products, the section counts ``np.add.at``.
Not collected by pytest."""
import numpy as np

from marex_amd.intensity import float_key, key_float

NCAT = 6


def present(x, match=0):
    x = np.asarray(x).astype(np.int64)
    return (x == match) if match else (x > 0)


def classes(a, h):
    """The class 0..5 of float32 anomalies ``a`` under float32 thresholds ``h``, by the intervals of the definition."""
    a, h = np.asarray(a, np.float32), np.asarray(h, np.float32)
    with np.errstate(over="ignore", invalid="ignore"):
        h2, h3, h4 = np.float32(2) * h, np.float32(3) * h, np.float32(4) * h
        assert h2.dtype == h3.dtype == h4.dtype == np.float32
        c = np.full(a.shape, -1, np.int64)
        c[a < h] = 0
        c[(h <= a) & (a < h2)] = 1
        c[(h2 <= a) & (a < h3)] = 2
        c[(h3 <= a) & (a < h4)] = 3
        c[a >= h4] = 4
        c[~np.isfinite(h) | (h <= 0)] = 5
    return c


def new_state(G, C, cats=False, G2=0, R=0):
    return {"days": np.zeros((G, C), np.uint32), "invalid": np.zeros((G, C), np.uint32), "sum": np.zeros((G, C), np.float64),
            "key": np.zeros((G, C), np.uint32), "tmax": np.zeros((G, C), np.int32),
            "cat_days": np.zeros((G, NCAT, C), np.uint32) if cats else None,
            "sec_cnt": np.zeros((G2, R, NCAT), np.uint64) if G2 else None, "status": [0, 0]}


def accumulate(x, anom, t0=0, grp=None, G=1, thr=None, doy=None, sgrp=None, G2=0, cls=None, R=0, match=0, state=None):
    """The rows ``t0 .. t0 + Tb - 1`` added to ``state`` (a fresh one by default), exactly as the kernel defines it; ``grp``,
    ``doy`` and ``sgrp`` are indexed by the global step.  Returns the state: ``key`` is the uint32 key of the maximum (0:
    none), ``tmax`` its earliest global step (0 where none, like the zeroed accumulator)."""
    x, anom = np.asarray(x), np.asarray(anom, np.float32)
    Tb, C = x.shape
    cats = thr is not None
    s = new_state(G, C, cats, G2 if sgrp is not None else 0, R) if state is None else state
    p_all = present(x, match)
    s["status"][0] += int((x.astype(np.int64) < 0).sum()) if x.dtype != bool else 0
    if cls is not None:
        cls = np.asarray(cls)
        in_cls = (cls >= 0) & (cls < R)
    for r in range(Tb):
        t = t0 + r
        p = p_all[r]
        g = 0 if grp is None else int(grp[t])
        d = int(doy[t]) if cats else 0
        if not 0 <= g < G or (cats and not 0 <= d < thr.shape[0]):
            s["status"][1] += int(p.sum())  # the step addresses nothing
            continue
        a = anom[r]
        ok = p & np.isfinite(a)
        s["days"][g] += ok.astype(np.uint32)
        s["invalid"][g] += (p & ~ok).astype(np.uint32)
        s["sum"][g] += np.where(ok, a.astype(np.float64), 0.0)
        key = np.where(ok, float_key(a), np.uint32(0))
        better = key > s["key"][g]
        s["key"][g] = np.where(better, key, s["key"][g])
        s["tmax"][g] = np.where(better, np.int32(t), s["tmax"][g])
        if cats:
            c = np.where(ok, classes(a, np.asarray(thr, np.float32)[d]), -1)
            for k in range(NCAT):
                s["cat_days"][g, k] += (c == k).astype(np.uint32)
            if sgrp is not None:
                sg = int(sgrp[t])
                sel = (c >= 0) & in_cls
                if 0 <= sg < G2:
                    np.add.at(s["sec_cnt"][sg], (cls[sel], c[sel]), np.uint64(1))
                else:
                    s["status"][1] += int(sel.sum())
    return s


def finish(s):
    """The host view of a state: ``vmax`` float32 (NaN: none) and ``tmax`` -1 where none."""
    has = s["key"] != 0
    out = dict(s)
    out["vmax"] = np.where(has, key_float(s["key"]), np.float32(np.nan)).astype(np.float32)
    out["tmax"] = np.where(has, s["tmax"], np.int32(-1)).astype(np.int32)
    return out


def ratio(num, den):
    num, den = np.broadcast_arrays(np.asarray(num, np.float64), np.asarray(den, np.float64))
    out = np.full(num.shape, np.nan)
    np.divide(num, den, out=out, where=den != 0)
    return out


def local_intensity(x, anom, tv=None, grp=None, G=1, thr=None, doy=None, sgrp=None, G2=0, cls=None, R=0, class_cells=None, match=0):
    """The variables of ``marex_amd.local_intensity`` over ``[T, C]`` fields, flat in space and with the group axis kept."""
    x = np.asarray(x)
    T = x.shape[0]
    s = finish(accumulate(x, anom, 0, grp, G, thr, doy, sgrp, G2, cls, R, match))
    has = s["tmax"] >= 0
    tv = np.arange(T) if tv is None else np.asarray(tv)
    if tv.dtype.kind == "M":
        tom = np.where(has, tv[np.where(has, s["tmax"], 0)], np.array("NaT", dtype=tv.dtype))
    else:
        tom = np.where(has, tv[np.where(has, s["tmax"], 0)], -1)
    out = {"days": s["days"], "invalid_steps": s["invalid"], "intensity_cumulative": s["sum"],
           "intensity_mean": ratio(s["sum"], s["days"]), "intensity_max": s["vmax"], "time_of_max": tom,
           "steps_by": np.bincount(np.asarray(grp), minlength=G).astype(np.int64) if grp is not None else np.asarray(np.int64(T))}
    if thr is not None:
        cat = s["cat_days"]
        peak = np.zeros(s["days"].shape, np.uint8)
        for g in range(cat.shape[0]):
            for c in range(cat.shape[2]):
                for k in (1, 2, 3, 4):
                    if cat[g, k, c]:
                        peak[g, c] = k
        out.update(category_days=cat, category_peak=peak)
    if sgrp is not None:
        sec = s["sec_cnt"]
        per_cat = sec.sum(axis=1)
        out.update(category_cells=sec, category_share=ratio(per_cat, per_cat.sum(axis=1)[:, None]),
                   class_cells=np.asarray(class_cells, np.int64))
    return out
