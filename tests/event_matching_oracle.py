"""A NumPy oracle of ``marex_amd.event_matching``, written from its definitions: a plain loop over the steps, ``np.unique``
over the stacked (a, b) of the present cells, Python integers for every area and plain loops over dictionaries for everything
that is derived.  Not collected by pytest."""
import math

import numpy as np


def step_records(a, b, q=None, t0=0):
    """The records of ``a`` and ``b`` ``[T, C]``, sorted by (a, b, t): dicts of ``t`` (``t0`` + row), ``a``, ``b`` (0: the
    other field holds no event there), ``cells`` and ``area`` (a Python integer: the sum of ``q``, or the cells)."""
    a, b = np.asarray(a), np.asarray(b)
    assert a.shape == b.shape and a.ndim == 2
    out = []
    for t in range(a.shape[0]):
        ra, rb = np.maximum(a[t].astype(np.int64), 0), np.maximum(b[t].astype(np.int64), 0)
        cells = np.flatnonzero((ra > 0) | (rb > 0))
        if not cells.size:
            continue
        for i, j in np.unique(np.stack([ra[cells], rb[cells]], axis=1), axis=0):
            sel = cells[(ra[cells] == i) & (rb[cells] == j)]
            out.append({"t": t0 + t, "a": int(i), "b": int(j), "cells": int(sel.size),
                        "area": int(sel.size) if q is None else sum(int(q[c]) for c in sel)})
    out.sort(key=lambda d: (d["a"], d["b"], d["t"]))
    return out


def as_arrays(recs):
    """The records in the arrays that ``HotPath.event_matching`` returns."""
    def col(k, dt):
        return np.array([d[k] for d in recs], dt).reshape(len(recs))

    return {"t": col("t", np.int64), "a": col("a", np.int32), "b": col("b", np.int32), "cells": col("cells", np.int64),
            "area": col("area", np.int64)}


def _ratio(num, den):
    """One division of two integers, each converted once."""
    return float(num) / float(den) if den != 0 else np.nan


def matching(a, b, cell_areas=None, min_share=0.0, per_timestep=False, tv=None, n_a=None, n_b=None):
    """``({name: array}, coords)`` of the Dataset of ``marex_amd.event_matching`` for ``a`` and ``b`` ``[T, C]`` and flat
    ``cell_areas``."""
    from marex_amd.regional import area_weight_table

    a, b = np.asarray(a), np.asarray(b)
    T, C = a.shape
    tv = np.arange(T) if tv is None else np.asarray(tv)
    e, q = 0, None
    if cell_areas is not None and C:
        e, q = area_weight_table(np.asarray(cell_areas, np.float64).reshape(-1))
    recs = step_records(a, b, q) if T and C else []
    Na = max([d["a"] for d in recs], default=0) if n_a is None else n_a
    Nb = max([d["b"] for d in recs], default=0) if n_b is None else n_b

    def area(S):  # an exact integer -> float64, rounded once, scaled by a power of two
        return math.ldexp(float(S), -e)

    def whole(key, N):  # per event of one field: area-steps, cell-steps, the steps it lives at, the uncovered area-steps
        other = "b" if key == "a" else "a"
        tot, cs, only = [0] * (N + 1), [0] * (N + 1), [0] * (N + 1)
        at = [set() for _ in range(N + 1)]
        for d in recs:
            i = d[key]
            if i > 0:
                tot[i] += d["area"]
                cs[i] += d["cells"]
                at[i].add(d["t"])
                if d[other] == 0:
                    only[i] += d["area"]
        return tot, cs, at, only

    A = whole("a", Na)
    B = whole("b", Nb)
    pairs = {}
    for d in recs:
        if d["a"] > 0 and d["b"] > 0:
            pairs.setdefault((d["a"], d["b"]), []).append(d)  # ascending time
    keys = sorted(pairs)
    P = len(keys)
    names = ("pair_ID_a", "pair_ID_b", "pair_steps", "pair_time_start", "pair_time_end", "pair_cell_steps", "pair_area_steps",
             "pair_cells_max", "pair_area_max", "pair_time_of_max_area", "pair_share_of_a", "pair_share_of_b", "pair_iou",
             "pair_onset_lag", "pair_end_lag")
    o = {k: [] for k in names}
    rec_cols = {"record_time": [], "record_cells": [], "record_area": []}
    offsets = [0]
    overlap = {}
    for i, j in keys:
        ds = pairs[(i, j)]
        O = sum(d["area"] for d in ds)
        amax = max(d["area"] for d in ds)
        overlap[(i, j)] = O
        o["pair_ID_a"].append(i), o["pair_ID_b"].append(j), o["pair_steps"].append(len(ds))
        o["pair_time_start"].append(tv[ds[0]["t"]]), o["pair_time_end"].append(tv[ds[-1]["t"]])
        o["pair_cell_steps"].append(sum(d["cells"] for d in ds)), o["pair_area_steps"].append(area(O))
        o["pair_cells_max"].append(max(d["cells"] for d in ds)), o["pair_area_max"].append(area(amax))
        o["pair_time_of_max_area"].append(tv[next(d["t"] for d in ds if d["area"] == amax)])
        o["pair_share_of_a"].append(_ratio(O, A[0][i])), o["pair_share_of_b"].append(_ratio(O, B[0][j]))
        o["pair_iou"].append(_ratio(O, A[0][i] + B[0][j] - O))
        o["pair_onset_lag"].append(min(B[2][j]) - min(A[2][i])), o["pair_end_lag"].append(max(B[2][j]) - max(A[2][i]))
        for d in ds:
            rec_cols["record_time"].append(tv[d["t"]]), rec_cols["record_cells"].append(d["cells"])
            rec_cols["record_area"].append(area(d["area"]))
        offsets.append(offsets[-1] + len(ds))
    i64, f64 = np.int64, np.float64
    types = {"pair_ID_a": i64, "pair_ID_b": i64, "pair_steps": i64, "pair_time_start": tv.dtype, "pair_time_end": tv.dtype,
             "pair_cell_steps": i64, "pair_area_steps": f64, "pair_cells_max": i64, "pair_area_max": f64,
             "pair_time_of_max_area": tv.dtype, "pair_share_of_a": f64, "pair_share_of_b": f64, "pair_iou": f64,
             "pair_onset_lag": i64, "pair_end_lag": i64, "record_time": tv.dtype, "record_cells": i64, "record_area": f64}
    out = {k: np.array(v, types[k]).reshape(P) for k, v in o.items()}
    counts = {}
    for name, W, N, pos in (("a", A, Na, 0), ("b", B, Nb, 1)):
        tot, cs, at, only = W
        matches, best, best_share, m_share = [], [], [], []
        n_ev = n_matched = 0
        for i in range(1, N + 1):
            mine = sorted((k[1 - pos], overlap[k]) for k in keys if k[pos] == i)  # ascending partner
            matches.append(len(mine))
            top = max((area(v) for _, v in mine), default=0.0)
            first = next(((p_, v) for p_, v in mine if area(v) == top), (0, 0))  # the smaller ID wins a tie
            best.append(first[0])
            has = cs[i] > 0
            best_share.append(_ratio(first[1], tot[i]) if has else np.nan)
            share = _ratio(tot[i] - only[i], tot[i]) if has else np.nan
            m_share.append(share)
            n_ev += has
            n_matched += bool(has and share > 0 and share >= min_share)
        out[name + "_steps"] = np.array([len(s) for s in at[1:]], i64).reshape(N)
        out[name + "_cell_steps"] = np.array(cs[1:], i64).reshape(N)
        out[name + "_area_steps"] = np.array([area(v) for v in tot[1:]], f64).reshape(N)
        out[name + "_matches"] = np.array(matches, i64).reshape(N)
        out[name + "_best_match"] = np.array(best, i64).reshape(N)
        out[name + "_best_share"] = np.array(best_share, f64).reshape(N)
        out[name + "_matched_share"] = np.array(m_share, f64).reshape(N)
        counts[name] = (n_ev, n_matched)
    (na, ma), (nb, mb) = counts["a"], counts["b"]
    out.update(n_a=i64(na), n_b=i64(nb), matched_a=i64(ma), matched_b=i64(mb),
               pod=f64(ma / na if na else np.nan), far=f64(1.0 - (mb / nb if nb else np.nan)),
               csi=f64(ma / (na + nb - mb) if na + nb - mb else np.nan))
    for name, test in (("both", lambda d: d["a"] > 0 and d["b"] > 0), ("only_a", lambda d: d["b"] == 0),
                       ("only_b", lambda d: d["a"] == 0)):
        sel = [d for d in recs if test(d)]
        out["cell_steps_" + name] = i64(sum(d["cells"] for d in sel))
        out["area_steps_" + name] = f64(area(sum(d["area"] for d in sel)))
        per = np.zeros(T, i64)
        for d in sel:
            per[d["t"]] += d["cells"]
        out["step_cells_" + name] = per
    if per_timestep:
        out["pair_record_offsets"] = np.array(offsets, i64)
        for k, v in rec_cols.items():
            out[k] = np.array(v, types[k]).reshape(offsets[-1])
    return out, {"ID_a": np.arange(1, Na + 1), "ID_b": np.arange(1, Nb + 1), "time": tv}
