"""A NumPy oracle of ``marex_amd.event_exposure``, written from its definitions: a plain loop over the steps, ``np.unique``
over the (id, rank) of the event cells, Python integers for the areas and ``math.fsum`` for the two float sums of a record.
Not collected by pytest."""
import math

import numpy as np

U = 2.0 ** -53
F = np.float32


def _better(a, best):
    """``a`` above ``best`` in the order of the device key: by value, -0 below +0."""
    if best is None or a > best:
        return True
    return a == best and math.copysign(1.0, best) < 0 < math.copysign(1.0, a)


def step_records(ids, rank, R, q=None, wf=None, anom=None, t0=0):
    """The records of ``ids [T, C]``, sorted by (id, rank, t): dicts of ``t`` (``t0`` + row), ``rank`` (``R``: no region),
    ``id``, ``cells``, ``finite``, ``area`` (a Python integer: the sum of ``q``, or the cells), ``sw`` / ``swa`` (the exactly
    rounded sums of w and w a over the cells with a finite anomaly), ``abs`` (the same of \\|w a\\|) and ``vmax`` (None: no
    finite cell)."""
    ids, rank = np.asarray(ids), np.asarray(rank)
    T, C = ids.shape
    rk = np.where((rank >= 0) & (rank < R), rank, R).astype(np.int64)
    out = []
    for t in range(T):
        row = ids[t].astype(np.int64)
        cells = np.flatnonzero(row > 0)
        if not cells.size:
            continue
        pairs = np.unique(np.stack([row[cells], rk[cells]], axis=1), axis=0)
        for i, r in pairs:
            sel = cells[(row[cells] == i) & (rk[cells] == r)]
            rec = {"t": t0 + t, "rank": int(r), "id": int(i), "cells": int(sel.size), "finite": int(sel.size),
                   "area": int(sel.size) if q is None else sum(int(q[c]) for c in sel), "sw": 0.0, "swa": 0.0, "abs": 0.0,
                   "vmax": None}
            if anom is not None:
                a = anom[t, sel]
                ok = np.isfinite(a)
                w = np.ones(sel.size, F) if wf is None else np.asarray(wf, F)[sel]
                terms = [float(np.float64(wc) * np.float64(ac)) for wc, ac in zip(w[ok], a[ok])]  # exact products
                rec.update(finite=int(ok.sum()), sw=math.fsum(float(v) for v in w[ok]), swa=math.fsum(terms),
                           abs=math.fsum(abs(v) for v in terms))
                for v in a[ok]:
                    if _better(float(v), rec["vmax"]):
                        rec["vmax"] = float(v)
            out.append(rec)
    out.sort(key=lambda d: (d["id"], d["rank"], d["t"]))
    return out


def as_arrays(recs, anomalies):
    """The records in the arrays that ``HotPath.event_exposure`` returns."""
    def col(k, dt):
        return np.array([d[k] for d in recs], dt).reshape(len(recs))

    out = {"t": col("t", np.int64), "rank": col("rank", np.int32), "id": col("id", np.int32), "cells": col("cells", np.int64),
           "finite": col("finite", np.int64), "area": col("area", np.int64), "sums": None, "vmax": None}
    if anomalies:
        out["sums"] = np.array([[d["sw"], d["swa"]] for d in recs], np.float64).reshape(len(recs), 2)
        out["vmax"] = np.array([np.nan if d["vmax"] is None else d["vmax"] for d in recs], F).reshape(len(recs))
    return out


def ranks(regions, mask=None):
    r = np.asarray(regions).reshape(-1).astype(np.int64)
    rvals = np.unique(r[r >= 0])
    rank = np.where(r >= 0, np.searchsorted(rvals, r), -1).astype(np.int32)
    if mask is not None:
        rank = np.where(np.asarray(mask).reshape(-1) != 0, rank, -1).astype(np.int32)
    return rvals, rank


def _ratio(a, b):
    return a / b if b != 0 else np.nan


def exposure(ids, regions, cell_areas=None, anom=None, mask=None, per_timestep=False, tv=None, n_events=None):
    """``{name: array}`` of the Dataset of ``marex_amd.event_exposure`` for ``ids [T, C]`` and flat ``regions``,
    ``cell_areas`` and ``mask``."""
    from marex_amd.regional import area_weight_table

    ids = np.asarray(ids)
    T, C = ids.shape
    tv = np.arange(T) if tv is None else np.asarray(tv)
    rvals, rank = ranks(regions, mask)
    R = rvals.size
    e, q, wf = 0, None, None
    if cell_areas is not None:
        e, q = area_weight_table(np.asarray(cell_areas, np.float64).reshape(-1))
        wf = np.asarray(cell_areas).reshape(-1).astype(F)
    an = anom is not None
    recs = step_records(ids, rank, R, q, wf if an else None, None if anom is None else np.asarray(anom, F).reshape(T, C)) if R else []
    N = max([d["id"] for d in recs], default=0) if n_events is None else n_events

    def area(S):  # an exact integer -> float64, rounded once, scaled by a power of two
        return math.ldexp(float(S), -e)

    ev_total, ev_out = [0] * (N + 1), [0] * (N + 1)
    for d in recs:
        ev_total[d["id"]] += d["area"]
        if d["rank"] == R:
            ev_out[d["id"]] += d["area"]
    pairs = {}
    for d in recs:
        if d["rank"] < R:
            pairs.setdefault((d["id"], d["rank"]), []).append(d)  # ascending time
    keys = sorted(pairs)
    P = len(keys)
    region_cells = [int(((rank == r)).sum()) for r in range(R)]
    region_q = [region_cells[r] if q is None else sum(int(v) for v in q[rank == r]) for r in range(R)]
    o = {k: [] for k in ("pair_ID", "pair_region", "pair_steps", "pair_time_start", "pair_time_end", "pair_cell_steps",
                         "pair_area_steps", "pair_cells_max", "pair_area_max", "pair_time_of_max_area", "pair_share_of_event",
                         "pair_region_share_max")}
    if an:
        o.update({k: [] for k in ("pair_intensity_max", "pair_time_of_intensity_max", "pair_intensity_integral",
                                  "pair_intensity_mean", "pair_invalid_cells")})
    rec_cols = {k: [] for k in ("record_time", "record_cells", "record_area", "record_intensity_max", "record_intensity_integral",
                                "record_intensity_mean", "record_invalid_cells")}
    offsets = [0]
    best = {}
    t_none = []
    for i, r in keys:
        ds = pairs[(i, r)]
        total = sum(d["area"] for d in ds)
        amax = max(d["area"] for d in ds)
        o["pair_ID"].append(i), o["pair_region"].append(int(rvals[r])), o["pair_steps"].append(len(ds))
        o["pair_time_start"].append(tv[ds[0]["t"]]), o["pair_time_end"].append(tv[ds[-1]["t"]])
        o["pair_cell_steps"].append(sum(d["cells"] for d in ds)), o["pair_area_steps"].append(area(total))
        o["pair_cells_max"].append(max(d["cells"] for d in ds)), o["pair_area_max"].append(area(amax))
        o["pair_time_of_max_area"].append(tv[next(d["t"] for d in ds if d["area"] == amax)])
        o["pair_share_of_event"].append(_ratio(float(total), float(ev_total[i])))
        o["pair_region_share_max"].append(_ratio(area(amax), area(region_q[r])))
        if i not in best or area(total) > best[i][0]:  # ascending region: the smallest wins a tie
            best[i] = (area(total), int(rvals[r]))
        if an:
            vm = None
            for d in ds:
                if d["vmax"] is not None and _better(d["vmax"], vm):
                    vm, tm = d["vmax"], d["t"]
            w = sa = 0.0
            for d in ds:  # one record after the other in ascending time
                w, sa = w + d["sw"], sa + d["swa"]
            fin = sum(d["finite"] for d in ds)
            o["pair_intensity_max"].append(np.nan if vm is None else vm)
            t_none.append(vm is None)
            o["pair_time_of_intensity_max"].append(tv[0 if vm is None else tm])
            o["pair_intensity_integral"].append(sa)
            o["pair_intensity_mean"].append(sa / w if fin and w != 0 else np.nan)
            o["pair_invalid_cells"].append(sum(d["cells"] - d["finite"] for d in ds))
        for d in ds:
            rec_cols["record_time"].append(tv[d["t"]]), rec_cols["record_cells"].append(d["cells"])
            rec_cols["record_area"].append(area(d["area"]))
            rec_cols["record_intensity_max"].append(np.nan if d["vmax"] is None else d["vmax"])
            rec_cols["record_intensity_integral"].append(d["swa"])
            rec_cols["record_intensity_mean"].append(d["swa"] / d["sw"] if d["finite"] and d["sw"] != 0 else np.nan)
            rec_cols["record_invalid_cells"].append(d["cells"] - d["finite"])
        offsets.append(offsets[-1] + len(ds))
    i64, f64 = np.int64, np.float64
    types = {"pair_ID": i64, "pair_region": i64, "pair_steps": i64, "pair_time_start": tv.dtype, "pair_time_end": tv.dtype,
             "pair_cell_steps": i64, "pair_area_steps": f64, "pair_cells_max": i64, "pair_area_max": f64,
             "pair_time_of_max_area": tv.dtype, "pair_share_of_event": f64, "pair_region_share_max": f64,
             "pair_intensity_max": F, "pair_time_of_intensity_max": tv.dtype, "pair_intensity_integral": f64,
             "pair_intensity_mean": f64, "pair_invalid_cells": i64, "record_time": tv.dtype, "record_cells": i64,
             "record_area": f64, "record_intensity_max": F, "record_intensity_integral": f64, "record_intensity_mean": f64,
             "record_invalid_cells": i64}
    out = {k: np.array(v, types[k]).reshape(P) for k, v in o.items()}
    if an and any(t_none):  # a missing time: NaT for dates, NaN (and a float axis) otherwise
        tm = out["pair_time_of_intensity_max"]
        if tm.dtype.kind in "mM":
            tm[np.array(t_none)] = np.array("NaT", tm.dtype)
        else:
            tm = tm.astype(f64)
            tm[np.array(t_none)] = np.nan
        out["pair_time_of_intensity_max"] = tm
    has = [False] * (N + 1)
    for d in recs:
        has[d["id"]] = True
    out["event_regions"] = np.array([sum(1 for k in keys if k[0] == i) for i in range(1, N + 1)], i64).reshape(N)
    out["event_main_region"] = np.array([best[i][1] if i in best else -1 for i in range(1, N + 1)], i64).reshape(N)
    out["event_outside_share"] = np.array([_ratio(float(ev_out[i]), float(ev_total[i])) if has[i] else np.nan
                                           for i in range(1, N + 1)], f64).reshape(N)
    out["region_events"] = np.array([sum(1 for k in keys if k[1] == r) for r in range(R)], i64).reshape(R)
    out["region_event_steps"] = np.array([sum(len(pairs[k]) for k in keys if k[1] == r) for r in range(R)], i64).reshape(R)
    out["region_cells"] = np.array(region_cells, i64).reshape(R)
    out["region_area"] = np.array([area(v) for v in region_q], f64).reshape(R)
    if per_timestep:
        out["pair_record_offsets"] = np.array(offsets, i64)
        n = offsets[-1]
        for k, v in rec_cols.items():
            if an or k in ("record_time", "record_cells", "record_area"):
                out[k] = np.array(v, types[k]).reshape(n)
    return out, {"ID": np.arange(1, N + 1), "region": rvals}
