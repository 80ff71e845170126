"""NumPy restatements of ``marex_amd.cell_events`` (not collected by pytest).

``spans`` / ``direct_*``: the definition itself, per cell -- label the runs, drop the short ones, join the qualifying runs
at most ``gap`` steps apart, slice the span.  ``walk`` / ``finish``: the row loop of the state machine the device runs,
with its two accumulators per cell and their order of summation, carried across windows in ``state``."""
import math

import numpy as np


# ------------------------------------------------------------------ the direct definition
def spans(col, D, gap):
    """``[(start, end)]`` of the events of one cell."""
    p = (np.asarray(col) > 0).astype(np.int8)
    d = np.diff(np.concatenate(([0], p, [0])))
    starts, ends = np.flatnonzero(d == 1), np.flatnonzero(d == -1) - 1
    ev = []
    for s, e in zip(starts.tolist(), ends.tolist()):
        if e - s + 1 < D:
            continue  # never a bridge
        if ev and s - ev[-1][1] - 1 <= gap:
            ev[-1][1] = e
        else:
            ev.append([s, e])
    return [(s, e) for s, e in ev]


def direct_mask(x, D, gap):
    m = np.zeros(x.shape, bool)
    for c in range(x.shape[1]):
        for s, e in spans(x[:, c], D, gap):
            m[s:e + 1, c] = True
    return m


def direct_records(x, a, D, gap):
    """Per event, by cell then start: cell, start, end and, with ``a``, the finite steps' ``np.max``, the earliest step that
    attains it (-1 for none), ``np.sum`` in float64, ``math.fsum``, ``sum |a|`` and the non-finite steps."""
    out = {k: [] for k in ("cell", "start", "end", "vmax", "tmax", "sum", "fsum", "abs", "invalid")}
    for c in range(x.shape[1]):
        for s, e in spans(x[:, c], D, gap):
            out["cell"].append(c), out["start"].append(s), out["end"].append(e)
            if a is None:
                continue
            v = a[s:e + 1, c]
            ok = np.isfinite(v)
            f = v[ok].astype(np.float64)
            out["invalid"].append(int((~ok).sum()))
            out["sum"].append(float(np.sum(f)) if f.size else 0.0)
            out["fsum"].append(math.fsum(f.tolist()))
            out["abs"].append(math.fsum(np.abs(f).tolist()))
            if f.size:
                m = np.max(v[ok])
                hit = np.flatnonzero(ok & (v == m))
                if m == 0:  # +0 lies above -0
                    pos = np.flatnonzero(ok & (v == 0) & ~np.signbit(v))
                    hit, m = (pos, np.float32(0.0)) if pos.size else (hit, m)
                out["vmax"].append(np.float32(m)), out["tmax"].append(s + int(hit[0]))
            else:
                out["vmax"].append(np.float32(np.nan)), out["tmax"].append(-1)
    dt = dict(cell=np.int64, start=np.int32, end=np.int32, vmax=np.float32, tmax=np.int32, sum=np.float64, fsum=np.float64,
              abs=np.float64, invalid=np.uint32)
    return {k: np.asarray(v, dt[k]) for k, v in out.items() if a is not None or k in ("cell", "start", "end")}


def direct_summary(x, a, D, gap, grp=None, G=1):
    """``events``, ``event_days``, ``duration_max`` uint32 ``[G, C]`` by the group of the start step and, with ``a``,
    ``sum`` (the events' ``np.sum``, added in time order), ``vmax`` (NaN: none) and ``invalid``."""
    C = x.shape[1]
    r = direct_records(x, a, D, gap)
    out = {"events": np.zeros((G, C), np.uint32), "event_days": np.zeros((G, C), np.uint32), "duration_max": np.zeros((G, C), np.uint32)}
    if a is not None:
        out.update(sum=np.zeros((G, C)), vmax=np.full((G, C), np.nan, np.float32), invalid=np.zeros((G, C), np.uint32))
    for k in range(r["cell"].size):
        c, s, e = int(r["cell"][k]), int(r["start"][k]), int(r["end"][k])
        g = 0 if grp is None else int(grp[s])
        out["events"][g, c] += 1
        out["event_days"][g, c] += e - s + 1
        out["duration_max"][g, c] = max(out["duration_max"][g, c], e - s + 1)
        if a is not None:
            out["sum"][g, c] += r["sum"][k]
            out["invalid"][g, c] += r["invalid"][k]
            if not np.isnan(r["vmax"][k]) and not out["vmax"][g, c] >= r["vmax"][k]:
                out["vmax"][g, c] = r["vmax"][k]
    return out


# ------------------------------------------------------------------ the state machine, row by row
def key(a):
    """The ordered key of a float32: ascending with the value, +0 above -0; 0 is no value."""
    b = np.ascontiguousarray(a, np.float32).view(np.uint32)
    return np.where(b & np.uint32(0x80000000), ~b, b | np.uint32(0x80000000)).astype(np.uint32)


def unkey(k):
    k = np.asarray(k, np.uint32)
    b = np.where(k & np.uint32(0x80000000), k & np.uint32(0x7FFFFFFF), ~k).astype(np.uint32).view(np.float32)
    return np.where(k != 0, b, np.float32(np.nan)).astype(np.float32)


def new_state(C, G, anomalies):
    z = lambda dt, *s: np.zeros(s or (C,), dt)  # noqa: E731
    return {"run": z(np.int64), "st1": z(np.int64), "end": z(np.int64), "es": z(np.float64), "emax": z(np.uint32), "etm": z(np.int64),
            "einv": z(np.uint32), "ts": z(np.float64), "tmx": z(np.uint32), "ttm": z(np.int64), "tinv": z(np.uint32),
            "events": z(np.uint32, G, C), "event_days": z(np.uint32, G, C), "duration_max": z(np.uint32, G, C),
            "sum": z(np.float64, G, C), "vmax": z(np.uint32, G, C), "invalid": z(np.uint32, G, C), "status": [0, 0], "rec": [],
            "anomalies": anomalies, "G": G}


def _emit(st, sel, grp):
    for c in np.flatnonzero(sel).tolist():
        s, e = int(st["st1"][c]) - 1, int(st["end"][c])
        st["st1"][c] = 0
        g = 0 if grp is None else int(grp[s])
        if g < 0 or g >= st["G"]:
            st["status"][0] += 1
            continue
        st["events"][g, c] += 1
        st["event_days"][g, c] += e - s + 1
        st["duration_max"][g, c] = max(int(st["duration_max"][g, c]), e - s + 1)
        st["sum"][g, c] += st["es"][c]
        st["vmax"][g, c] = max(st["vmax"][g, c], st["emax"][c])
        st["invalid"][g, c] += st["einv"][c]
        st["rec"].append((c, s, e, int(st["emax"][c]), int(st["etm"][c]), float(st["es"][c]), int(st["einv"][c])))


def walk(x, a=None, t0=0, D=5, gap=2, grp=None, G=1, mask=None, finish=True, state=None):
    """The rows ``t0 .. t0 + Tb - 1``: ``x`` ``[Tb, C]``, ``a`` float32 ``[Tb, C]`` or None, ``grp`` by the global step,
    ``mask`` the whole bool / uint8 ``[T, C]`` output or None.  Returns the state."""
    x = np.asarray(x)
    Tb, C = x.shape
    st = new_state(C, G, a is not None) if state is None else state
    run, st1, end = st["run"], st["st1"], st["end"]
    for r in range(Tb):
        t = t0 + r
        p = x[r] > 0
        av = np.zeros(C, np.float32) if a is None else np.asarray(a[r], np.float32)
        fin, k = np.isfinite(av), key(av)
        run[:] = np.where(p, run + 1, 0)
        gap_open = ~p & (st1 > 0)
        close = gap_open & (t - end > gap)
        _emit(st, close, grp)
        short = p & (run <= D)
        restart = short & (run == 1) & (st1 == 0)  # a run starts with no event open: the tail restarts
        st["ts"][restart], st["tmx"][restart], st["ttm"][restart], st["tinv"][restart] = 0.0, 0, 0, 0
        straight = p & (run > D)  # a step of a qualified run goes to the event
        sf = straight & fin
        st["es"][sf] += av[sf].astype(np.float64)
        up = sf & (k > st["emax"])
        st["emax"][up], st["etm"][up] = k[up], t
        st["einv"][straight & ~fin] += 1
        end[straight] = t
        tail = short | (gap_open & ~close)
        tf = tail & fin
        st["ts"][tf] += av[tf].astype(np.float64)
        up = tf & (k > st["tmx"])
        st["tmx"][up], st["ttm"][up] = k[up], t
        st["tinv"][tail & ~fin] += 1
        qual = p & (run == D)  # the run qualifies: it opens an event or joins the open one
        if mask is not None:
            for c in np.flatnonzero(qual).tolist():
                mask[(int(end[c]) + 1 if st1[c] else t - D + 1):t, c] = 1
        fresh = qual & (st1 == 0)
        st1[fresh] = t - D + 2
        st["es"][fresh], st["emax"][fresh], st["etm"][fresh], st["einv"][fresh] = 0.0, 0, 0, 0
        st["es"][qual] = st["es"][qual] + st["ts"][qual]  # the tail joins as one term
        up = qual & (st["tmx"] > st["emax"])
        st["emax"][up], st["etm"][up] = st["tmx"][up], st["ttm"][up]
        st["einv"][qual] += st["tinv"][qual]
        st["ts"][qual], st["tmx"][qual], st["ttm"][qual], st["tinv"][qual] = 0.0, 0, 0, 0
        end[qual] = t
        if mask is not None:
            mask[t] = p & (run >= D)
    if finish:
        _emit(st, st1 > 0, grp)
    return st


def finish(st):
    """The outputs of a finished walk: the ``[G, C]`` accumulators and ``rec``, the records by cell, then start."""
    C = st["run"].size
    out = {k: st[k].copy() for k in ("events", "event_days", "duration_max")}
    rec = sorted(st["rec"], key=lambda v: (v[0], v[1]))
    cols = list(zip(*rec)) if rec else [[]] * 7
    cell = np.asarray(cols[0], np.int64)
    r = {"off": np.concatenate(([0], np.cumsum(np.bincount(cell, minlength=C)))).astype(np.int64), "cell": cell,
         "start": np.asarray(cols[1], np.int32), "end": np.asarray(cols[2], np.int32)}
    if st["anomalies"]:
        out.update(sum=st["sum"].copy(), vmax=unkey(st["vmax"]), invalid=st["invalid"].copy())
        ek = np.asarray(cols[3], np.uint32)
        r.update(vmax=unkey(ek), tmax=np.where(ek != 0, np.asarray(cols[4], np.int32), np.int32(-1)).astype(np.int32),
                 sum=np.asarray(cols[5], np.float64), invalid=np.asarray(cols[6], np.uint32))
    out["rec"] = r
    return out


def rates(rec, a, T):
    """``(rate_onset, rate_decline)`` of the records, one at a time in Python floats."""
    on, off = [], []
    for c, s, e, peak, tm in zip(rec["cell"].tolist(), rec["start"].tolist(), rec["end"].tolist(), rec["vmax"].tolist(), rec["tmax"].tolist()):
        col = [float(v) for v in a[:, c]]
        ops_on = [peak, col[s]] + ([col[s - 1]] if s > 0 else [])
        ops_off = [peak, col[e]] + ([col[e + 1]] if e < T - 1 else [])
        if not all(math.isfinite(v) for v in ops_on):
            on.append(math.nan)
        elif s > 0:
            on.append((peak - 0.5 * (col[s - 1] + col[s])) / (tm - s + 0.5))
        else:
            on.append((peak - col[s]) / max(tm - s, 1))
        if not all(math.isfinite(v) for v in ops_off):
            off.append(math.nan)
        elif e < T - 1:
            off.append((peak - 0.5 * (col[e] + col[e + 1])) / (e - tm + 0.5))
        else:
            off.append((peak - col[e]) / max(e - tm, 1))
    return np.asarray(on, np.float64), np.asarray(off, np.float64)
