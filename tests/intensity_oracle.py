"""NumPy / plain-Python restatement of the per-event intensity metrics (``marex_amd.event_intensity``), written without the
package: a loop over (timestep, event), ``math.fsum`` for the sums (the exactly rounded sum, whatever the order), Python
floats in ascending time for the event-level finish.  Not collected by pytest."""
import math

import numpy as np


def float_key(a: float) -> int:
    """Order-preserving uint32 key of a float32 value, from its bits."""
    b = int(np.array([a], np.float32).view(np.uint32)[0])
    return (~b) & 0xFFFFFFFF if b & 0x80000000 else b | 0x80000000


def key_float(k: int) -> float:
    b = k & 0x7FFFFFFF if k & 0x80000000 else (~k) & 0xFFFFFFFF
    return float(np.array([b], np.uint32).view(np.float32)[0])


def slots(ids, anom, w=None, n_ev=None):
    """``{(t, e): (finite cells, non-finite cells, W, S, sum |w a|, max or None)}`` for every (timestep, event 1..n_ev)
    with at least one cell.  ``ids`` / ``anom``: ``[T, C]``; ``w``: float32 ``[C]`` or None."""
    ids, anom = np.asarray(ids), np.asarray(anom, np.float32)
    n_ev = int(ids.max()) if n_ev is None else n_ev
    wd = np.ones(ids.shape[1]) if w is None else np.asarray(w, np.float32).astype(np.float64)
    out = {}
    for t in range(ids.shape[0]):
        for e in np.unique(ids[t]):
            if e < 1 or e > n_ev:
                continue
            c = np.nonzero(ids[t] == e)[0]
            a = anom[t, c].astype(np.float64)
            ok = np.isfinite(a)
            terms = wd[c][ok] * a[ok]  # float32 x float32 in float64: exact
            out[(t, int(e))] = (int(ok.sum()), int((~ok).sum()), math.fsum(wd[c][ok]), math.fsum(terms),
                                math.fsum(np.abs(terms)), float(np.max(anom[t, c][ok])) if ok.any() else None)
    return out


def intensity(ids, anom, w=None, n_ev=None):
    """Every variable of the Dataset as arrays (``event_step_of_max``: the index of the timestep, -1 for none) plus
    ``abs_integral``, the sum of |w a| per slot that the error bound of the sums needs."""
    ids = np.asarray(ids).reshape(np.asarray(ids).shape[0], -1)
    anom = np.asarray(anom, np.float32).reshape(ids.shape)
    T = ids.shape[0]
    N = int(max(ids.max(), 0)) if n_ev is None else n_ev
    sl = slots(ids, anom, None if w is None else np.asarray(w).reshape(-1), N)
    r = {"intensity_max": np.full((T, N), np.nan, np.float32), "intensity_mean": np.full((T, N), np.nan, np.float32),
         "intensity_integral": np.full((T, N), np.nan, np.float64), "intensity_cells": np.zeros((T, N), np.int64),
         "abs_integral": np.zeros((T, N), np.float64),
         "event_duration": np.zeros(N, np.int32), "event_intensity_max": np.full(N, np.nan, np.float32),
         "event_step_of_max": np.full(N, -1, np.int64), "event_intensity_mean": np.full(N, np.nan, np.float32),
         "event_intensity_cumulative": np.full(N, np.nan, np.float32), "event_invalid_cells": np.zeros(N, np.int64)}
    for e in range(1, N + 1):
        sum_s = sum_w = cum = 0.0
        any_ratio = False
        best = None
        for t in range(T):
            if (t, e) not in sl:
                continue
            n, bad, W, S, A, mx = sl[(t, e)]
            r["event_duration"][e - 1] += 1
            r["event_invalid_cells"][e - 1] += bad
            if n == 0:
                continue
            r["intensity_cells"][t, e - 1] = n
            r["intensity_max"][t, e - 1] = mx
            r["intensity_integral"][t, e - 1] = S
            r["abs_integral"][t, e - 1] = A
            sum_s += S
            sum_w += W
            if W != 0:
                r["intensity_mean"][t, e - 1] = np.float32(S / W)
                cum += S / W
                any_ratio = True
            if best is None or mx > best:
                best = mx
                r["event_step_of_max"][e - 1] = t
        if best is not None:
            r["event_intensity_max"][e - 1] = best
            if sum_w != 0:
                r["event_intensity_mean"][e - 1] = np.float32(sum_s / sum_w)
        if any_ratio:
            r["event_intensity_cumulative"][e - 1] = np.float32(cum)
    return r
