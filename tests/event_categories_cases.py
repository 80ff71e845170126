"""Seeded inputs of the event-category tests (host and GPU).  Not collected by pytest."""
import numpy as np

N_EV = 6
N_DOY = 3


def weights(C):
    """Multiples of 2^-10 below 2^8: every float64 partial sum of them is exact, whatever the order."""
    return (np.random.default_rng(C).integers(1, 2**18, C) / 1024.0).astype(np.float32)


def spans(ids, n_ev=N_EV):
    """First / last timestep of the events 0..n_ev (INT_MAX / -1 when absent; entry 0 unused)."""
    tmin, tmax = np.full(n_ev + 1, 2**31 - 1, np.int64), np.full(n_ev + 1, -1, np.int64)
    for e in range(1, n_ev + 1):
        ts = np.nonzero((ids == e).any(axis=1))[0]
        if ts.size:
            tmin[e], tmax[e] = ts[0], ts[-1]
    return tmin, tmax


def case(T, C):
    """``(ids, anom, thr, doy)``: int32 / float32 ``[T, C]``, float32 ``[N_DOY, C]``, int32 ``[T]``.

    IDs 1..6 are events, -3, 0 and 9 background; runs of up to 150 cells cross the 64-cell pieces, the 1024 cells of a wave
    and the 4096 of a workgroup; the first eight cells of row 1 hold five events in one piece.  The thresholds are multiples
    of 2^-10, with NaN, +inf, 0 and a negative value mixed in.  An anomaly is a float32 product of its threshold with one of
    0.5, 1, 1.5, 2, 2.5, 3, 3.5, 4, 5 -- so every class boundary is hit exactly -- or the float32 just below such a product,
    or NaN / +inf / -inf; under a threshold that is no positive number it is a finite value of either sign."""
    rng = np.random.default_rng(1000 * T + C)
    ids = rng.integers(0, N_EV + 1, (T, C)).astype(np.int32)
    runs = np.repeat(rng.integers(0, N_EV + 1, (T, (C + 149) // 150)).astype(np.int32), 150, axis=1)[:, :C]
    ids = np.where(rng.random((T, C)) < 0.6, runs, ids)
    ids[rng.random((T, C)) < 0.05] = -3
    ids[rng.random((T, C)) < 0.03] = 9                     # above n_ev: background at the C ABI
    if C >= 65:
        ids[0, 3:min(C, 300)] = 3                          # one run over several pieces
    if C >= 8:
        ids[1, :8] = [1, 2, 3, 4, 6, 9, -3, 0]             # several events inside one piece
    if C > 4096:
        ids[3, 900:1200] = 4                               # across the end of a wave's 1024 cells
        ids[2, 3000:C] = 1                                 # across the end of a workgroup's 4096 cells
        ids[T - 1, 4090:C] = 2
    thr = (rng.integers(1, 2**12, (N_DOY, C)) / 1024.0).astype(np.float32)
    odd = rng.random((N_DOY, C)) < 0.08
    thr[odd] = np.resize(np.array([np.nan, np.inf, 0.0, -1.5], np.float32), int(odd.sum()))
    doy = rng.integers(0, N_DOY, T).astype(np.int32)
    h = thr[doy]
    mult = rng.choice(np.array([0.5, 1, 1.5, 2, 2.5, 3, 3.5, 4, 5], np.float32), (T, C))
    with np.errstate(invalid="ignore"):
        anom = (mult * h).astype(np.float32)
        below = rng.random((T, C)) < 0.3
        anom[below] = np.nextafter(anom[below], np.float32(-np.inf))
    nothr = ~(np.isfinite(h) & (h > 0))
    anom[nothr] = (rng.integers(-2**12, 2**12, int(nothr.sum())) / 1024.0).astype(np.float32)
    bad = rng.random((T, C)) < 0.04
    anom[bad] = np.resize(np.array([np.nan, np.inf, -np.inf], np.float32), int(bad.sum()))
    return ids, anom, thr, doy


def public_case(T, C):
    """:func:`case` as the trackers give it: everything that is not an event is 0."""
    ids, anom, thr, doy = case(T, C)
    return np.where((ids > 0) & (ids <= N_EV), ids, 0).astype(np.int32), anom, thr, doy
