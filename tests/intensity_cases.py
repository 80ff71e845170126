"""Seeded inputs of the event-intensity tests (host and GPU).  Not collected by pytest."""
import numpy as np

N_EV = 6
#: (6, 335) and (6, 693): no multiple of 64; (5, 4200): runs across a wave's 1024-cell and a workgroup's 4096-cell chunk end
SHAPES = [(6, 335), (6, 693), (5, 4200)]


def exact_field(T, C):
    """``(ids, anom)``: int32 / float32 ``[T, C]``.  IDs 1..6 are events, -3, 0 and 9 background.  Anomalies are multiples
    of 2^-10 below 64 in size, so that with the weights of :func:`weights` every float64 partial sum is exact.

    Event 2 is absent at t = 2 inside its span; event 5 is one cell; event 6 has only non-finite cells at t = 4; event 4
    has only negative anomalies at t = 1; NaN, +inf and -inf lie inside events; runs of 150 cells cross the pieces."""
    rng = np.random.default_rng(1000 * T + C)
    ids = rng.integers(0, N_EV + 1, (T, C)).astype(np.int32)
    runs = np.repeat(rng.integers(0, N_EV + 1, (T, (C + 149) // 150)).astype(np.int32), 150, axis=1)[:, :C]
    ids = np.where(rng.random((T, C)) < 0.6, runs, ids)
    ids[rng.random((T, C)) < 0.05] = -3
    ids[rng.random((T, C)) < 0.03] = 9                     # above n_ev: background at the C ABI
    ids[0, 40:300] = 3                                     # one run over five pieces
    if C > 4196:
        ids[0, 900:1200] = 3                               # across the end of a wave's chunk
        ids[1, 4000:4196] = 1                              # across the end of a workgroup's chunk
    ids[2][ids[2] == 2] = 0                                # event 2 absent inside its span ...
    ids[0, 7], ids[T - 1, 7] = 2, 2                        # ... which runs from the first step to the last
    ids[ids == 5] = 0
    ids[3, 17] = 5                                         # a single cell
    ids[1, :8] = [1, 2, 3, 4, 6, 9, -3, 0]
    anom = (rng.integers(-2**16 + 1, 2**16, (T, C)) / 1024.0).astype(np.float32)
    bad = rng.random((T, C)) < 0.04
    anom[bad] = np.resize(np.array([np.nan, np.inf, -np.inf], np.float32), int(bad.sum()))
    anom[4][ids[4] == 6] = np.resize(np.array([np.nan, -np.inf, np.inf], np.float32), int((ids[4] == 6).sum()))
    neg = (ids[1] == 4) & np.isfinite(anom[1])
    anom[1][neg] = -np.abs(anom[1][neg]) - np.float32(0.5)
    anom[3, 17] = np.float32(1.25)
    return ids, anom


def weights(C):
    """Multiples of 2^-8 below 2^10 (the weights of tests/test_gpu_event_rename.py)."""
    return (np.random.default_rng(C).integers(1, 2**18, C) / 256.0).astype(np.float32)


def spans(ids, n_ev=N_EV):
    """First / last timestep of the events 0..n_ev (INT_MAX / -1 when absent; entry 0 unused)."""
    tmin, tmax = np.full(n_ev + 1, 2**31 - 1, np.int64), np.full(n_ev + 1, -1, np.int64)
    for e in range(1, n_ev + 1):
        ts = np.nonzero((ids == e).any(axis=1))[0]
        if ts.size:
            tmin[e], tmax[e] = ts[0], ts[-1]
    return tmin, tmax


def public_field(T, C):
    """:func:`exact_field` as the trackers give it: everything that is not an event is 0."""
    ids, anom = exact_field(T, C)
    return np.where((ids > 0) & (ids <= N_EV), ids, 0).astype(np.int32), anom


def blobs(T=12, ny=24, nx=48):
    """A binary field of a few drifting discs that meet and part, one of them across the x seam."""
    yy, xx = np.mgrid[0:ny, 0:nx]
    #       y0,  x0,  vy,   vx,  r
    discs = [(6.0, 8.0, 0.2, 1.0, 3.2), (8.0, 30.0, 0.0, -1.0, 3.6), (17.0, 44.0, -0.1, 1.0, 3.0), (18.0, 14.0, -0.3, 0.2, 2.6)]
    out = np.zeros((T, ny, nx), bool)
    for t in range(T):
        for k, (y0, x0, vy, vx, r) in enumerate(discs):
            cy, cx = y0 + vy * t, (x0 + vx * t) % nx
            dx = np.abs(xx - cx)
            dx = np.minimum(dx, nx - dx)
            out[t] |= (yy - cy) ** 2 + dx ** 2 <= (r * (1 + 0.2 * np.sin(t / 2 + k))) ** 2
    return out


def blob_anomalies(shape, seed=5):
    """Positive multiples of 2^-10 below 8, a few NaN."""
    rng = np.random.default_rng(seed)
    a = (rng.integers(1, 2**13, shape) / 1024.0).astype(np.float32)
    a[rng.random(shape) < 0.02] = np.nan
    return a
