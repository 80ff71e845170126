"""The shared cases of the event exposure tests: ID fields, region maps, areas and anomalies at the edges of the kernel's
layout and of its key, and the comparison of an engine result with the oracle.  Not collected by pytest."""
import numpy as np

import event_exposure_oracle as eo

F = np.float32
NAN, INF = np.nan, np.inf


def id_field(rng, T, C, cover=0.4, n_ids=5):
    return np.where(rng.random((T, C)) < cover, rng.integers(1, n_ids + 1, (T, C)), 0).astype(np.int32)


def blob_field(rng, T, C, n_ids=6, width=9):
    """Events as runs of cells that drift: what a tracked field looks like along a row."""
    x = np.zeros((T, C), np.int32)
    for i in range(1, n_ids + 1):
        t0, n, c = int(rng.integers(0, T)), int(rng.integers(1, T + 1)), int(rng.integers(0, C))
        for t in range(t0, min(T, t0 + n)):
            c = (c + int(rng.integers(-2, 3))) % C
            x[t, c:c + width] = i
    return x


def dyadic_anomalies(rng, shape):
    """Multiples of 2^-10 below 64 in magnitude: with the weights below every partial sum of w a is exact in float64."""
    return (rng.integers(-(2**16) + 1, 2**16, shape) / 1024.0).astype(F)


def dyadic_weights(rng, C):
    """Multiples of 2^-8 below 2^10."""
    return (rng.integers(0, 2**18, C) / 256.0).astype(F)


def spoil(rng, anom, x):
    """NaN and both infinities under event cells."""
    p = np.argwhere(x > 0)
    pick = p[rng.permutation(len(p))[:max(3, len(p) // 10)]]
    for n, (t, c) in enumerate(pick):
        anom[t, c] = (NAN, INF, -INF)[n % 3]
    return anom


def region_map(name, C, cuts=()):
    """``(rank int32 [C], R)``."""
    c = np.arange(C)
    if name == "one":
        return np.zeros(C, np.int32), 1
    if name == "own":
        return c.astype(np.int32), C
    if name == "mod3":
        return (c % 3).astype(np.int32), 3
    if name == "holes":
        return np.where(c % 7 == 3, -1, c // 50).astype(np.int32), int((C - 1) // 50) + 1
    if name == "none":
        return np.full(C, -1, np.int32), 1
    if name == "edges":  # regions that change exactly at and one cell past every cut
        e = sorted({p + d for p in cuts for d in (0, 1) if p + d < C})
        return np.searchsorted(np.array(e, np.int64), c, side="right").astype(np.int32), len(e) + 1
    raise KeyError(name)


def assert_same(r, recs, anomalies, float_bytes=True):
    """An engine result against the oracle's records: keys, integers and maxima equal; the float64 sums byte for byte
    (``float_bytes``: dyadic inputs) or within 2 n u sum|w a|."""
    exp = eo.as_arrays(recs, anomalies)
    for k in ("t", "rank", "id", "cells", "finite", "area"):
        assert r[k].dtype == exp[k].dtype and r[k].shape == exp[k].shape, (k, r[k].dtype, r[k].shape, exp[k].shape)
        assert np.array_equal(r[k], exp[k]), (k, np.flatnonzero(r[k] != exp[k])[:5])
    assert (r["sums"] is None) == (not anomalies) and (r["vmax"] is None) == (not anomalies)
    if not anomalies:
        return
    assert r["vmax"].dtype == F and np.array_equal(r["vmax"], exp["vmax"], equal_nan=True)
    assert np.array_equal(np.signbit(r["vmax"]), np.signbit(exp["vmax"]))
    assert r["sums"].dtype == np.float64 and r["sums"].shape == exp["sums"].shape
    if float_bytes:
        assert r["sums"].tobytes() == exp["sums"].tobytes()
        return
    n = np.array([d["finite"] for d in recs], np.float64)
    dW, dS = np.abs(r["sums"][:, 0] - exp["sums"][:, 0]), np.abs(r["sums"][:, 1] - exp["sums"][:, 1])
    bW, bS = 2 * n * eo.U * exp["sums"][:, 0], 2 * n * eo.U * np.array([d["abs"] for d in recs])
    print("largest error of sum w: %.3e of bound %.3e; of sum w a: %.3e of bound %.3e" % (dW.max(), bW.max(), dS.max(), bS.max()))
    assert (dW <= bW).all() and (dS <= bS).all()
