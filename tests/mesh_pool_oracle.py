"""Oracle of ``neighbour_rings_hobday``: day-of-year thresholds pooled over mesh neighbour rings, from the committed oracle's
pieces (not collected by pytest; shared by test_mesh_pool_host.py, test_gpu_mesh_pool.py and test_gpu_mesh_pool_api.py).

    digitize_bins -> doy_bin_counts -> sum over pool(c, r) -> rolling_histogram_quantile
    -> NaN where the cell's own first kept anomaly is NaN, clamp and range statistics as hobday_thresholds_approx -> mask_ge_doy

``pool(c, r)`` is what ``r`` steps along LISTED links reach from ``c`` (``c`` included, every member once): the rows of
``M^r`` for ``M = I + listed links``, the reading ``oracle._mesh_dilation_matrix`` has of the neighbours table, without any
symmetrisation.  The pools are made here by plain set expansion, not by the code under test.
"""
import numpy as np

from oracle import marex_oracle as orc

N_DOY = orc.N_DOY


def pools(neighbours_1based, rings):
    """``[set of 0-based members]`` per cell.  ``neighbours_1based``: ``[nv, C]``, 0 = none."""
    nbr = np.asarray(neighbours_1based)
    C = nbr.shape[1]
    listed = [sorted({int(v) - 1 for v in nbr[:, c] if v > 0}) for c in range(C)]
    out = []
    for c in range(C):
        members = {c}
        for _ in range(int(rings)):
            members = members | {j for m in members for j in listed[m]}
        out.append(members)
    return out


def ring_and_chords(rng, C):
    """Neighbour table in the manner of ``_tri_mesh`` (tests/test_gpu_track_pre.py), 1-based with 0 = none: cells on a ring,
    one random chord each, some neighbours missing, some links listed from one end only."""
    nb = np.zeros((3, C), dtype=np.int32)
    nb[0] = (np.arange(C) + 1) % C + 1
    nb[1] = (np.arange(C) - 1) % C + 1
    nb[2] = rng.integers(0, C, C) + 1
    nb[2][rng.random(C) < 0.2] = 0
    nb[1][rng.random(C) < 0.05] = 0
    return nb


def pooled_thresholds(anom, doy_out, q, wd, edges, centres, neighbours_1based, rings, cells=None, chunk=64):
    """``(thr [C, 366] float32, stats)`` as ``orc.hobday_thresholds_approx`` returns them, the histograms summed over the pools.
    Cells are processed 64 at a time (the dense histogram is about 1.5 MB per cell): ``doy_bin_counts`` of the k-th members of
    the chunk's cells, for k = 0, 1, ..., added up.  ``cells=(c0, c1)``: only these cells (the others stay NaN and count in no
    statistic)."""
    anom = np.asarray(anom, dtype=np.float32)
    T, C = anom.shape
    nb = len(edges) - 1
    bins = orc.digitize_bins(anom, edges)
    pl = [sorted(p) for p in pools(neighbours_1based, rings)] if rings else [[c] for c in range(C)]
    thr = np.full((C, N_DOY), np.nan, dtype=np.float32)
    first, last = cells if cells is not None else (0, C)
    for c0 in range(first, last, chunk):
        own = list(range(c0, min(last, c0 + chunk)))
        pooled = np.zeros((len(own), N_DOY, nb), dtype=np.int64)
        for k in range(max(len(pl[c]) for c in own)):
            has = [i for i, c in enumerate(own) if len(pl[c]) > k]
            pooled[has] += orc.doy_bin_counts(bins[:, [pl[own[i]][k] for i in has]], doy_out, nb)
        thr[c0:c0 + len(own)] = orc.rolling_histogram_quantile(pooled, wd, q, centres)
    thr[np.isnan(anom[0])] = np.nan  # the cell's own first kept anomaly
    upper, lower = edges[-2], edges[3]
    with np.errstate(invalid="ignore"):
        too_high = thr > upper
        too_low = thr < lower
    stats = {
        "n_too_high": int(too_high.sum()),
        "n_too_low": int(too_low.sum()),
        "max": float(np.nanmax(thr)) if np.isfinite(thr).any() else float("nan"),
        "min": float(np.nanmin(thr)) if np.isfinite(thr).any() else float("nan"),
    }
    thr = np.where(too_low, lower, thr).astype(np.float32)
    return thr, stats


def pooled_extremes(anom, doy_out, q, wd, edges, centres, neighbours_1based, rings):
    """``(thr, stats, extreme [T, C] bool)``."""
    thr, stats = pooled_thresholds(anom, doy_out, q, wd, edges, centres, neighbours_1based, rings)
    return thr, stats, orc.mask_ge_doy(np.asarray(anom, dtype=np.float32), thr, doy_out)
