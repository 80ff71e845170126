"""A brute-force NumPy oracle for ``marex_amd.nearest_cell_index`` and ``marex_amd.resample_nearest``: every (source,
target) pair, in chunks of targets, with exactly the operation order of the contract -- unit vectors
``x = cos(lat) cos(lon)``, ``y = cos(lat) sin(lon)``, ``z = sin(lat)`` in float64, squared chord
``q = (dx * dx + dy * dy) + dz * dz`` with every operation a separate NumPy float64 one, ``argmin`` on ``q`` and the lowest
cell number among the equals -- and the host distance formula.  Not collected by pytest."""
import numpy as np


def unit_vectors(lat, lon):
    """float64 ``[3, cells]`` of flat ``lat`` / ``lon`` in degrees; a NaN column where a coordinate is not finite."""
    lat, lon = np.asarray(lat, np.float64).reshape(-1), np.asarray(lon, np.float64).reshape(-1)
    with np.errstate(invalid="ignore"):
        la, lo = np.radians(lat), np.radians(lon)
        v = np.stack([np.cos(la) * np.cos(lo), np.cos(la) * np.sin(lo), np.sin(la)])
    v[:, ~(np.isfinite(lat) & np.isfinite(lon))] = np.nan
    return v


def expand(lat, lon):
    """The flat C-order ``(lat, lon)`` of a rectilinear grid spanned by 1-D ``lat [ny]`` and ``lon [nx]``."""
    la, lo = np.meshgrid(np.asarray(lat, np.float64), np.asarray(lon, np.float64), indexing="ij")
    return la.reshape(-1), lo.reshape(-1)


def brute(src, ids, dst, chunk=4096):
    """``(index int32 [M], q float64 [M])``: per target the smallest ``(q, cell number)`` over the sources ``src [3, N]``
    with cell numbers ``ids [N]`` (None: ``0 .. N - 1``); -1 and +inf for a target with a NaN coordinate."""
    N, M = src.shape[1], dst.shape[1]
    ids = np.arange(N, dtype=np.int64) if ids is None else np.asarray(ids, np.int64)
    index, q = np.full(M, -1, np.int32), np.full(M, np.inf)
    big = np.iinfo(np.int64).max
    for a in range(0, M, chunk):
        t = dst[:, a:a + chunk]
        with np.errstate(invalid="ignore"):
            dx, dy, dz = src[0][:, None] - t[0][None, :], src[1][:, None] - t[1][None, :], src[2][:, None] - t[2][None, :]
            qq = (dx * dx + dy * dy) + dz * dz
        ok = ~np.isnan(t).any(axis=0)
        qq[:, ~ok] = np.inf
        best = qq[qq.argmin(axis=0), np.arange(qq.shape[1])]  # argmin on q ...
        low = np.where(qq == best[None, :], ids[:, None], big).min(axis=0)  # ... then the lowest cell number among the equals
        index[a:a + chunk] = np.where(ok, low, -1)
        q[a:a + chunk] = np.where(ok, best, np.inf)
    return index, q


def distance_km(q, radius_km=6371.0):
    return 2.0 * radius_km * np.arcsin(np.minimum(1.0, np.sqrt(q) / 2.0))


def nearest(src_lat, src_lon, dst_lat, dst_lon, src_mask=None, max_distance_km=None, radius_km=6371.0):
    """The whole definition over flat coordinates: ``(index int32, distance_km float64, q float64)``."""
    s, d = unit_vectors(src_lat, src_lon), unit_vectors(dst_lat, dst_lon)
    ok = ~np.isnan(s).any(axis=0)
    if src_mask is not None:
        ok &= np.asarray(src_mask, bool).reshape(-1)
    ids = np.flatnonzero(ok)
    index, q = brute(s[:, ok], ids, d)
    with np.errstate(invalid="ignore"):
        dist = np.where(index >= 0, distance_km(np.where(index >= 0, q, 0.0), radius_km), np.nan)
        if max_distance_km is not None:
            keep = dist <= max_distance_km
            index, dist = np.where(keep, index, -1).astype(np.int32), np.where(keep, dist, np.nan)
    return index, dist, q


def gather(field, index, fill):
    """``field [T, C]`` at ``index [M]``, ``fill`` where the index is negative, in the field's dtype."""
    field, index = np.asarray(field), np.asarray(index).reshape(-1)
    out = field.reshape(field.shape[0], -1)[:, np.where(index >= 0, index, 0)].copy()
    out[:, index < 0] = fill
    return out
