"""Nearest-cell resampling between any two geometries on the sphere: meshes, curvilinear and rectilinear grids, point lists.

Every join of this package (``event_matching``, ``compound_events``, ``event_exposure``, ``regional_series`` with a region
map, ``event_composites`` with a second variable) needs both fields on the same cells.  Masks and ID fields are categorical
and cannot be averaged, so the resampler that keeps them meaningful is the nearest cell: :func:`nearest_cell_index` finds,
once per pair of geometries, the nearest eligible source cell of every target, and :func:`resample_nearest` gathers any
``(time, space)`` field through that index.  Both run on the device (``marex_nearest.hip``): the search
is exact -- the smallest ``(squared chord, cell number)`` pair, whatever the search structure -- and the gather is a copy.
The unit vectors, the distances and ``max_distance_km`` are host arithmetic in float64.
"""
from __future__ import annotations

import numpy as np

from . import _stream
from ._stream import _Windows, _check_block_steps
from .exceptions import ConfigurationError, create_data_validation_error
from .track import _host, _tensor_of

_I32_MAX = 2**31 - 1
METHODS = ("auto", "voxel", "brute")
MAX_VOXELS = 1024  # HotPath.NEAREST_MAX_VOXELS: the stopping margin of the ring search is derived for it
#: eligible source cells per voxel of the whole n^3 grid that the default n aims at: about 4.7 n^2 voxels touch the sphere,
#: so a quasi-uniform mesh leaves about 5 cells in an occupied voxel
CELLS_PER_N2 = 24
#: the rings a target searches before it goes to the brute kernel (the engine's ``max_rings``)
DEFAULT_MAX_RINGS = 32
#: method="auto": the brute kernel below this many eligible source cells, the voxel search from it on.  Measured (DESIGN.md
#: section 4): the brute kernel's time follows the sources, whatever the targets; it wins at 1024 sources (0.65 to 0.85 of
#: the voxel search's time) and loses at 4096 (1.5 to 2.1 times), so the rule sits between the two
AUTO_BRUTE_SOURCES = 2048


def default_voxels(n_eligible: int) -> int:
    """Voxels per axis for ``n_eligible`` source cells."""
    return int(max(1, min(MAX_VOXELS, round(float(np.sqrt(n_eligible / CELLS_PER_N2))))))


def default_max_rings(voxels: int) -> int:
    return int(min(voxels, DEFAULT_MAX_RINGS))


def unit_vectors(lat, lon) -> np.ndarray:
    """float64 ``[3, ...]``: ``x = cos(lat) cos(lon)``, ``y = cos(lat) sin(lon)``, ``z = sin(lat)`` of the radians of the
    broadcast ``lat`` and ``lon`` (degrees), each operation a NumPy float64 one; NaN where a coordinate is not finite."""
    lat, lon = np.asarray(lat, dtype=np.float64), np.asarray(lon, dtype=np.float64)
    with np.errstate(invalid="ignore"):
        la, lo = np.radians(lat), np.radians(lon)
        cl = np.cos(la)
        v = np.stack(np.broadcast_arrays(cl * np.cos(lo), cl * np.sin(lo), np.sin(la)))
    v[:, ~np.isfinite(v).all(axis=0)] = np.nan
    return v


def chord_distance_km(q, radius_km: float = 6371.0) -> np.ndarray:
    """The great-circle distance of a squared chord ``q`` on the unit sphere: ``2 R arcsin(min(1, sqrt(q) / 2))``."""
    return 2.0 * radius_km * np.arcsin(np.minimum(1.0, np.sqrt(q) / 2.0))


def _numbers(v, name: str) -> np.ndarray:
    a = np.asarray(_host(v))
    if a.dtype.kind not in "fiu":
        raise create_data_validation_error(f"{name} must be numbers in degrees", details=f"Found dtype {a.dtype}")
    return a.astype(np.float64)


def _geometry(lat, lon, rectilinear: bool, side: str) -> dict:
    """A side of the pair: ``shape``, ``dims``, ``coords`` and the float64 ``[3, cells]`` unit vectors ``xyz`` (NaN columns
    where a coordinate is not finite) in C order."""
    la, lo = _numbers(lat, f"{side}_lat"), _numbers(lon, f"{side}_lon")
    d_la, d_lo = tuple(getattr(lat, "dims", ()) or ()), tuple(getattr(lon, "dims", ()) or ())
    if rectilinear:
        if la.ndim != 1 or lo.ndim != 1:
            raise create_data_validation_error(f"{side}_rectilinear=True needs a 1-D {side}_lat [ny] and a 1-D {side}_lon [nx]",
                                               details=f"{side}_lat {la.shape}, {side}_lon {lo.shape}")
        dims = (d_la[0] if d_la else "lat", d_lo[0] if d_lo else "lon")
        if dims[0] == dims[1]:
            raise create_data_validation_error(f"{side}_lat and {side}_lon of a rectilinear grid need two dimension names", details=f"both {dims[0]!r}")
        shape = (la.shape[0], lo.shape[0])
        coords = {dims[0]: ((dims[0],), la), dims[1]: ((dims[1],), lo)}
        xyz = unit_vectors(la[:, None], lo[None, :])
    else:
        if la.shape != lo.shape or la.ndim < 1:
            raise create_data_validation_error(f"{side}_lat and {side}_lon must have one common shape (or pass {side}_rectilinear=True)",
                                               details=f"{side}_lat {la.shape}, {side}_lon {lo.shape}")
        if d_la and d_lo and d_la != d_lo:
            raise create_data_validation_error(f"{side}_lat and {side}_lon differ in their dimensions", details=f"{d_la} and {d_lo}")
        dims = d_la or d_lo or (("cells",) if la.ndim == 1 else ("y", "x") if la.ndim == 2 else tuple(f"dim_{k}" for k in range(la.ndim)))
        shape = la.shape
        coords = {}
        for src in (lon, lat):
            for k, c in (getattr(src, "coords", None) or {}).items():
                cd = tuple(getattr(c, "dims", ()) or ())
                if cd and all(d in dims for d in cd):
                    coords[k] = (cd, np.asarray(_host(c)))
        for k, v in (("lat", la), ("lon", lo)):
            if k not in dims:
                coords.setdefault(k, (dims, v))
        xyz = unit_vectors(la, lo)
    bad = np.abs(la[np.isfinite(la)]) > 90.0
    if bad.any():
        raise create_data_validation_error(f"{side}_lat must lie in -90 .. 90 degrees", details=f"{int(bad.sum())} values outside")
    cells = int(np.prod(shape))
    if cells >= _I32_MAX:
        raise create_data_validation_error(f"the {side} geometry has {cells} cells: the index is int32", details="2^31 - 1 or more")
    return {"shape": tuple(int(k) for k in shape), "dims": tuple(dims), "coords": coords, "xyz": np.ascontiguousarray(xyz.reshape(3, cells))}


def _check_search_args(max_distance_km, radius_km, method, voxels):
    """``(max_distance_km or None, radius_km)`` as floats; refuses what is not a search."""
    if method not in METHODS:
        raise ConfigurationError("method must be 'auto', 'voxel' or 'brute'", details=f"method={method!r}")
    v = voxels.item() if isinstance(voxels, np.generic) else voxels
    if v is not None and (isinstance(v, bool) or not isinstance(v, int) or not 1 <= v <= MAX_VOXELS):
        raise ConfigurationError(f"voxels must be a positive integer, at most {MAX_VOXELS} per axis", details=f"voxels={voxels!r}")

    def number(x, name):
        try:
            f = float(x)
        except (TypeError, ValueError):
            f = np.nan
        if isinstance(x, bool) or not (np.isfinite(f) and f > 0):
            raise ConfigurationError(f"{name} must be a finite number above 0", details=f"{name}={x!r}")
        return f

    return (None if max_distance_km is None else number(max_distance_km, "max_distance_km")), number(radius_km, "radius_km")


def search_limit(max_distance_km, radius_km: float) -> float:
    """The squared chord beyond which the device search may give up: that of ``max_distance_km``, widened by 2^-20 -- far
    more than the rounding of the host's distance formula, so that ``q`` above it always fails ``distance_km <=
    max_distance_km``.  +inf without a limit or where the limit reaches the antipode."""
    if max_distance_km is None:
        return float("inf")
    half = max_distance_km / (2.0 * radius_km)
    if half >= np.pi / 2:
        return float("inf")
    c = 2.0 * np.sin(half)
    return float(c * c * (1.0 + 2.0 ** -20))


def _engine(device):
    from .detect import get_engine

    return get_engine(0 if device is None else device)


def _nearest_cell_index(src_lat, src_lon, dst_lat, dst_lon, src_mask, max_distance_km, src_rectilinear, dst_rectilinear, radius_km,
                        method, voxels, device):
    from .xr_compat import DataArray, Dataset

    max_km, R = _check_search_args(max_distance_km, radius_km, method, voxels)
    src = _geometry(src_lat, src_lon, bool(src_rectilinear), "src")
    dst = _geometry(dst_lat, dst_lon, bool(dst_rectilinear), "dst")
    N, M = src["xyz"].shape[1], dst["xyz"].shape[1]
    ok = np.isfinite(src["xyz"]).all(axis=0)
    if src_mask is not None:
        m = np.asarray(_host(src_mask))
        if m.dtype != np.bool_ or (m.shape != src["shape"] and m.shape != (N,)):
            raise create_data_validation_error("src_mask must be a bool array over the source cells",
                                               details=f"got {m.dtype} {m.shape}, the source is {src['shape']}")
        ok &= m.reshape(-1)
    ids = np.flatnonzero(ok).astype(np.int32)
    if ids.size == 0:
        raise create_data_validation_error("no eligible source cell", details=f"{N} source cells, none finite and inside src_mask")
    n = int(voxels) if voxels is not None else default_voxels(ids.size)
    if method == "auto":
        method = "brute" if ids.size < AUTO_BRUTE_SOURCES else "voxel"
    index, q, fallback = np.full(M, -1, np.int32), np.full(M, np.inf), 0
    if M:
        r = _engine(device).nearest_index(np.ascontiguousarray(src["xyz"][:, ok]), ids, dst["xyz"], method=method, voxels=n,
                                          max_rings=default_max_rings(n), qmax=search_limit(max_km, R))
        index, q, fallback = r["index"], r["q"], r["fallback"]
    with np.errstate(invalid="ignore"):
        dist = np.where(index >= 0, chord_distance_km(np.where(index >= 0, q, 0.0), R), np.nan)
        if max_km is not None:
            keep = dist <= max_km
            index, dist = np.where(keep, index, -1).astype(np.int32), np.where(keep, dist, np.nan)
    c = {k: v for k, v in dst["coords"].items()}
    return Dataset({"index": DataArray(index.reshape(dst["shape"]), dims=dst["dims"], coords=c),
                    "distance_km": DataArray(dist.reshape(dst["shape"]), dims=dst["dims"], coords=c)},
                   attrs={"n_source": int(N), "source_shape": tuple(src["shape"]), "radius_km": R, "method": method,
                          "voxels": n if method == "voxel" else 0, "fallback_targets": int(fallback)})


def nearest_cell_index(src_lat, src_lon, dst_lat, dst_lon, src_mask=None, max_distance_km=None, src_rectilinear=False,
                       dst_rectilinear=False, radius_km=6371.0, method="auto", voxels=None, device=None):
    """The nearest source cell of every target cell on the sphere: the index that :func:`resample_nearest` gathers through.

    Latitudes and longitudes are degrees, in any longitude convention, and the two sides may differ in it.  Without
    ``*_rectilinear`` the ``lat`` and ``lon`` of a side have one common shape -- a mesh ``[cells]``, a curvilinear grid
    ``[y, x]``, a point list; with ``*_rectilinear=True`` the 1-D ``lat [ny]`` and ``lon [nx]`` span an ``(ny, nx)`` grid in C
    order.  So mesh to grid, grid to mesh, grid to grid and mesh to mesh are one function.  ``src_mask`` (bool over the source
    cells) names the cells that may be chosen, e.g. the ocean; a source cell with a non-finite coordinate counts as masked, a
    target with one gets index -1.  ``|lat| > 90`` and a source without any eligible cell raise
    :class:`DataValidationError`; ``voxels`` (a positive integer, at most 1024), ``method`` (``"auto"``, ``"voxel"``,
    ``"brute"``), ``max_distance_km`` and ``radius_km`` (positive numbers) raise :class:`ConfigurationError`.

    The contract: with the float64 unit vectors ``x = cos(lat) cos(lon)``, ``y = cos(lat) sin(lon)``, ``z = sin(lat)`` of
    NumPy, the squared chord of source ``i`` and target ``j`` is ``q = (dx * dx + dy * dy) + dz * dz``, every operation
    rounded on its own, and ``index[j]`` is the smallest ``i`` among the eligible cells that minimise ``q``.  Both methods
    give exactly that: ``"brute"`` compares every pair, ``"voxel"`` searches rings of a ``voxels^3`` grid around the target
    and stops only when no unseen cell can win or tie; ``"auto"`` takes the brute kernel below 2048 eligible source cells.
    ``distance_km`` is ``2 radius_km arcsin(min(1, sqrt(q) / 2))`` of the winning pair; ``max_distance_km`` keeps a target
    where ``distance_km <= max_distance_km`` and gives it -1 and NaN otherwise.

    Returns a Dataset over the target's shape, with the target's dimensions and coordinates: ``index`` (int32, the flat
    source cell in C order, -1: none) and ``distance_km`` (float64, NaN where ``index < 0``); attrs ``n_source``,
    ``source_shape``, ``radius_km``, ``method``, ``voxels`` (0 for the brute kernel) and ``fallback_targets`` (targets the
    ring search handed to the brute kernel)."""
    return _nearest_cell_index(src_lat, src_lon, dst_lat, dst_lon, src_mask, max_distance_km, src_rectilinear, dst_rectilinear,
                               radius_km, method, voxels, device)


def _index_of(index, C: int) -> dict:
    """The host side of an index: the int32 ``[M]`` values, validated against the ``C`` cells of a timestep, and the
    target's ``shape``, ``dims`` and ``coords``."""
    n_source = None
    if hasattr(index, "data_vars") or (hasattr(index, "attrs") and not hasattr(index, "shape")):
        n_source = index.attrs.get("n_source")
        index = index["index"]
    a = np.asarray(_host(index))
    if a.dtype.kind not in "iu":
        raise create_data_validation_error("index must be an integer array of source cells (-1: none)", details=f"Found dtype {a.dtype}")
    if a.ndim < 1:
        raise create_data_validation_error("index must have at least one dimension", details=f"got shape {a.shape}")
    if n_source is not None and int(n_source) != C:
        raise create_data_validation_error("the index was made for another source geometry",
                                           details=f"n_source = {int(n_source)}, a timestep of the field has {C} cells")
    if a.size and (int(a.min()) < -1 or int(a.max()) >= C):
        raise create_data_validation_error("index values must lie in -1 .. n_source - 1",
                                           details=f"found {int(a.min())} .. {int(a.max())} for {C} source cells")
    if a.size >= _I32_MAX:
        raise create_data_validation_error("the index has 2^31 - 1 or more target cells")
    dims = tuple(getattr(index, "dims", ()) or ())
    if not dims:
        dims = ("cells",) if a.ndim == 1 else ("y", "x") if a.ndim == 2 else tuple(f"dim_{k}" for k in range(a.ndim))
    coords = {}
    for k, c in (getattr(index, "coords", None) or {}).items():
        cd = tuple(getattr(c, "dims", ()) or ())
        if cd and all(d in dims for d in cd):
            coords[k] = (cd, np.asarray(_host(c)))
    return {"idx": np.ascontiguousarray(a.reshape(-1), dtype=np.int32), "shape": tuple(int(k) for k in a.shape), "dims": dims,
            "coords": coords}


def _fill_of(fill, kind: str, is_bool: bool):
    """The fill value of a field of ``kind`` ('m', 'i', 'f') as the Python number the engine takes."""
    if fill is None:
        return float("nan") if kind == "f" else 0
    f = fill.item() if isinstance(fill, np.generic) else fill
    if kind == "f":
        if isinstance(f, (bool, str)) or not isinstance(f, (int, float)):
            raise ConfigurationError("fill of a float field must be a number", details=f"fill={fill!r}")
        return float(np.float32(f))
    lo, hi = (0, 1 if is_bool else 255) if kind == "m" else (-_I32_MAX - 1, _I32_MAX)
    if isinstance(f, float) and f.is_integer():
        f = int(f)
    if isinstance(f, str) or not isinstance(f, (bool, int)) or not lo <= int(f) <= hi:
        raise ConfigurationError(f"fill of this field must be an integer in {lo} .. {hi}", details=f"fill={fill!r}")
    return int(f)


def _resample_nearest(field, index, fill, block_steps, device):
    from .xr_compat import DataArray

    what = "resample_nearest"
    block_steps = _check_block_steps(block_steps)
    p = _stream.plan_float_field(field, what, "field") if _stream._kind(field) == "f" else _stream.plan_field(field, what)
    name = _stream._dtype_name(field)
    if p["kind"] == "f" and name != "float32":
        raise create_data_validation_error("a float field must be float32", details=f"Found dtype {name}", data_info={"actual_dtype": name})
    T, C = p["T"], p["C"]
    ix = _index_of(index, C)
    M = ix["idx"].size
    fv = _fill_of(fill, p["kind"], p["bool"])
    np_dt = np.uint8 if p["kind"] == "m" else np.int32 if p["kind"] == "i" else np.float32
    out_np = np.bool_ if p["bool"] else np_dt
    resident = _tensor_of(field) is not None
    tc = {} if p["tv"] is None else {p["tname"]: (p["tname"], p["tv"])}
    dims, shape = (p["tname"],) + ix["dims"], (T,) + ix["shape"]
    if T == 0 or M == 0 or C == 0:  # nothing to gather (a source without cells admits an index of -1 only): no device work
        data = np.full(shape, fv, np_dt).astype(out_np)
        if resident:
            import torch

            data = torch.from_numpy(data).to(_tensor_of(field).device)
        return DataArray(data, dims=dims, coords={**ix["coords"], **tc})
    import torch

    from .engine import HotPath

    eng = _engine(device)
    fw = _Windows(eng, field, T, C, np_dt, p["kind"] == "i")
    per_step = fw.upload_bytes_per_step
    item = np.dtype(np_dt).itemsize
    B = _stream._window_steps(eng, what, T, max(C, M), per_step, T * M * item + 4 * M, block_steps,
                              f"the output of {T} x {M} cells of {item} bytes, the index, and the field of {T} timesteps of {C} cells, "
                              f"{item} bytes per cell, as far as it is not on the device already")
    out = HotPath._buf(None, "rs_out", (T, M), fw.tdt, eng.device)
    idx = torch.from_numpy(ix["idx"]).to(eng.device)
    for a in range(0, T, B):
        b = min(T, a + B)
        eng.resample_nearest(fw.get(a, b), idx, out[a:b], fv)
    if p["bool"]:
        out = out.view(torch.bool)
    data = out.reshape(shape) if resident else out.cpu().numpy().reshape(shape)
    return DataArray(data, dims=dims, coords={**ix["coords"], **tc})


def resample_nearest(field, index, fill=None, block_steps=None, device=None):
    """A ``(time, space)`` field on another geometry, by nearest cell: ``out[t, j] = field[t, index[j]]``, and ``fill`` where
    ``index[j] < 0``.

    ``field``: ``(time, cells)`` or ``(time, y, x)``, on the host or device resident (then it is read in place): a bool or
    uint8 mask (``extreme_events``, ``hobday_events``, ``compound_events``, ``alert_level``), an integer ID field (int32 is
    read as it is; another integer type is range-checked like the other statistics' ID fields and comes back as int32) or a
    float32 field (``dat_anomaly``, ``dhw``).  ``index``: the Dataset of :func:`nearest_cell_index`, its ``index`` variable,
    or a plain integer array over the target cells; it must be an integer type with values in ``-1 .. n_source - 1``, and
    ``n_source`` (taken from the field for a plain array) must be the cells of a timestep of ``field`` -- else
    :class:`DataValidationError`, before anything is launched.  ``fill``: None is 0 / False for masks and integers, NaN for
    floats.  ``block_steps``: as in :func:`marex_amd.event_intensity`; the result does not depend on it.

    Returns a DataArray with the field's time axis and the index's spatial dimensions and coordinates, in the field's dtype
    (a bool field stays bool): a device tensor when ``field`` was resident, a NumPy array otherwise.  It goes straight into
    ``tracker``, ``event_matching``, ``compound_events`` and the rest.  A resampled ID field keeps the source's IDs: an event
    whose cells fall apart, or two events that touch, on the target geometry are not re-labelled."""
    return _resample_nearest(field, index, fill, block_steps, device)
