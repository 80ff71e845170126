"""First half of the tracker's pre-processing stage on the device: the step that follows
``preprocess_data`` in the reference pipeline and consumes ``extreme_events`` / ``mask`` while they are in HBM.

Mirrors ``marEx.tracker.fill_holes`` (track.py:1520-1676, gridded branch) and ``marEx.tracker.fill_time_gaps``
(track.py:1678-1726), ``marEx.tracker.identify_objects(time_connectivity=False)`` (track.py:1912-2049) and
``marEx.tracker.filter_small_objects`` (track.py:1755-1911), for gridded data and -- given ``neighbours`` -- for
unstructured meshes.
"""
from __future__ import annotations

import numpy as np

from .exceptions import ConfigurationError


def _host(a) -> np.ndarray:
    """The values of a DataArray-like or array-like input."""
    return np.asarray(a.values if hasattr(a, "values") else a)


def _as_u8(a) -> np.ndarray:
    return np.ascontiguousarray(_host(a)).astype(np.uint8)


def _check(data_bin, mask, R_fill, T_fill, neighbours=None):
    d, m = _host(data_bin), _host(mask)
    if neighbours is not None:
        nb = _host(neighbours)
        if d.ndim != 2 or m.shape != d.shape[1:] or nb.shape != (3, d.shape[1]):  # track.py:1063-1090
            raise ConfigurationError("Invalid neighbour array shape for unstructured grid",
                                     details=f"data {d.shape}, mask {m.shape}, neighbours {nb.shape}; expected (time, ncells), (ncells), (3, ncells)")
    elif d.ndim != 3 or m.shape != d.shape[1:]:
        raise ConfigurationError("fill_holes / fill_time_gaps on the device need gridded data (time, y, x) and a (y, x) mask",
                                 details=f"data {d.shape}, mask {m.shape}")
    if T_fill % 2 != 0:  # track.py:704-709
        raise ConfigurationError("T_fill must be even for temporal symmetry", details=f"Provided T_fill={T_fill} is odd")
    if int(R_fill) < 0 or int(R_fill) > 63:
        raise ConfigurationError("R_fill must be between 0 and 63 on the device path", details=f"R_fill={R_fill}")
    return d, m


def _nbr0(neighbours) -> np.ndarray:
    """The reference's ``neighbours.astype(np.int32) - 1`` (track.py:1060): 1-based input, 0 = no neighbour."""
    return np.ascontiguousarray(_host(neighbours).astype(np.int32) - 1)


def _upload(eng, a: np.ndarray):
    import torch

    return torch.from_numpy(a).to(eng.device)


def _upload_grid(eng, d, m=None):
    """Gridded ``(time, y, x)`` data as uint8 ``[T, ny * nx]`` on the device (and the ``(y, x)`` mask as ``[ny * nx]``)."""
    T, ny, nx = d.shape
    x = _upload(eng, _as_u8(d).reshape(T, ny * nx))
    return x, (None if m is None else _upload(eng, _as_u8(m).reshape(-1))), ny, nx


def _wrap(data_bin, t):
    """A uint8 device result as a bool array of the input's shape, with the input's labels when it has any."""
    res = t.cpu().numpy().astype(bool).reshape(_host(data_bin).shape)
    return data_bin.copy(data=res) if hasattr(data_bin, "copy") and hasattr(data_bin, "dims") else res


def fill_holes(data_bin, mask, R_fill: int, regional_mode: bool = False, neighbours=None, device: int = 0):
    """Fill holes and remove specks: binary closing then opening with a disk of radius ``R_fill`` (track.py:1520-1676);
    with ``neighbours`` (1-based ``[3, ncells]``) the unstructured-mesh form on ``(time, ncells)`` data.
    Returns a bool array (or DataArray with the input's labels) of the input's shape."""
    from .detect import get_engine

    d, m = _check(data_bin, mask, R_fill, 0, neighbours)
    eng = get_engine(device)
    if neighbours is not None:
        out = eng.fill_holes_mesh(_upload(eng, _as_u8(d)), _upload(eng, _as_u8(m)), _upload(eng, _nbr0(neighbours)), int(R_fill))
    else:
        x, mk, ny, nx = _upload_grid(eng, d, m)
        out = eng.fill_holes(x, mk, ny, nx, int(R_fill), regional_mode)
    eng.sync()
    return _wrap(data_bin, out)


def fill_time_gaps(data_bin, mask, R_fill: int, T_fill: int = 2, regional_mode: bool = False, neighbours=None, device: int = 0):
    """Close gaps of up to ``T_fill`` steps in time, then ``fill_holes(R_fill // 2)`` (track.py:1678-1726)."""
    from .detect import get_engine

    d, m = _check(data_bin, mask, R_fill, T_fill, neighbours)
    eng = get_engine(device)
    if neighbours is not None:
        if T_fill == 0:
            return data_bin
        tmp = eng.time_closing(_upload(eng, _as_u8(d)), int(T_fill))
        out = eng.fill_holes_mesh(tmp, _upload(eng, _as_u8(m)), _upload(eng, _nbr0(neighbours)), int(R_fill) // 2)
    else:
        x, mk, ny, nx = _upload_grid(eng, d, m)
        out = eng.fill_time_gaps(x, mk, ny, nx, int(R_fill), int(T_fill), regional_mode)
    eng.sync()
    return _wrap(data_bin, out)


def identify_objects_2d(data_bin, regional_mode: bool = False, device: int = 0):
    """Per-timestep 8-connected components, periodic in x unless ``regional_mode`` (track.py:2013-2031 with
    ``time_connectivity=False``).  Returns ``(ID field int32 [T, ny, nx], number of objects)``; IDs are unique across
    time, 0 = background; their numbering (1 + smallest linear index of the object) differs from the reference's."""
    from .detect import get_engine

    d = _host(data_bin)
    if d.ndim != 3:
        raise ConfigurationError("identify_objects_2d on the device needs gridded data (time, y, x)", details=f"data {d.shape}")
    eng = get_engine(device)
    x, _, ny, nx = _upload_grid(eng, d)
    r = eng.label_objects_2d(x, ny, nx, wrap_x=not regional_mode)
    eng.sync()
    n = int((r["areas"] > 0).sum().item())
    return r["labels"].cpu().numpy().reshape(d.shape), n


def filter_small_objects(data_bin, area_filter_quartile: float = 0.5, area_filter_absolute=None, regional_mode: bool = False,
                         mask=None, neighbours=None, device: int = 0):
    """Remove objects smaller than the ``area_filter_quartile`` percentile of all object areas (or an absolute number of
    cells).  Returns ``(filtered, area_threshold, object_areas, N_objects_prefiltered, N_objects_filtered)`` like
    track.py:1755-1911 (gridded branch: areas in cells)."""
    from .detect import get_engine

    d = _host(data_bin)
    if neighbours is not None:  # unstructured mesh: sizes in cells, clusters > 50 (5) cells enter the percentile, keep "> threshold"
        d, m = _check(data_bin, mask, 0, 0, neighbours)
        eng = get_engine(device)
        r = eng.filter_small_objects_mesh(_upload(eng, _as_u8(d)), _upload(eng, _as_u8(m)), _upload(eng, _nbr0(neighbours)),
                                          area_filter_quartile, area_filter_absolute)
    else:
        if d.ndim != 3:
            raise ConfigurationError("filter_small_objects on the device needs gridded data (time, y, x)", details=f"data {d.shape}")
        eng = get_engine(device)
        x, _, ny, nx = _upload_grid(eng, d)
        r = eng.filter_small_objects(x, ny, nx, area_filter_quartile, area_filter_absolute, regional_mode)
    eng.sync()
    return _wrap(data_bin, r["filtered"]), r["area_threshold"], r["object_areas"].cpu().numpy(), r["n_before"], r["n_after"]


def _preprocess_device(eng, x, mk, ny: int, nx: int, R_fill: int, T_fill: int, area_filter_quartile: float,
                       area_filter_absolute, regional_mode: bool):
    """The pipeline behind :func:`run_preprocess` and ``tracker.run_preprocess`` on device tensors (``x`` uint8
    ``[T, ny * nx]``, ``mk`` uint8 ``[ny * nx]``).  Returns the filtered uint8 tensor and ``object_stats``."""
    import torch

    raw_area = float(x.sum(dtype=torch.int64).item())
    a = eng.fill_holes(x, mk, ny, nx, int(R_fill), regional_mode)
    g = eng.fill_time_gaps(a, mk, ny, nx, int(R_fill), int(T_fill), regional_mode)
    r = eng.filter_small_objects(g, ny, nx, area_filter_quartile, area_filter_absolute, regional_mode)
    eng.sync()
    areas = r["object_areas"].to(torch.float64)
    total = float(areas.sum().item())
    accepted = float(areas[areas > r["area_threshold"]].sum().item())  # strictly above, as track.py:1337
    processed = float(r["filtered"].sum(dtype=torch.int64).item())
    stats = (total, r["n_before"], r["n_after"], r["area_threshold"], accepted / total,
             raw_area / processed if processed else float("nan"))
    return r["filtered"], stats


def _upload_rows(host: np.ndarray, t0: int, t1: int, buf) -> None:
    """Rows ``[t0, t1)`` of a host field (bool or 0 / 1 bytes, time first) into the uint8 ``[t1 - t0, C]`` device tensor
    ``buf``: the only way a host input of the blocked pre-processing reaches the device."""
    import torch

    rows = np.ascontiguousarray(host[t0:t1]).astype(np.uint8, copy=False).reshape(t1 - t0, -1)
    buf.copy_(torch.from_numpy(rows))


def _blocked_stats(r: dict):
    """``object_stats`` from the result of ``HotPath.preprocess_blocked``, as :func:`_preprocess_device` forms them."""
    import torch

    areas = r["object_areas"].to(torch.float64)
    total = float(areas.sum().item())
    accepted = float(areas[areas > r["area_threshold"]].sum().item())  # strictly above, as track.py:1337
    processed = r["processed_area"]
    return (total, r["n_before"], r["n_after"], r["area_threshold"], accepted / total,
            r["raw_area"] / processed if processed else float("nan"))


def _preprocess_blocked_device(eng, x, host, mk, ny: int, nx: int, R_fill: int, T_fill: int, area_filter_quartile: float,
                               area_filter_absolute, regional_mode: bool, block_steps: int):
    """:func:`_preprocess_device` in time blocks of ``block_steps`` steps (``HotPath.preprocess_blocked``): the same
    filtered tensor and ``object_stats``.  The field is ``x`` (uint8 ``[T, ny * nx]`` on the device) or, with ``x=None``,
    the host array ``host`` (time first), of which one window at a time is uploaded."""
    if x is None:
        T = int(host.shape[0])
        r = eng.preprocess_blocked(None, mk, int(R_fill), int(T_fill), int(block_steps), area_filter_quartile,
                                   area_filter_absolute, ny=ny, nx=nx, regional_mode=regional_mode, shape=(T, ny * nx),
                                   fetch=lambda t0, t1, buf: _upload_rows(host, t0, t1, buf))
    else:
        r = eng.preprocess_blocked(x, mk, int(R_fill), int(T_fill), int(block_steps), area_filter_quartile,
                                   area_filter_absolute, ny=ny, nx=nx, regional_mode=regional_mode)
    eng.sync()
    return r["filtered"], _blocked_stats(r)


def run_preprocess(extreme_events, mask, R_fill: int, T_fill: int = 2, area_filter_quartile: float = 0.5,
                   area_filter_absolute=None, regional_mode: bool = False, device: int = 0, block_steps=None):
    """The whole pre-processing stage of ``marEx.tracker.run_preprocess`` (track.py:1283-1360) for gridded data, on the
    device without intermediate host copies: ``fill_holes`` -> ``fill_time_gaps`` -> ``filter_small_objects``.

    Returns ``(data_bin_filtered, object_stats)`` with ``object_stats = (total_area_IDed, N_objects_prefiltered,
    N_objects_filtered, area_threshold, accepted_area_fraction, preprocessed_area_fraction)`` as in the reference
    (areas in cells; ``accepted_area`` sums the objects STRICTLY above the threshold, as track.py:1337 does).

    ``block_steps`` (a positive number of timesteps) runs the stage in time blocks of that many steps: the same results,
    with only one window of the input on the device at a time."""
    from .detect import get_engine

    d, m = _check(extreme_events, mask, R_fill, T_fill)
    eng = get_engine(device)
    if block_steps is not None:
        if isinstance(block_steps, bool) or not isinstance(block_steps, (int, np.integer)) or block_steps <= 0:
            raise ConfigurationError("block_steps must be a positive number of timesteps", details=f"block_steps={block_steps!r}")
        _, ny, nx = d.shape
        filtered, stats = _preprocess_blocked_device(eng, None, d, _upload(eng, _as_u8(m).reshape(-1)), ny, nx, R_fill, T_fill,
                                                     area_filter_quartile, area_filter_absolute, regional_mode, int(block_steps))
        return _wrap(extreme_events, filtered), stats
    x, mk, ny, nx = _upload_grid(eng, d, m)
    filtered, stats = _preprocess_device(eng, x, mk, ny, nx, R_fill, T_fill, area_filter_quartile, area_filter_absolute,
                                         regional_mode)
    return _wrap(extreme_events, filtered), stats
