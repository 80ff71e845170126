"""Shape and movement of tracked events on a grid: extent, perimeter, coastal contact, axes and the path of the centroid.

The reference passes ``properties=`` of ``calculate_object_properties`` straight to ``regionprops_table`` on grids
(``bbox``, ``perimeter``, ``eccentricity``, ``orientation``, the axis lengths).  Here it is one streaming pass on the device
(``marex_event_shapes_i32``): per (timestep, event) integer sums only -- cells, first and second
moments, a bounding box split at the seam, and the exposed sides of the 4-neighbour stencil -- into the compact slots of
``event_intensity``.  The host turns the exact integers into the Dataset in float64.

The perimeter is the count (or the length) of exposed cell sides and the orientation is measured from +x toward +y: this
project's own definitions, not scikit-image's estimators (its perimeter weighs diagonal steps, its orientation is measured
from the row axis); nothing here is pinned to scikit-image.
"""
from __future__ import annotations

import math
from typing import Optional

import numpy as np

from ._stream import (_I32_MAX, _Windows, _check_block_steps, _dtype_name, _kind, _plan_windows, _time_of, area_weight_table,
                      event_spans, pad_events, slot_index, spatial, tracker_time, walk_event_slots)
from .exceptions import ConfigurationError, TrackingError, create_data_validation_error
from .intensity import _time_of_max_values
from .track import _host, _tensor_of

MAX_SIDE = 65536  # the second moments are 64-bit sums: nx^2 n < 2^63 needs nx <= 2^16 beside n < 2^31
# columns of the device's ``mom`` (include/marex_hip.h)
_N, _SY, _SX, _NR, _FL, _SYY, _SXX, _SXY, _SRX, _SRY, _ENS, _EEW, _EBD, _ECS, _LEN, _AREA = range(16)


def grid_edge_lengths(lat, lon, radius_km: float = 6371.0):
    """``(ns_len [ny + 1], ew_len [ny])`` in km: the side lengths of the cells of a regular lat-lon grid of cell centres
    (degrees).  ``ns_len[j]`` is one cell's side on the interface between the rows ``j - 1`` and ``j``, ``R cos(phi_j)
    dlambda``, with the interface latitudes ``phi_j`` midway between neighbouring centres, half a spacing beyond the first
    and the last centre, clipped to +-90 degrees; ``ew_len[y] = R dphi_y``, the distance between the two interfaces of row
    ``y``.  ``dlambda`` is the mean spacing of ``lon``.  Needs no GPU."""
    la = np.asarray(_host(lat), dtype=np.float64).reshape(-1)
    lo = np.asarray(_host(lon), dtype=np.float64).reshape(-1)
    if la.size == 0 or lo.size == 0 or not np.isfinite(la).all() or not np.isfinite(lo).all():
        raise create_data_validation_error("lat and lon must be non-empty and finite", details=f"lat {la.shape}, lon {lo.shape}")
    if not radius_km > 0:
        raise create_data_validation_error("radius_km must be positive", details=f"radius_km={radius_km}")
    ny, nx = la.size, lo.size
    edge = np.empty(ny + 1)
    if ny > 1:
        edge[1:-1] = 0.5 * (la[:-1] + la[1:])
        edge[0] = la[0] - 0.5 * (la[1] - la[0])
        edge[-1] = la[-1] + 0.5 * (la[-1] - la[-2])
    else:
        dl0 = abs(lo[1] - lo[0]) if nx > 1 else 1.0  # a single row: as tall as a cell is wide
        edge[0], edge[1] = la[0] - 0.5 * dl0, la[0] + 0.5 * dl0
    edge = np.clip(edge, -90.0, 90.0)
    dlam = abs(lo[-1] - lo[0]) / (nx - 1) if nx > 1 else 360.0
    k = math.pi / 180.0
    ns = radius_km * np.cos(edge * k) * (dlam * k)
    ew = radius_km * np.abs(np.diff(edge)) * k
    return np.maximum(ns, 0.0), ew


def edge_weight_tables(edge_lengths, ny: int, nx: int):
    """``(e, ns_q int64 [ny + 1], ew_q int64 [ny])``: the fixed-point side lengths, ``q = rint(v * 2^e)`` with ``e = 61 -
    ceil(log2(total))`` -- the rule of :func:`marex_amd.regional.area_weight_table` applied to the total length of all the
    sides of the grid, ``nx sum(ns_len) + (nx + 1) sum(ew_len)``: a sum over any set of sides, each counted once, stays
    below 2^62.  A length is ``ldexp(float64(S), -e)`` of its integer sum.  Needs no GPU."""
    try:
        ns, ew = edge_lengths
    except (TypeError, ValueError):
        raise create_data_validation_error("edge_lengths must be a pair (ns_len [ny + 1], ew_len [ny])") from None
    ns, ew = np.asarray(_host(ns), dtype=np.float64), np.asarray(_host(ew), dtype=np.float64)
    if ns.shape != (ny + 1,) or ew.shape != (ny,):
        raise create_data_validation_error("edge_lengths do not match the grid",
                                           details=f"ns_len {ns.shape} and ew_len {ew.shape}, a grid of {ny} rows needs "
                                                   f"({ny + 1},) and ({ny},)")
    both = np.concatenate([ns, ew])
    if not np.isfinite(both).all() or (both < 0).any():
        raise create_data_validation_error("edge_lengths must be finite and non-negative",
                                           details=f"{int((~np.isfinite(both)).sum())} non-finite, {int((both < 0).sum())} negative")
    total = float(nx * ns.sum() + (nx + 1) * ew.sum())
    if not (total > 0 and np.isfinite(total)):
        raise create_data_validation_error("edge_lengths must have a positive, finite sum", details=f"sum {total}")
    e = 61 - int(np.ceil(np.log2(total)))
    return e, np.rint(np.ldexp(ns, e)).astype(np.int64), np.rint(np.ldexp(ew, e)).astype(np.int64)


def _validate(ID_field, mask, cell_areas, edge_lengths, lat, lon):
    """Everything that can be refused without a device: a dict of the shape, the time axis and the host tables."""
    shape = tuple(int(k) for k in ID_field.shape)
    if len(shape) == 2:
        raise ConfigurationError("event_shapes: shapes are gridded only",
                                 details=f"got a (time, cells) field of shape {shape}: a mesh has no rows, columns or cell "
                                         "sides to measure; pass a (time, y, x) field, or measure a mesh with mesh_event_shapes")
    if len(shape) != 3:
        raise create_data_validation_error("ID_field must be (time, y, x)", details=f"got shape {shape}")
    if _kind(ID_field) != "i":
        raise create_data_validation_error("Object IDs must be integers", details=f"Found dtype {_dtype_name(ID_field)}",
                                           data_info={"actual_dtype": _dtype_name(ID_field)})
    T, ny, nx = shape
    C = ny * nx
    if C >= _I32_MAX or T >= _I32_MAX:
        raise TrackingError(f"event_shapes: a timestep of {C} cells or a record of {T} steps reaches 2^31 - 1",
                            details="the field may hold any number of cells, a single timestep and the time axis may not")
    if ny > MAX_SIDE or nx > MAX_SIDE:
        raise TrackingError(f"event_shapes: a grid of {ny} x {nx} has a side above {MAX_SIDE}",
                            details="the second moments are 64-bit integer sums: nx^2 n stays below 2^63 up to that side")
    if _tensor_of(ID_field) is None and T and C:
        h = np.asarray(ID_field.values if hasattr(ID_field, "values") else ID_field)
        lo = int(h.min())
        if lo < 0:
            raise create_data_validation_error("Object IDs must be non-negative", details=f"smallest ID {lo}; 0 is background",
                                               data_info={"min_id": lo, "max_id": int(h.max())})
    tname, tv = _time_of(ID_field, T)
    dims = tuple(getattr(ID_field, "dims", ()) or ())
    p = {"shape": shape, "T": T, "ny": ny, "nx": nx, "C": C, "tname": tname, "tv": tv if tv is not None else np.arange(T),
         "labelled": bool(dims), "sdims": dims[1:], "mask": None, "area": None, "edges": None, "lat": None, "lon": None}
    if mask is not None:
        m = spatial(mask, p, "mask", mismatch="mask does not match the spatial shape of ID_field")
        if m.dtype != bool and m.dtype.kind not in "iu":
            raise create_data_validation_error("mask must be boolean (True: inside the domain)", details=f"Found dtype {m.dtype}")
        p["mask"] = np.ascontiguousarray(m != 0).view(np.uint8)
    if cell_areas is not None:
        a = spatial(cell_areas, p, "cell_areas", True, "cell_areas do not match the spatial shape of ID_field", numbers=True)
        if C:
            p["area"] = area_weight_table(a)  # in float64, whatever type the areas came in
    if edge_lengths is not None and C:
        p["edges"] = edge_weight_tables(edge_lengths, ny, nx)
    if (lat is None) != (lon is None):
        raise create_data_validation_error("lat and lon come together")
    if lat is not None:
        la, lo = np.asarray(_host(lat), np.float64), np.asarray(_host(lon), np.float64)
        if la.shape != (ny,) or lo.shape != (nx,) or not np.isfinite(la).all() or not np.isfinite(lo).all():
            raise create_data_validation_error("lat and lon must be finite 1-D coordinates of the grid's rows and columns",
                                               details=f"lat {la.shape}, lon {lo.shape}, a timestep {(ny, nx)}")
        p["lat"], p["lon"] = la, lo
    return p


def _no_slots():
    return 0, np.zeros(1, np.int64), np.zeros(2, np.int64), np.zeros((0, 16), np.int64), np.zeros((0, 6), np.int32)


def _device_slots(eng, ID_field, p: dict, regional: bool, block_steps):
    """The two passes over the field: the events' spans, then the sums.  ``(N, tmin, off, mom, box)`` on the host."""
    T, C, ny, nx = p["T"], p["C"], p["ny"], p["nx"]
    ids_w = _Windows(eng, ID_field, T, C, np.int32, True)
    B = _plan_windows(eng, T, C, ids_w.upload_bytes_per_step, block_steps, "event_shapes",
                      f"the ID field of {T} timesteps of {C} cells, 4 bytes per cell, as far as it is not on the device already")
    N, tmin, tmax, wins, kept = event_spans(eng, ids_w, T, B)
    if N <= 0:
        return _no_slots()
    dev = {"mask": None if p["mask"] is None else eng._dev(p["mask"]),
           "area_q": None if p["area"] is None else eng._dev(p["area"][1]),
           "ns_q": None if p["edges"] is None else eng._dev(p["edges"][1]),
           "ew_q": None if p["edges"] is None else eng._dev(p["edges"][2])}
    r = walk_event_slots(ids_w, wins, kept, lambda x, a, b, acc, finish: eng.event_shapes(
        x, ny, nx, tmin, tmax, regional=regional, t0=a, acc=acc, finish=finish, **dev))
    return N, tmin, r["off"], r["mom"], r["box"]


def _exact_axes(n, sy, sx, syy, sxx, sxy):
    """``(TR, ROOT, DET, NXY2, DIFF)`` float64 from the exact integer numerators ``Nxx = n sxx - sx^2``, ``Nyy``, ``Nxy`` of the
    second central moments (times ``n^2``): ``TR = Nxx + Nyy``, ``ROOT = sqrt((Nxx - Nyy)^2 + 4 Nxy^2)``, ``DET = Nxx Nyy -
    Nxy^2``, ``NXY2 = 2 Nxy``, ``DIFF = Nxx - Nyy``.  Each row is computed in int64 where a bound of every intermediate
    product stays below 2^62, in Python integers otherwise -- decided row by row, never wrapped."""
    f = np.float64
    nf = n.astype(f)
    m = np.maximum(np.maximum(sxx.astype(f), syy.astype(f)), np.abs(sxy.astype(f)))
    big1 = nf * m + np.maximum(np.abs(sx.astype(f)), np.abs(sy.astype(f))) ** 2  # bounds |Nxx|, |Nyy|, |Nxy| and their parts
    bound = 8.0 * big1 * big1  # (Nxx - Nyy)^2 + 4 Nxy^2 <= 8 max^2, Nxx Nyy + Nxy^2 <= 2 max^2
    small = bound < 2.0 ** 62
    out = [np.zeros(n.size, f) for _ in range(5)]

    def numerators(n_, sy_, sx_, syy_, sxx_, sxy_):
        nxx, nyy, nxy = n_ * sxx_ - sx_ * sx_, n_ * syy_ - sy_ * sy_, n_ * sxy_ - sx_ * sy_
        d = nxx - nyy
        return nxx + nyy, d * d + 4 * nxy * nxy, nxx * nyy - nxy * nxy, 2 * nxy, d

    if small.any():
        tr, disc, det, nxy2, d = numerators(*(v[small] for v in (n, sy, sx, syy, sxx, sxy)))
        for o, v in zip(out, (tr.astype(f), np.sqrt(disc.astype(f)), det.astype(f), nxy2.astype(f), d.astype(f))):
            o[small] = v
    for i in np.nonzero(~small)[0]:
        tr, disc, det, nxy2, d = numerators(*(int(v[i]) for v in (n, sy, sx, syy, sxx, sxy)))
        out[0][i], out[1][i], out[2][i], out[3][i], out[4][i] = float(tr), math.sqrt(disc), float(det), float(nxy2), float(d)
    return out


def _haversine_km(la1, lo1, la2, lo2, radius_km: float = 6371.0):
    k = math.pi / 180.0
    p1, p2 = la1 * k, la2 * k
    dp, dl = p2 - p1, (lo2 - lo1) * k
    s1, s2 = np.sin(dp / 2.0), np.sin(dl / 2.0)
    a = s1 * s1 + np.cos(p1) * np.cos(p2) * (s2 * s2)
    return 2.0 * radius_km * np.arcsin(np.minimum(1.0, np.sqrt(a)))


def _interp_latlon(cy, cx, lat, lon):
    """The centroids in degrees: linear in the coordinate arrays, longitude periodic (the column after the last is the first,
    a step between two columns goes the short way round 360 degrees)."""
    ny, nx = lat.size, lon.size
    i0 = np.clip(np.floor(cy).astype(np.int64), 0, ny - 1)
    i1 = np.minimum(i0 + 1, ny - 1)
    la = lat[i0] + (cy - i0) * (lat[i1] - lat[i0])
    j0 = np.clip(np.floor(cx).astype(np.int64), 0, nx - 1)
    j1 = (j0 + 1) % nx
    d = lon[j1] - lon[j0]
    d = d - 360.0 * np.rint(d / 360.0)
    return la, lon[j0] + (cx - j0) * d


def _finish(p: dict, N: int, tmin, off, mom, box, regional: bool, per_timestep: bool, tname: str, tv, tcoord: Optional[str] = None):
    """The Dataset from the compact slots, in float64 from the exact integers and in ascending time per event."""
    from .xr_compat import DataArray, Dataset

    T, ny, nx = p["T"], p["ny"], p["nx"]
    tv = np.asarray(tv)
    ids = np.arange(1, N + 1, dtype=np.int32)
    idc = {"ID": ("ID", ids)}
    tid = {tcoord or tname: (tname, tv), **idc}
    e_all, t_all = slot_index(off, tmin, N)
    mom = np.asarray(mom).astype(np.int64, copy=False).reshape(-1, 16)
    box = np.asarray(box).reshape(-1, 6)
    here = mom[:, _N] > 0
    e_of, t_of, m, bx = e_all[here], t_all[here], mom[here], box[here].astype(np.int64)
    n, sy, sx, nr = m[:, _N], m[:, _SY], m[:, _SX], m[:, _NR]
    seam = (m[:, _FL] == 3) & (not regional)
    # centroid: the values of object_moments
    cy = sy / n
    cx = sx / n
    c = (sx[seam] - nx * nr[seam]) / n[seam]
    cx[seam] = np.where(c < 0, c + nx, c)
    # bounding box under the same seam rule: the cells right of nx // 2 of a wrapped object stand nx to the left
    has_l, has_r = bx[:, 3] >= 0, bx[:, 5] >= 0
    shift = np.where(seam, nx, 0)
    lo_r, hi_r = bx[:, 4] - shift, bx[:, 5] - shift
    big = np.int64(2**40)
    x0 = np.minimum(np.where(has_l, bx[:, 2], big), np.where(has_r, lo_r, big))
    x1 = np.maximum(np.where(has_l, bx[:, 3], -big), np.where(has_r, hi_r, -big))
    width, height = x1 - x0 + 1, bx[:, 1] - bx[:, 0] + 1
    x0 = np.mod(x0, nx) if nx else x0
    # second moments: the seam shift is algebra on the sums (exact in Python integers where int64 would not hold it)
    sxs, sxx, sxy = sx.copy(), m[:, _SXX].copy(), m[:, _SXY].copy()
    obj = False
    if seam.any():
        if float(nx) ** 2 * float(nr[seam].max()) + 2.0 * nx * float(m[seam, _SRX].max()) < 2.0 ** 62:
            sxs[seam] = sx[seam] - nx * nr[seam]
            sxx[seam] = sxx[seam] - 2 * nx * m[seam, _SRX] + nx * nx * nr[seam]
            sxy[seam] = sxy[seam] - nx * m[seam, _SRY]
        else:
            obj = True
            sxs, sxx, sxy = sxs.astype(object), sxx.astype(object), sxy.astype(object)
            for i in np.nonzero(seam)[0]:
                sxs[i] = int(sx[i]) - nx * int(nr[i])
                sxx[i] = int(m[i, _SXX]) - 2 * nx * int(m[i, _SRX]) + nx * nx * int(nr[i])
                sxy[i] = int(m[i, _SXY]) - nx * int(m[i, _SRY])
    tr, root, det, nxy2, diff = _exact_axes(n.astype(object) if obj else n, sy.astype(object) if obj else sy, sxs,
                                            m[:, _SYY].astype(object) if obj else m[:, _SYY], sxx, sxy)
    n2 = n.astype(np.float64) ** 2
    l1n = (tr + root) / 2.0
    some = l1n > 0
    safe = np.where(some, l1n, 1.0)
    major = np.where(some, 4.0 * np.sqrt(l1n / n2), 0.0)
    minor = np.where(some, 4.0 * np.sqrt(np.maximum(det / safe, 0.0) / n2), 0.0)
    ecc = np.where(some, np.sqrt(np.minimum(root / safe, 1.0)), 0.0)  # 1 - l2 / l1 = sqrt(disc) / l1, without the cancellation
    orient = np.where(some, 0.5 * np.arctan2(nxy2, diff), 0.0)
    # sides
    ens, eew, ebd, ecs = m[:, _ENS], m[:, _EEW], m[:, _EBD], m[:, _ECS]
    sides = ens + eew
    area = np.ldexp(m[:, _AREA].astype(np.float64), -p["area"][0]) if p["area"] is not None else n.astype(np.float64)
    perim = np.ldexp(m[:, _LEN].astype(np.float64), -p["edges"][0]) if p["edges"] is not None else sides.astype(np.float64)
    with np.errstate(invalid="ignore", divide="ignore"):
        share = np.where(sides > 0, ecs / np.where(sides > 0, sides, 1), np.nan)
        compact = np.where(perim > 0, 4.0 * math.pi * area / np.where(perim > 0, perim * perim, 1.0), np.nan)
    extent = n / (height * width).astype(np.float64)
    data = {}
    if per_timestep:
        def dense(v, dt, fill):
            d = np.full((T, N), fill, dt)
            d[t_of, e_of - 1] = v
            return DataArray(d, dims=(tname, "ID"), coords=tid)

        for name, v, dt, fill in (
                ("cells", n, np.int64, 0), ("area", area, np.float64, np.nan), ("bbox_y0", bx[:, 0], np.int64, -1),
                ("bbox_x0", x0, np.int64, -1), ("bbox_height", height, np.int64, 0), ("bbox_width", width, np.int64, 0),
                ("extent", extent, np.float64, np.nan), ("edges_ns", ens, np.int64, 0), ("edges_ew", eew, np.int64, 0),
                ("border_edges", ebd, np.int64, 0), ("coast_edges", ecs, np.int64, 0), ("perimeter", perim, np.float64, np.nan),
                ("coast_share", share, np.float64, np.nan), ("compactness", compact, np.float64, np.nan),
                ("centroid_y", cy, np.float64, np.nan), ("centroid_x", cx, np.float64, np.nan),
                ("axis_major_length", major, np.float64, np.nan), ("axis_minor_length", minor, np.float64, np.nan),
                ("eccentricity", ecc, np.float64, np.nan), ("orientation", orient, np.float64, np.nan)):
            data[name] = dense(v, dt, fill)
    # per event; the rows of an event are in ascending time, and np.add.at adds one element after the other
    E = N + 1
    duration = np.bincount(e_of, minlength=E).astype(np.int32)
    has = duration > 0

    def emax(v, dt, fill):
        o = np.full(E, fill, dt)
        np.maximum.at(o, e_of, v.astype(dt))
        return o

    cells_max = emax(n, np.int64, 0)
    first = np.full(E, np.iinfo(np.int64).max, np.int64)
    at_max = n == cells_max[e_of]
    np.minimum.at(first, e_of[at_max], t_of[at_max])

    def esum(v, sel=None):
        o = np.zeros(E)
        if sel is None:
            np.add.at(o, e_of, v)
        else:
            np.add.at(o, e_of[sel], v[sel])
        return o

    with np.errstate(invalid="ignore", divide="ignore"):
        dur_f = np.where(has, duration, 1).astype(np.float64)
        compact_mean = np.where(has, esum(compact) / dur_f, np.nan)
        ecc_mean = np.where(has, esum(ecc) / dur_f, np.nan)
        all_sides, all_coast = np.zeros(E, np.int64), np.zeros(E, np.int64)
        np.add.at(all_sides, e_of, sides)
        np.add.at(all_coast, e_of, ecs)
        coast_share = np.where(all_sides > 0, all_coast / np.where(all_sides > 0, all_sides, 1), np.nan)
    coast_steps = np.bincount(e_of[ecs > 0], minlength=E).astype(np.int32)
    # the path of the centroid: consecutive present steps of one event are consecutive rows
    eo, cyo, cxo = e_of, cy, cx
    pair = eo[1:] == eo[:-1]
    if p["lat"] is not None:
        la, lo = _interp_latlon(cyo, cxo, p["lat"], p["lon"])
        step = _haversine_km(la[:-1], lo[:-1], la[1:], lo[1:])
    else:
        dy, dx = cyo[1:] - cyo[:-1], np.abs(cxo[1:] - cxo[:-1])
        if not regional:
            dx = np.minimum(dx, nx - dx)
        step = np.sqrt(dy * dy + dx * dx)
    path = np.zeros(E)
    np.add.at(path, eo[1:][pair], step[pair])
    i_first = np.full(E, eo.size, np.int64)
    i_last = np.full(E, -1, np.int64)
    np.minimum.at(i_first, eo, np.arange(eo.size))
    np.maximum.at(i_last, eo, np.arange(eo.size))
    disp = np.full(E, np.nan)
    if has.any():
        a, b = i_first[has], i_last[has]
        if p["lat"] is not None:
            disp[has] = _haversine_km(la[a], lo[a], la[b], lo[b])
        else:
            dy, dx = cyo[b] - cyo[a], np.abs(cxo[b] - cxo[a])
            if not regional:
                dx = np.minimum(dx, nx - dx)
            disp[has] = np.sqrt(dy * dy + dx * dx)
    with np.errstate(invalid="ignore", divide="ignore"):
        speed = np.where(duration > 1, path / np.where(duration > 1, duration - 1, 1), np.nan)
    for name, v in (("event_duration", duration[1:]), ("event_cells_max", cells_max[1:]),
                    ("event_time_of_max_cells", _time_of_max_values(tv, first[1:], has[1:])),
                    ("event_height_max", emax(height, np.int64, 0)[1:]), ("event_width_max", emax(width, np.int64, 0)[1:]),
                    ("event_perimeter_max", np.where(has, emax(perim, np.float64, -np.inf), np.nan)[1:]),
                    ("event_compactness_mean", compact_mean[1:]), ("event_eccentricity_mean", ecc_mean[1:]),
                    ("event_coast_steps", coast_steps[1:]), ("event_coast_share", coast_share[1:]),
                    ("event_path_length", np.where(has, path, np.nan)[1:]), ("event_displacement", disp[1:]),
                    ("event_speed_mean", speed[1:])):
        data[name] = DataArray(v, dims=("ID",), coords=idc)
    ds = Dataset(data, coords=tid)
    ds.attrs["distance_units"] = "km" if p["lat"] is not None else "cells"
    ds.attrs["perimeter_units"] = "km" if p["edges"] is not None else "sides"
    return ds


def _event_shapes(ID_field, mask, cell_areas, edge_lengths, lat, lon, regional_mode, per_timestep, block_steps, device,
                  n_events: Optional[int] = None, time: Optional[tuple] = None):
    block_steps = _check_block_steps(block_steps)
    p = _validate(ID_field, mask, cell_areas, edge_lengths, lat, lon)
    tracker_time(p, time)
    if p["T"] == 0 or p["C"] == 0:
        N, tmin, off, mom, box = _no_slots()
    else:
        from .detect import get_engine

        N, tmin, off, mom, box = _device_slots(get_engine(device), ID_field, p, bool(regional_mode), block_steps)
    N, tmin, off = pad_events("event_shapes", N, n_events, tmin, off)
    return _finish(p, N, tmin, off, mom, box, bool(regional_mode), bool(per_timestep), p["tname"], p["tv"], p["tcoord"])


def event_shapes(ID_field, mask=None, cell_areas=None, edge_lengths=None, lat=None, lon=None, regional_mode: bool = False,
                 per_timestep: bool = True, block_steps=None, device: int = 0):
    """What shape every tracked event has, how much of its edge lies on the coast and how far it moves, from one pass over
    a gridded event field on the device.

    ``ID_field``: an integer ``(time, y, x)`` event field of the basic or the merge tracker, a host array or DataArray or
    device resident (then it is read in place); the positive values are the event numbers, a negative value is refused.  A
    mesh field ``(time, cells)`` raises :class:`ConfigurationError`: shapes are gridded only.  ``mask``: boolean ``[ny,
    nx]``, True inside the domain (ocean), for ``coast_edges``.  ``cell_areas``: non-negative areas, ``[ny, nx]``, ``[C]`` or
    ``[ny]`` (broadcast along x).  ``edge_lengths``: a pair ``(ns_len [ny + 1], ew_len [ny])`` such as
    :func:`grid_edge_lengths` gives.  ``lat`` / ``lon``: 1-D degrees of the rows and columns, for distances in km.
    ``regional_mode``: x is not periodic and the first and last column are domain border.  ``block_steps`` as in
    :func:`marex_amd.event_intensity`; the results do not depend on it.

    A side of a cell is exposed when the neighbour across it holds a different value, 0 included, or lies outside the
    domain (above row 0, below row ny - 1, and beside the first and last column in ``regional_mode``); each of the four
    sides of a cell is tested on its own, so an edge between two events counts once for each.

    Returns a Dataset over ``time`` and ``ID = 1 .. N``.  With ``per_timestep``, dense ``(time, ID)``, where the event is
    absent NaN, 0 for counts and -1 for ``bbox_y0`` / ``bbox_x0``: ``cells``; ``area`` (the cells, or the sum of
    ``cell_areas``); ``bbox_y0``, ``bbox_x0`` (mod nx), ``bbox_height``, ``bbox_width`` (an object that
    ``calculate_centroid``'s rule treats as wrapped has its cells right of ``nx // 2`` moved ``nx`` to the left first);
    ``extent = cells / (height width)``; ``edges_ns``, ``edges_ew``, ``border_edges``, ``coast_edges`` (exposed sides whose
    neighbour is inside the domain and False in ``mask``); ``perimeter`` (the exposed sides, or with ``edge_lengths`` their
    length); ``coast_share = coast_edges / (edges_ns + edges_ew)``; ``compactness = 4 pi area / perimeter^2`` (meaningful
    where both are counts or both physical); ``centroid_y``, ``centroid_x`` (the values of ``object_moments``);
    ``axis_major_length = 4 sqrt(l1)``, ``axis_minor_length = 4 sqrt(l2)``, ``eccentricity = sqrt(1 - l2 / l1)`` and
    ``orientation = atan2(2 vxy, vxx - vyy) / 2`` in radians from +x toward +y, from the eigenvalues ``l1 >= l2`` of the
    second central moments in cell units (all 0 for a single cell).  Per ``ID``: ``event_duration``, ``event_cells_max``,
    ``event_time_of_max_cells`` (the first step reaching it), ``event_height_max``, ``event_width_max``,
    ``event_perimeter_max``, ``event_compactness_mean`` and ``event_eccentricity_mean`` (plain means over the present
    steps), ``event_coast_steps`` (steps with ``coast_edges > 0``), ``event_coast_share`` (sum of coast sides / sum of
    exposed sides) and the path of the centroid through the present steps in ascending time, gaps skipped:
    ``event_path_length``, ``event_displacement`` (first to last) and ``event_speed_mean`` (path length / (duration - 1),
    NaN for one step) -- in cell units with x the short way round unless ``regional_mode``, or with ``lat`` / ``lon`` in
    great-circle km (haversine on the centroids interpolated linearly in the coordinates, longitude periodic).

    The side-count perimeter and the orientation convention are this project's own definitions, not scikit-image's
    estimators.  The device sums integers only: every count is exact and the floats are float64 of exact integers."""
    return _event_shapes(ID_field, mask, cell_areas, edge_lengths, lat, lon, regional_mode, per_timestep, block_steps, device)
