"""Shape and movement of tracked events on an unstructured mesh of three-sided cells: perimeter, coastal contact, contact with
other events, axes on the sphere and the path of the centroid -- what :func:`marex_amd.shapes.event_shapes` gives on grids.

A mesh has no rows or columns, but it has cell sides (the three neighbour slots of the mesh tracker), a geometry (``lat``,
``lon``, ``cell_areas``) and the fixed-point contract of ``track_mesh.mesh_weight_tables`` that makes sums on it exact.  One
streaming pass on the device (``marex_mesh_event_shapes_i64``) adds, per (timestep, event), integers
only -- cells, the ten rows of a weight table, side counts and lengths, a box of integer coordinate keys -- into the compact
slots of ``event_intensity``.  The host turns the exact integers into the Dataset in float64.  The reference has nothing of
the kind; every definition here is this project's own.
"""
from __future__ import annotations

import math
from typing import Optional

import numpy as np

from ._stream import (_I32_MAX, _Windows, _check_block_steps, _dtype_name, _kind, _plan_windows, _time_of, event_spans,
                      pad_events, slot_index, tracker_time, walk_event_slots)
from .exceptions import TrackingError, create_data_validation_error
from .intensity import _time_of_max_values
from .shapes import _haversine_km
from .track import _host, _tensor_of
from .track_mesh import mesh_unit_vectors, mesh_weight_tables

KEY_BITS = 22  # the coordinate keys are rint(degrees * 2^22): |180 * 2^22| < 2^31
# columns of the device's ``mom`` (include/marex_hip.h); 1 .. 10 are the sums of the rows of q
_N, _S0, _S1, _S2, _S3, _SXX, _SYY, _SZZ, _SXY, _SXZ, _SYZ, _EEX, _EBD, _ECS, _LEN, _ECT = range(16)
_M32 = np.uint64(0xFFFFFFFF)


def mesh_shape_tables(cell_areas, lat, lon):
    """``(e, q)``: the fixed-point weights of the shape sums, ``q`` int64 ``[10, C]``, in NumPy float64 on the host.  Rows
    0 .. 3 are those of :func:`marex_amd.track_mesh.mesh_weight_tables` (``rint(a 2^e)`` and ``rint(a x 2^e)``, ``y``, ``z``
    with the unit vector ``(x, y, z)`` of a cell and ``e = 61 - ceil(log2(sum(a)))``); rows 4 .. 9 are ``rint(a (x x) 2^e)``,
    ``y y``, ``z z``, ``x y``, ``x z``, ``y z``.  Every ``|x_i x_j| <= 1``, so the sum of any row over any set of cells stays
    below 2^62 in magnitude.  Needs no GPU."""
    e, q4 = mesh_weight_tables(cell_areas, lat, lon)
    a = np.asarray(cell_areas, dtype=np.float64).reshape(-1)
    x, y, z = mesh_unit_vectors(lat, lon)
    q = np.empty((10, a.size), np.int64)
    q[:4] = q4
    for k, p in enumerate((x * x, y * y, z * z, x * y, x * z, y * z)):
        q[4 + k] = np.rint(np.ldexp(a * p, e))
    return e, q


def mesh_edge_weight_table(edge_lengths, C: int):
    """``(e_len, len_q int64 [3, C])``: the fixed-point side lengths, ``rint(v 2^e_len)`` with ``e_len = 61 -
    ceil(log2(sum(edge_lengths)))`` -- the rule of :func:`marex_amd.shapes.edge_weight_tables`: a sum over any set of sides,
    each counted once, stays below 2^62.  Needs no GPU."""
    v = np.asarray(_host(edge_lengths))
    if v.dtype.kind not in "fiu" or v.shape != (3, C):
        raise create_data_validation_error("edge_lengths must be numbers of shape (3, cells)",
                                           details=f"got {v.dtype} {v.shape}, the mesh has {C} cells")
    v = v.astype(np.float64)
    if not np.isfinite(v).all() or (v < 0).any():
        raise create_data_validation_error("edge_lengths must be finite and non-negative",
                                           details=f"{int((~np.isfinite(v)).sum())} non-finite, {int((v < 0).sum())} negative")
    total = float(v.sum())
    if not (total > 0 and np.isfinite(total)):
        raise create_data_validation_error("edge_lengths must have a positive, finite sum", details=f"sum {total}")
    e = 61 - int(np.ceil(np.log2(total)))
    return e, np.rint(np.ldexp(v, e)).astype(np.int64)


def coordinate_keys(lat, lon):
    """``(lat_k, lon_k)`` int32: ``rint(lat 2^22)`` and ``rint(lon_folded 2^22)`` of coordinates in degrees, with
    ``lon_folded = lon - 360 floor((lon + 180) / 360)`` (less 360 where that rounds to 180) in ``[-180, 180)``."""
    la, lo = np.asarray(lat, np.float64), np.asarray(lon, np.float64)
    f = lo - 360.0 * np.floor((lo + 180.0) / 360.0)
    f = np.where(f >= 180.0, f - 360.0, f)
    return np.rint(np.ldexp(la, KEY_BITS)).astype(np.int32), np.rint(np.ldexp(f, KEY_BITS)).astype(np.int32)


def _neighbours(neighbours, C: int, zero_based: bool):
    """int32 ``[3, C]``, 0-based, -1 for none, of the 1-based table of ``tracker(neighbours=)`` (0 or less: none), validated
    as the mesh tracker validates it; ``zero_based``: the tracker's own table, taken as it is."""
    nb = np.asarray(_host(neighbours))
    if nb.ndim != 2 or nb.shape[0] != 3 or nb.shape[1] != C:
        raise create_data_validation_error("Invalid neighbour array for triangular grid",
                                           details=f"Expected shape (3, {C}), got {nb.shape}",
                                           data_info={"actual_shape": tuple(nb.shape), "expected_shape": "(3, ncells)"})
    top = C - 1 if zero_based else C
    if nb.dtype.kind not in "iuf" or not np.isfinite(nb).all() or (nb != np.rint(nb)).any() or nb.max() > top:
        raise create_data_validation_error(
            "Invalid neighbour array for triangular grid",
            details=f"Expected whole {'0' if zero_based else '1'}-based cell numbers up to {top}, largest value {nb.max()}")
    nb = nb.astype(np.int64) - (0 if zero_based else 1)
    return np.ascontiguousarray(np.maximum(nb, -1).astype(np.int32))


def _validate(ID_field, neighbours, lat, lon, cell_areas, edge_lengths, mask, radius_km, zero_based: bool) -> dict:
    """Everything that can be refused without a device: the shape, the time axis and the host tables."""
    shape = tuple(int(k) for k in ID_field.shape)
    if len(shape) == 3:
        raise create_data_validation_error("mesh_event_shapes: ID_field must be (time, cells)",
                                           details=f"got a gridded field of shape {shape}: marex_amd.event_shapes measures grids")
    if len(shape) != 2:
        raise create_data_validation_error("ID_field must be (time, cells)", details=f"got shape {shape}")
    if _kind(ID_field) != "i":
        raise create_data_validation_error("Object IDs must be integers", details=f"Found dtype {_dtype_name(ID_field)}",
                                           data_info={"actual_dtype": _dtype_name(ID_field)})
    T, C = shape
    if C >= _I32_MAX or T >= _I32_MAX:
        raise TrackingError(f"mesh_event_shapes: a timestep of {C} cells or a record of {T} steps reaches 2^31 - 1",
                            details="the field may hold any number of cells, a single timestep and the time axis may not")
    if _tensor_of(ID_field) is None and T and C:
        h = np.asarray(ID_field.values if hasattr(ID_field, "values") else ID_field)
        lo = int(h.min())
        if lo < 0:
            raise create_data_validation_error("Object IDs must be non-negative", details=f"smallest ID {lo}; 0 is background",
                                               data_info={"min_id": lo, "max_id": int(h.max())})
    if not (isinstance(radius_km, (int, float, np.integer, np.floating)) and radius_km > 0 and math.isfinite(radius_km)):
        raise create_data_validation_error("radius_km must be positive", details=f"radius_km={radius_km!r}")
    tname, tv = _time_of(ID_field, T)
    p = {"T": T, "C": C, "tname": tname, "tv": tv if tv is not None else np.arange(T), "radius": float(radius_km),
         "mask": None, "edges": None}
    if lat is None or lon is None:
        raise create_data_validation_error("mesh_event_shapes needs lat and lon: a mesh has no other geometry")
    la, lo = np.asarray(_host(lat)), np.asarray(_host(lon))
    if la.dtype.kind not in "fiu" or lo.dtype.kind not in "fiu" or la.shape != (C,) or lo.shape != (C,):
        raise create_data_validation_error("lat and lon must be numbers, one per cell of the mesh",
                                           details=f"lat {la.dtype} {la.shape}, lon {lo.dtype} {lo.shape}, {C} cells")
    la, lo = la.astype(np.float64), lo.astype(np.float64)
    if not (np.isfinite(la).all() and np.isfinite(lo).all()) or (C and float(np.abs(la).max()) > 90.0):
        raise create_data_validation_error("lat and lon must be finite degrees with |lat| <= 90")
    p["nbr"] = _neighbours(neighbours, C, zero_based)
    if cell_areas is None:
        a = np.ones(C)
    else:
        a = np.asarray(_host(cell_areas))
        if a.dtype.kind not in "fiu" or a.shape != (C,):
            raise create_data_validation_error("cell_areas must be numbers, one per cell of the mesh",
                                               details=f"cell_areas {a.dtype} {a.shape}, {C} cells")
        a = a.astype(np.float64)
    if C:
        p["e"], p["q"] = mesh_shape_tables(a, la, lo)  # refuses areas that are negative, not finite or sum to zero
        p["lat_k"], p["lon_k"] = coordinate_keys(la, lo)
        if edge_lengths is not None:
            p["edges"] = mesh_edge_weight_table(edge_lengths, C)
    if mask is not None:
        m = np.asarray(_host(mask))
        if m.dtype != bool and m.dtype.kind not in "iu":
            raise create_data_validation_error("mask must be boolean (True: inside the domain)", details=f"Found dtype {m.dtype}")
        if m.shape != (C,):
            raise create_data_validation_error("mask does not match the cells of ID_field", details=f"mask {m.shape}, {C} cells")
        p["mask"] = np.ascontiguousarray(m != 0).view(np.uint8)
    return p


def _no_slots():
    return 0, np.zeros(1, np.int64), np.zeros(2, np.int64), np.zeros((0, 16), np.int64), np.zeros((0, 6), np.int32)


def _device_slots(eng, ID_field, p: dict, block_steps):
    """The two passes over the field: the events' spans, then the sums.  ``(N, tmin, off, mom, box)`` on the host."""
    T, C = p["T"], p["C"]
    ids_w = _Windows(eng, ID_field, T, C, np.int32, True)
    B = _plan_windows(eng, T, C, ids_w.upload_bytes_per_step, block_steps, "mesh_event_shapes",
                      f"the ID field of {T} timesteps of {C} cells, 4 bytes per cell, as far as it is not on the device already")
    N, tmin, tmax, wins, kept = event_spans(eng, ids_w, T, B)
    if N <= 0:
        return _no_slots()
    nbr, q = eng._dev(p["nbr"]), eng._dev(p["q"])
    dev = {"mask": None if p["mask"] is None else eng._dev(p["mask"]),
           "len_q": None if p["edges"] is None else eng._dev(p["edges"][1]),
           "lat_k": eng._dev(p["lat_k"]), "lon_k": eng._dev(p["lon_k"])}
    r = walk_event_slots(ids_w, wins, kept, lambda x, a, b, acc, finish: eng.mesh_event_shapes(
        x, nbr, q, tmin, tmax, t0=a, acc=acc, finish=finish, **dev))
    return N, tmin, r["off"], r["mom"], r["box"]


def _limbs(a, b):
    """The signed product ``a b`` of int64 vectors as four int64 limbs of 32 bits (least significant first), each carrying
    the product's sign: ``sum(limb[k] 2^(32 k))`` is the exact product.  From 32-bit halves of the magnitudes."""
    neg = (a < 0) ^ (b < 0)
    ua, ub = np.abs(a).astype(np.uint64), np.abs(b).astype(np.uint64)
    a0, a1, b0, b1 = ua & _M32, ua >> np.uint64(32), ub & _M32, ub >> np.uint64(32)
    p00, p01, p10, p11 = a0 * b0, a0 * b1, a1 * b0, a1 * b1
    mid = (p00 >> np.uint64(32)) + (p01 & _M32) + (p10 & _M32)
    top = p11 + (p01 >> np.uint64(32)) + (p10 >> np.uint64(32)) + (mid >> np.uint64(32))
    limbs = [p00 & _M32, mid & _M32, top & _M32, top >> np.uint64(32)]
    sign = np.where(neg, -1, 1).astype(np.int64)
    return [v.astype(np.int64) * sign for v in limbs]


def _carry(d):
    """The limbs with 0 <= d[k] < 2^32 for k < 3; the sign of the number is that of d[3]."""
    d = list(d)
    for k in range(3):
        d[k + 1] = d[k + 1] + (d[k] >> 32)  # the shift floors
        d[k] = d[k] & 0xFFFFFFFF
    return d


def exact_numerator(s0, sij, si, sj):
    """float64 of ``s0 sij - si sj`` for int64 vectors below 2^62 in magnitude: the 128-bit difference is formed exactly
    (64 x 64 -> 128 multiplies from 32-bit halves) and rounded once, to nearest-even, as ``float()`` of a Python integer."""
    s0, sij, si, sj = (np.asarray(v, np.int64) for v in (s0, sij, si, sj))
    d = _carry([u - v for u, v in zip(_limbs(s0, sij), _limbs(si, sj))])
    neg = d[3] < 0
    d = _carry([np.where(neg, -v, v) for v in d])  # the magnitude
    hi = (d[3].astype(np.uint64) << np.uint64(32)) | d[2].astype(np.uint64)  # < 2^62
    lo = (d[1].astype(np.uint64) << np.uint64(32)) | d[0].astype(np.uint64)
    small = hi == 0
    out = lo.astype(np.float64)
    if not small.all():
        h, lw = hi[~small], lo[~small]
        bl = np.frexp(h.astype(np.float64))[1].astype(np.int64)  # the bit length, or one more where the conversion rounded up
        bl = np.where((h >> (bl - 1).astype(np.uint64)) == 0, bl - 1, bl)
        s = (64 - bl).astype(np.uint64)  # 2 .. 63: the top 64 bits of the number, the bits below them kept as a sticky bit
        top = (h << s) | (lw >> (np.uint64(64) - s))
        top = top | ((lw << s) != 0).astype(np.uint64)
        out[~small] = np.ldexp(top.astype(np.float64), bl.astype(np.int64))
    return np.where(neg, -out, out)


def _centroid(s1, s2, s3):
    """``(phi, lam)`` in radians: the direction of the float64 vector, (0, 0) for a zero vector (the rule of
    ``track_mesh.mesh_moments_finish``, kept in float64)."""
    norm = np.sqrt(s1 * s1 + s2 * s2 + s3 * s3)
    norm = np.where(norm > 0, norm, 1.0)
    return np.arcsin(np.clip(s3 / norm, -1.0, 1.0)), np.arctan2(s2 / norm, s1 / norm)


def _fold_degrees(lon):
    return np.where(lon > 180.0, lon - 360.0, np.where(lon < -180.0, lon + 360.0, lon))


def _finish(p: dict, N: int, tmin, off, mom, box, per_timestep: bool):
    """The Dataset from the compact slots, in float64 from the exact integers and in ascending time per event."""
    from .xr_compat import DataArray, Dataset

    T, R = p["T"], p["radius"]
    tname, tcoord, tv = p["tname"], p["tcoord"], np.asarray(p["tv"])
    ids = np.arange(1, N + 1, dtype=np.int32)
    idc = {"ID": ("ID", ids)}
    tid = {tcoord or tname: (tname, tv), **idc}
    e_all, t_all = slot_index(off, tmin, N)
    mom = np.asarray(mom).astype(np.int64, copy=False).reshape(-1, 16)
    box = np.asarray(box).reshape(-1, 6)
    here = mom[:, _N] > 0
    e_of, t_of, m, bx = e_all[here], t_all[here], mom[here], box[here].astype(np.int64)
    n, s0 = m[:, _N], m[:, _S0]
    f = np.float64
    e = p.get("e", 0)
    area = np.ldexp(s0.astype(f), -e)
    phi, lam = _centroid(m[:, _S1].astype(f), m[:, _S2].astype(f), m[:, _S3].astype(f))
    clat, clon = np.degrees(phi), _fold_degrees(np.degrees(lam))
    # the box: exact keys; the longitude pair is the shorter of the direct arc and the arc across the date line
    has_w, has_e = bx[:, 2] <= bx[:, 3], bx[:, 4] <= bx[:, 5]
    lo_min = np.where(has_w, bx[:, 2], bx[:, 4])
    lo_max = np.where(has_e, bx[:, 5], bx[:, 3])
    direct = lo_max - lo_min
    wrapped = bx[:, 3] + (360 << KEY_BITS) - bx[:, 4]
    across = has_w & has_e & (wrapped < direct)  # a tie goes to the direct arc
    west = np.where(across, bx[:, 4], lo_min)
    width = np.where(across, wrapped, direct)
    # second moments on the sphere: exact numerators over float(S0)^2, projected onto the local frame at the centroid
    s0f2 = s0.astype(f) ** 2
    live = s0 > 0
    den = np.where(live, s0f2, 1.0)
    si = {"x": m[:, _S1], "y": m[:, _S2], "z": m[:, _S3]}
    M = {k: exact_numerator(s0, m[:, col], si[k[0]], si[k[1]]) / den
         for k, col in (("xx", _SXX), ("yy", _SYY), ("zz", _SZZ), ("xy", _SXY), ("xz", _SXZ), ("yz", _SYZ))}
    sp, cp, sl, cl = np.sin(phi), np.cos(phi), np.sin(lam), np.cos(lam)
    ex, ey = -sl, cl
    nx_, ny_, nz_ = -sp * cl, -sp * sl, cp
    vxx = ex * ex * M["xx"] + ey * ey * M["yy"] + 2.0 * (ex * ey * M["xy"])
    vyy = (nx_ * nx_ * M["xx"] + ny_ * ny_ * M["yy"] + nz_ * nz_ * M["zz"]
           + 2.0 * (nx_ * ny_ * M["xy"] + nx_ * nz_ * M["xz"] + ny_ * nz_ * M["yz"]))
    vxy = (ex * nx_ * M["xx"] + ey * ny_ * M["yy"] + (ex * ny_ + ey * nx_) * M["xy"] + ex * nz_ * M["xz"] + ey * nz_ * M["yz"])
    tr, root = vxx + vyy, np.hypot(vxx - vyy, 2.0 * vxy)
    l1 = (tr + root) / 2.0
    some = (l1 > 0) & (n > 1)  # a single cell, and a spread that is not positive, have no axes: all 0
    safe = np.where(some, l1, 1.0)
    l2 = np.maximum((vxx * vyy - vxy * vxy) / safe, 0.0)
    nan = np.where(live, 0.0, np.nan)  # no area: NaN
    major = np.where(some & live, 4.0 * np.sqrt(np.where(some, l1, 0.0)) * R, nan)
    minor = np.where(some & live, 4.0 * np.sqrt(np.where(some, l2, 0.0)) * R, nan)
    ecc = np.where(some & live, np.sqrt(np.minimum(root / safe, 1.0)), nan)
    orient = np.where(some & live, 0.5 * np.arctan2(2.0 * vxy, vxx - vyy), nan)
    # sides
    eex, ebd, ecs, ect = m[:, _EEX], m[:, _EBD], m[:, _ECS], m[:, _ECT]
    perim = np.ldexp(m[:, _LEN].astype(f), -p["edges"][0]) if p["edges"] is not None else eex.astype(f)
    with np.errstate(invalid="ignore", divide="ignore"):
        share = np.where(eex > 0, ecs / np.where(eex > 0, eex, 1), np.nan)
        compact = np.where(perim > 0, 4.0 * math.pi * area / np.where(perim > 0, perim * perim, 1.0), np.nan)
    data = {}
    if per_timestep:
        def dense(v, dt, fill):
            d = np.full((T, N), fill, dt)
            d[t_of, e_of - 1] = v
            return DataArray(d, dims=(tname, "ID"), coords=tid)

        key = lambda v: np.ldexp(v.astype(f), -KEY_BITS)  # noqa: E731
        for name, v, dt, fill in (
                ("cells", n, np.int64, 0), ("area", area, f, np.nan), ("centroid_lat", clat, f, np.nan),
                ("centroid_lon", clon, f, np.nan), ("bbox_lat_min", key(bx[:, 0]), f, np.nan),
                ("bbox_lat_max", key(bx[:, 1]), f, np.nan), ("bbox_lon_west", key(west), f, np.nan),
                ("bbox_lon_width", key(width), f, np.nan), ("edges", eex, np.int64, 0), ("border_edges", ebd, np.int64, 0),
                ("coast_edges", ecs, np.int64, 0), ("contact_edges", ect, np.int64, 0), ("perimeter", perim, f, np.nan),
                ("coast_share", share, f, np.nan), ("compactness", compact, f, np.nan),
                ("axis_major_length", major, f, np.nan), ("axis_minor_length", minor, f, np.nan),
                ("eccentricity", ecc, f, np.nan), ("orientation", orient, f, np.nan)):
            data[name] = dense(v, dt, fill)
    # per event; the rows of an event are in ascending time, and np.add.at adds one element after the other
    E = N + 1
    duration = np.bincount(e_of, minlength=E).astype(np.int32)
    has = duration > 0

    def emax(v, dt, fill):
        o = np.full(E, fill, dt)
        np.maximum.at(o, e_of, v.astype(dt))
        return o

    s0_max = emax(s0, np.int64, 0)
    first = np.full(E, np.iinfo(np.int64).max, np.int64)
    at_max = s0 == s0_max[e_of]
    np.minimum.at(first, e_of[at_max], t_of[at_max])

    def esum(v):
        o = np.zeros(E)
        np.add.at(o, e_of, v)
        return o

    with np.errstate(invalid="ignore", divide="ignore"):
        dur_f = np.where(has, duration, 1).astype(f)
        compact_mean = np.where(has, esum(compact) / dur_f, np.nan)
        ecc_mean = np.where(has, esum(ecc) / dur_f, np.nan)
        all_sides, all_coast = np.zeros(E, np.int64), np.zeros(E, np.int64)
        np.add.at(all_sides, e_of, eex)
        np.add.at(all_coast, e_of, ecs)
        coast_share = np.where(all_sides > 0, all_coast / np.where(all_sides > 0, all_sides, 1), np.nan)
    coast_steps = np.bincount(e_of[ecs > 0], minlength=E).astype(np.int32)
    # the path of the centroid: consecutive present steps of one event are consecutive rows
    pair = e_of[1:] == e_of[:-1]
    step = _haversine_km(clat[:-1], clon[:-1], clat[1:], clon[1:], R)
    path = np.zeros(E)
    np.add.at(path, e_of[1:][pair], step[pair])
    i_first, i_last = np.full(E, e_of.size, np.int64), np.full(E, -1, np.int64)
    np.minimum.at(i_first, e_of, np.arange(e_of.size))
    np.maximum.at(i_last, e_of, np.arange(e_of.size))
    disp = np.full(E, np.nan)
    if has.any():
        a, b = i_first[has], i_last[has]
        disp[has] = _haversine_km(clat[a], clon[a], clat[b], clon[b], R)
    with np.errstate(invalid="ignore", divide="ignore"):
        speed = np.where(duration > 1, path / np.where(duration > 1, duration - 1, 1), np.nan)
    for name, v in (("event_duration", duration[1:]), ("event_cells_max", emax(n, np.int64, 0)[1:]),
                    ("event_area_max", np.where(has, np.ldexp(s0_max.astype(f), -e), np.nan)[1:]),
                    ("event_time_of_max_area", _time_of_max_values(tv, first[1:], has[1:])),
                    ("event_perimeter_max", np.where(has, emax(perim, f, -np.inf), np.nan)[1:]),
                    ("event_compactness_mean", compact_mean[1:]), ("event_eccentricity_mean", ecc_mean[1:]),
                    ("event_coast_steps", coast_steps[1:]), ("event_coast_share", coast_share[1:]),
                    ("event_path_length", np.where(has, path, np.nan)[1:]), ("event_displacement", disp[1:]),
                    ("event_speed_mean", speed[1:])):
        data[name] = DataArray(v, dims=("ID",), coords=idc)
    ds = Dataset(data, coords=tid)
    ds.attrs["distance_units"] = "km"
    ds.attrs["perimeter_units"] = "km" if p["edges"] is not None else "sides"
    return ds


def _mesh_event_shapes(ID_field, neighbours, lat, lon, cell_areas, edge_lengths, mask, radius_km, per_timestep, block_steps,
                       device, zero_based: bool = False, n_events: Optional[int] = None, time: Optional[tuple] = None):
    block_steps = _check_block_steps(block_steps)
    p = _validate(ID_field, neighbours, lat, lon, cell_areas, edge_lengths, mask, radius_km, zero_based)
    tracker_time(p, time)
    if p["T"] == 0 or p["C"] == 0:
        N, tmin, off, mom, box = _no_slots()
    else:
        from .detect import get_engine

        N, tmin, off, mom, box = _device_slots(get_engine(device), ID_field, p, block_steps)
    N, tmin, off = pad_events("mesh_event_shapes", N, n_events, tmin, off)
    return _finish(p, N, tmin, off, mom, box, bool(per_timestep))


def mesh_event_shapes(ID_field, neighbours, lat, lon, cell_areas=None, edge_lengths=None, mask=None, radius_km: float = 6371.0,
                      per_timestep: bool = True, block_steps=None, device: int = 0):
    """What shape every tracked event has on an unstructured mesh, how much of its edge lies on the coast or against other
    events and how far it moves, from one pass over a ``(time, cells)`` event field on the device.

    ``ID_field``: an integer ``(time, cells)`` event field of the basic or the merge mesh tracker, a host array or DataArray
    or device resident (then it is read in place); the positive values are the event numbers, a negative value is refused
    on the host path.  A gridded ``(time, y, x)`` field is refused: :func:`marex_amd.event_shapes` measures grids.
    ``neighbours``: ``(3, cells)``, 1-based, 0 or less for "none", as ``tracker(neighbours=)`` takes it.  ``lat`` / ``lon``:
    degrees, one per cell, finite, ``|lat| <= 90``.  ``cell_areas``: non-negative, one per cell (None: unit areas).
    ``edge_lengths``: non-negative ``[3, cells]``, entry ``[k, c]`` the length of the side of cell ``c`` that faces its k-th
    listed neighbour (on ICON meshes ``edge_length`` through ``edge_of_cell``); None: every side counts 1.  ``mask``: boolean
    ``[cells]``, True inside the domain.  ``block_steps`` as in :func:`marex_amd.event_intensity`; the results do not depend
    on it.

    **Exposed side.**  Side ``k`` of a cell ``c`` of event ``e`` at step ``t``, with ``j = neighbours[k][c]``: without a
    neighbour it is exposed and a ``border_edge``; otherwise it is exposed when ``ID_field[t][j] != e`` as the value stands
    (0 and any other number differ).  An exposed side is a ``coast_edge`` when ``mask[j]`` is False and a ``contact_edge``
    when ``ID_field[t][j] > 0`` (it faces another event).  Each slot is tested on its own: a neighbour listed twice counts
    twice, and a side between two events counts once for each.

    **Weights.**  :func:`mesh_shape_tables` (areas and area-weighted first and second powers of the cells' unit vectors,
    int64 fixed point, no sum reaches 2^62) and :func:`mesh_edge_weight_table`; the device adds integers only.

    **Box.**  From the integer keys of :func:`coordinate_keys`: ``bbox_lat_min``, ``bbox_lat_max``, and ``bbox_lon_west`` /
    ``bbox_lon_width``, the shorter of two covering arcs -- the direct one from the smallest to the largest folded longitude
    and the one across the date line, from the smallest non-negative longitude to the largest negative one plus 360 degrees
    (a tie goes to the direct arc).  All four are ``ldexp(integer, -22)``, hence exact.  It is the shorter of these two arcs,
    not the minimal covering arc, and the longitude box of an event that lies over a pole is meaningless.

    **Axes.**  With ``S0`` the sum of row 0, ``S_i`` of rows 1 .. 3 and ``S_ij`` of rows 4 .. 9, the numerators ``N_ij = S0
    S_ij - S_i S_j`` are formed exactly (they reach 2^124), rounded to float64 once and divided by ``float(S0)^2``: the
    symmetric matrix ``M``.  The centroid ``(phi_c, lambda_c)`` is the direction of ``(S1, S2, S3)`` in float64 ((0, 0) for
    a zero vector; the rule of ``mesh_moments_finish`` without its rounding to float32).  With east ``(-sin lambda_c, cos
    lambda_c, 0)`` and north ``(-sin phi_c cos lambda_c, -sin phi_c sin lambda_c, cos phi_c)``: ``vxx = e M e``, ``vyy = n M
    n``, ``vxy = e M n``, ``tr = vxx + vyy``, ``root = hypot(vxx - vyy, 2 vxy)``, ``l1 = (tr + root) / 2``, ``l2 = max((vxx
    vyy - vxy^2) / l1, 0)``; ``axis_major_length = 4 sqrt(l1) radius_km``, ``axis_minor_length = 4 sqrt(l2) radius_km``,
    ``eccentricity = sqrt(min(root / l1, 1))`` and ``orientation = atan2(2 vxy, vxx - vyy) / 2`` in radians from east
    toward north.  All four are 0 for a single cell (and where ``l1`` is not positive) and NaN where ``S0 == 0``.  This is a
    tangent-plane (chord) measure: it understates arcs by O(theta^2) for an event of angular radius theta.

    **Path.**  Great-circle km (haversine with ``radius_km``) between the float64 centroids of consecutive present steps of
    an event, gaps skipped.

    Returns a Dataset over ``time`` and ``ID = 1 .. N``.  With ``per_timestep``, dense ``(time, ID)``, where the event is
    absent NaN and 0 for counts: ``cells``, ``area``, ``centroid_lat``, ``centroid_lon``, ``bbox_lat_min``, ``bbox_lat_max``,
    ``bbox_lon_west``, ``bbox_lon_width``, ``edges`` (exposed sides), ``border_edges``, ``coast_edges``, ``contact_edges``,
    ``perimeter`` (the exposed sides, or with ``edge_lengths`` their length), ``coast_share = coast_edges / edges``,
    ``compactness = 4 pi area / perimeter^2`` (meaningful where both are physical), ``axis_major_length``,
    ``axis_minor_length``, ``eccentricity``, ``orientation``.  Per ``ID``: ``event_duration``, ``event_cells_max``,
    ``event_area_max``, ``event_time_of_max_area`` (the first step reaching the largest integer ``S0``),
    ``event_perimeter_max``, ``event_compactness_mean`` and ``event_eccentricity_mean`` (plain means over the present
    steps), ``event_coast_steps``, ``event_coast_share`` (sum of coast sides / sum of exposed sides), ``event_path_length``,
    ``event_displacement`` (first to last) and ``event_speed_mean`` (path length / (duration - 1), NaN for one step).
    Attributes: ``distance_units = "km"``; ``perimeter_units`` "km" with ``edge_lengths``, else "sides"."""
    return _mesh_event_shapes(ID_field, neighbours, lat, lon, cell_areas, edge_lengths, mask, radius_km, per_timestep,
                              block_steps, device)
