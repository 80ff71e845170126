"""A brute-force oracle of ``marex_amd.mesh_event_shapes``: per (timestep, event) plain Python loops over the cells, the
tables restated from the formulas of the contract, every sum and every numerator in Python integers, the float64 formulas as
the docstring writes them, with ``math``.  Shares no code with marex_amd/shapes_mesh.py.  Not collected by pytest."""
import math

import numpy as np

INT_KEYS = ["cells", "edges", "border_edges", "coast_edges", "contact_edges"]
EXACT_KEYS = ["area", "bbox_lat_min", "bbox_lat_max", "bbox_lon_west", "bbox_lon_width", "perimeter"]  # ldexp of exact integers
FLOAT_KEYS = ["centroid_lat", "centroid_lon", "coast_share", "compactness", "axis_major_length", "axis_minor_length",
              "eccentricity", "orientation"]
EVENT_INT_KEYS = ["event_duration", "event_cells_max", "event_coast_steps"]
EVENT_EXACT_KEYS = ["event_area_max", "event_perimeter_max"]
EVENT_FLOAT_KEYS = ["event_compactness_mean", "event_eccentricity_mean", "event_coast_share", "event_path_length",
                    "event_displacement", "event_speed_mean"]
TOL = 1e-12
KEY = 22


def weight_rows(areas, lat, lon):
    """``(e, rows)``: ten lists of Python integers."""
    a = np.asarray(areas, np.float64)
    phi, lam = np.radians(np.asarray(lat, np.float64)), np.radians(np.asarray(lon, np.float64))
    x, y, z = np.cos(phi) * np.cos(lam), np.cos(phi) * np.sin(lam), np.sin(phi)
    e = 61 - int(np.ceil(np.log2(float(a.sum()))))
    rows = [a, a * x, a * y, a * z, a * (x * x), a * (y * y), a * (z * z), a * (x * y), a * (x * z), a * (y * z)]
    return e, [[int(v) for v in np.rint(np.ldexp(r, e))] for r in rows]


def length_rows(edge_lengths):
    v = np.asarray(edge_lengths, np.float64)
    e = 61 - int(np.ceil(np.log2(float(v.sum()))))
    return e, [[int(u) for u in np.rint(np.ldexp(r, e))] for r in v]


def keys(lat, lon):
    lo = np.asarray(lon, np.float64)
    f = lo - 360.0 * np.floor((lo + 180.0) / 360.0)
    f = np.where(f >= 180.0, f - 360.0, f)
    return ([int(v) for v in np.rint(np.asarray(lat, np.float64) * 2.0 ** KEY)], [int(v) for v in np.rint(f * 2.0 ** KEY)])


def haversine(la1, lo1, la2, lo2, radius):
    p1, p2 = math.radians(la1), math.radians(la2)
    s1, s2 = math.sin((p2 - p1) / 2.0), math.sin(math.radians(lo2 - lo1) / 2.0)
    a = s1 * s1 + math.cos(p1) * math.cos(p2) * (s2 * s2)
    return 2.0 * radius * math.asin(min(1.0, math.sqrt(a)))


def slot(cells, row, e_id, nbr0, q, len_q, e, e_len, mask, lat_k, lon_k, radius):
    """One (timestep, event): ``cells`` its cell numbers, ``row`` the slice."""
    C = len(row)
    S = [sum(q[i][c] for c in cells) for i in range(10)]
    edges = border = coast = contact = length = 0
    for c in cells:
        for k in range(3):
            j = int(nbr0[k][c])
            if j < 0 or j >= C:
                edges, border = edges + 1, border + 1
            elif int(row[j]) != e_id:
                edges += 1
                coast += int(mask is not None and not mask[j])
                contact += int(row[j] > 0)
            else:
                continue
            if len_q is not None:
                length += len_q[k][c]
    r = {"cells": len(cells), "edges": edges, "border_edges": border, "coast_edges": coast, "contact_edges": contact, "S0": S[0]}
    r["area"] = math.ldexp(float(S[0]), -e)
    r["perimeter"] = math.ldexp(float(length), -e_len) if len_q is not None else float(edges)
    r["coast_share"] = coast / edges if edges else math.nan
    r["compactness"] = 4.0 * math.pi * r["area"] / (r["perimeter"] * r["perimeter"]) if r["perimeter"] > 0 else math.nan
    # box
    la = [lat_k[c] for c in cells]
    west, east = [lon_k[c] for c in cells if lon_k[c] < 0], [lon_k[c] for c in cells if lon_k[c] >= 0]
    lo = west + east
    w0, width = min(lo), max(lo) - min(lo)
    if west and east and max(west) + 360 * 2 ** KEY - min(east) < width:
        w0, width = min(east), max(west) + 360 * 2 ** KEY - min(east)
    for name, v in (("bbox_lat_min", min(la)), ("bbox_lat_max", max(la)), ("bbox_lon_west", w0), ("bbox_lon_width", width)):
        r[name] = math.ldexp(float(v), -KEY)
    # centroid
    s1, s2, s3 = float(S[1]), float(S[2]), float(S[3])
    norm = math.sqrt(s1 * s1 + s2 * s2 + s3 * s3)
    norm = norm if norm > 0 else 1.0
    phi, lam = math.asin(max(-1.0, min(1.0, s3 / norm))), math.atan2(s2 / norm, s1 / norm)
    r["centroid_lat"], r["centroid_lon"] = math.degrees(phi), math.degrees(lam)
    if r["centroid_lon"] > 180.0:
        r["centroid_lon"] -= 360.0
    # axes
    r["tr"] = r["root"] = math.nan
    if S[0] == 0:
        for k in ("axis_major_length", "axis_minor_length", "eccentricity", "orientation"):
            r[k] = math.nan
        return r
    pos = {(0, 0): 4, (1, 1): 5, (2, 2): 6, (0, 1): 7, (0, 2): 8, (1, 2): 9}
    M = [[0.0] * 3 for _ in range(3)]
    for (i, j), col in pos.items():
        M[i][j] = M[j][i] = float(S[0] * S[col] - S[1 + i] * S[1 + j]) / (float(S[0]) ** 2)
    east_v = (-math.sin(lam), math.cos(lam), 0.0)
    north_v = (-math.sin(phi) * math.cos(lam), -math.sin(phi) * math.sin(lam), math.cos(phi))
    quad = lambda u, v: sum(u[i] * M[i][j] * v[j] for i in range(3) for j in range(3))  # noqa: E731
    vxx, vyy, vxy = quad(east_v, east_v), quad(north_v, north_v), quad(east_v, north_v)
    tr, root = vxx + vyy, math.hypot(vxx - vyy, 2.0 * vxy)
    l1 = (tr + root) / 2.0
    if len(cells) == 1 or not l1 > 0:
        for k in ("axis_major_length", "axis_minor_length", "eccentricity", "orientation"):
            r[k] = 0.0
        return r
    l2 = max((vxx * vyy - vxy * vxy) / l1, 0.0)
    r.update(axis_major_length=4.0 * math.sqrt(l1) * radius, axis_minor_length=4.0 * math.sqrt(l2) * radius,
             eccentricity=math.sqrt(min(root / l1, 1.0)), orientation=math.atan2(2.0 * vxy, vxx - vyy) / 2.0, tr=tr, root=root)
    return r


def mesh_event_shapes(ids, nbr0, lat, lon, cell_areas=None, edge_lengths=None, mask=None, radius_km=6371.0, n_events=None):
    """``(steps, events)``: ``steps[(t, e)]`` and ``events[e]`` for e = 1 .. N (the largest number in the field, or
    ``n_events``).  ``nbr0``: 0-based, a value outside 0 .. C - 1 is no neighbour."""
    ids = np.asarray(ids)
    T, C = ids.shape
    e, q = weight_rows(np.ones(C) if cell_areas is None else cell_areas, lat, lon)
    e_len, len_q = length_rows(edge_lengths) if edge_lengths is not None else (0, None)
    lat_k, lon_k = keys(lat, lon)
    N = int(ids.max()) if n_events is None else n_events
    steps = {}
    for t in range(T):
        for ev in sorted(set(int(v) for v in ids[t] if v > 0)):
            cells = [c for c in range(C) if ids[t][c] == ev]
            steps[(t, ev)] = slot(cells, ids[t], ev, nbr0, q, len_q, e, e_len, mask, lat_k, lon_k, radius_km)
    events = {}
    for ev in range(1, N + 1):
        ts = [t for t in range(T) if (t, ev) in steps]
        rows = [steps[(t, ev)] for t in ts]
        r = {"event_duration": len(ts), "event_cells_max": max((x["cells"] for x in rows), default=0),
             "event_coast_steps": sum(1 for x in rows if x["coast_edges"] > 0), "event_time_of_max_area": None}
        for k in EVENT_EXACT_KEYS + EVENT_FLOAT_KEYS:
            r[k] = math.nan
        if rows:
            top = max(x["S0"] for x in rows)
            r["event_time_of_max_area"] = next(t for t, x in zip(ts, rows) if x["S0"] == top)
            r["event_area_max"] = math.ldexp(float(top), -e)
            r["event_perimeter_max"] = max(x["perimeter"] for x in rows)
            cm = em = 0.0
            for x in rows:
                cm, em = cm + x["compactness"], em + x["eccentricity"]
            r["event_compactness_mean"], r["event_eccentricity_mean"] = cm / len(rows), em / len(rows)
            sides, coast = sum(x["edges"] for x in rows), sum(x["coast_edges"] for x in rows)
            r["event_coast_share"] = coast / sides if sides else math.nan
            path = 0.0
            for a, b in zip(rows[:-1], rows[1:]):
                path += haversine(a["centroid_lat"], a["centroid_lon"], b["centroid_lat"], b["centroid_lon"], radius_km)
            r["event_path_length"] = path
            r["event_displacement"] = haversine(rows[0]["centroid_lat"], rows[0]["centroid_lon"], rows[-1]["centroid_lat"],
                                                rows[-1]["centroid_lon"], radius_km)
            r["event_speed_mean"] = path / (len(rows) - 1) if len(rows) > 1 else math.nan
        events[ev] = r
    return steps, events


def _close(got, exp, tol, what):
    if math.isnan(exp):
        assert math.isnan(got), (what, got, exp)
    else:
        assert abs(got - exp) <= tol, (what, got, exp, tol)


def compare(ds, steps, events, T, tvals=None):
    """The Dataset against the oracle: integers and ldexp values with ==, the other floats within ``TOL`` -- relative; the
    squared axis lengths relative to the squared major axis; the orientation absolute at ``TOL tr / root``, skipped where
    ``root == 0``."""
    N = len(events)
    assert list(np.asarray(ds["ID"].values)) == list(range(1, N + 1))
    tv = np.arange(T) if tvals is None else np.asarray(tvals)
    if "cells" in ds.data_vars:
        val = {k: np.asarray(ds[k].values) for k in INT_KEYS + EXACT_KEYS + FLOAT_KEYS}
        for k, v in val.items():
            assert v.shape == (T, N) and v.dtype == (np.int64 if k in INT_KEYS else np.float64), k
        for t in range(T):
            for ev in range(1, N + 1):
                r = steps.get((t, ev))
                what = (t, ev)
                if r is None:
                    assert all(val[k][t, ev - 1] == 0 for k in INT_KEYS), what
                    assert all(np.isnan(val[k][t, ev - 1]) for k in EXACT_KEYS + FLOAT_KEYS), what
                    continue
                for k in INT_KEYS:
                    assert val[k][t, ev - 1] == r[k], (what, k, val[k][t, ev - 1], r[k])
                for k in EXACT_KEYS:
                    assert val[k][t, ev - 1] == r[k], (what, k, val[k][t, ev - 1], r[k])
                for k in ("centroid_lat", "centroid_lon", "coast_share", "compactness", "eccentricity"):
                    _close(float(val[k][t, ev - 1]), r[k], TOL * abs(r[k]), (what, k))
                major2 = r["axis_major_length"] ** 2
                for k in ("axis_major_length", "axis_minor_length"):
                    got = float(val[k][t, ev - 1])
                    _close(got * got, r[k] ** 2, TOL * major2, (what, k))
                if not (r["root"] == 0):
                    tol = TOL * r["tr"] / r["root"] if r["root"] > 0 else 0.0
                    _close(float(val["orientation"][t, ev - 1]), r["orientation"], tol, (what, "orientation"))
    tmax = np.asarray(ds["event_time_of_max_area"].values)
    for ev in range(1, N + 1):
        r = events[ev]
        for k in EVENT_INT_KEYS:
            assert int(np.asarray(ds[k].values)[ev - 1]) == r[k], (ev, k)
        for k in EVENT_EXACT_KEYS:
            got = float(np.asarray(ds[k].values)[ev - 1])
            assert got == r[k] or (math.isnan(got) and math.isnan(r[k])), (ev, k, got, r[k])
        for k in EVENT_FLOAT_KEYS:
            _close(float(np.asarray(ds[k].values)[ev - 1]), r[k], TOL * abs(r[k]), (ev, k))
        if r["event_time_of_max_area"] is None:
            assert np.isnat(tmax[ev - 1]) if tmax.dtype.kind in "mM" else np.isnan(tmax[ev - 1]), ev
        else:
            assert tmax[ev - 1] == tv[r["event_time_of_max_area"]], (ev, tmax[ev - 1])
