"""Brute-force oracle of ``marex_amd.event_shapes``: per (timestep, ID) ``np.nonzero``, four explicit neighbour comparisons
per cell in a Python loop, Python integers for every sum and ``fractions.Fraction`` up to the final ``math.sqrt`` /
``math.atan2``.  Shares no code with marex_amd/shapes.py.  Not collected by pytest."""
import math
from fractions import Fraction

import numpy as np

INT_KEYS = ("cells", "bbox_y0", "bbox_x0", "bbox_height", "bbox_width", "edges_ns", "edges_ew", "border_edges", "coast_edges")
FLOAT_KEYS = ("area", "extent", "perimeter", "coast_share", "compactness", "centroid_y", "centroid_x", "axis_major_length",
              "axis_minor_length", "eccentricity", "orientation")
EVENT_INT_KEYS = ("event_duration", "event_cells_max", "event_time_of_max_cells", "event_height_max", "event_width_max",
                  "event_coast_steps")
EVENT_FLOAT_KEYS = ("event_perimeter_max", "event_compactness_mean", "event_eccentricity_mean", "event_coast_share",
                    "event_path_length", "event_displacement", "event_speed_mean")


def _ceil_log2(fr: Fraction) -> int:
    """The smallest integer k with fr <= 2^k, exactly."""
    k = fr.numerator.bit_length() - fr.denominator.bit_length()
    while Fraction(2) ** k < fr:
        k += 1
    while Fraction(2) ** (k - 1) >= fr:
        k -= 1
    return k


def _quantise(values, total: Fraction):
    """(e, [round-half-even(v 2^e)]) with e = 61 - ceil(log2(total)): sums of the integers stay below 2^62."""
    e = 61 - _ceil_log2(total)
    return e, [round(Fraction(float(v)) * Fraction(2) ** e) for v in values]


def quantise_areas(cell_areas):
    flat = [float(v) for v in np.asarray(cell_areas, dtype=np.float64).reshape(-1)]
    return _quantise(flat, sum((Fraction(v) for v in flat), Fraction(0)))


def quantise_edges(ns_len, ew_len, nx: int):
    ns, ew = [float(v) for v in ns_len], [float(v) for v in ew_len]
    total = nx * sum((Fraction(v) for v in ns), Fraction(0)) + (nx + 1) * sum((Fraction(v) for v in ew), Fraction(0))
    e, q = _quantise(ns + ew, total)
    return e, q[:len(ns)], q[len(ns):]


def grid_edge_lengths(lat, lon, radius_km=6371.0):
    ny, nx = len(lat), len(lon)
    edge = [0.0] * (ny + 1)
    for j in range(1, ny):
        edge[j] = 0.5 * (lat[j - 1] + lat[j])
    if ny > 1:
        edge[0] = lat[0] - 0.5 * (lat[1] - lat[0])
        edge[ny] = lat[ny - 1] + 0.5 * (lat[ny - 1] - lat[ny - 2])
    else:
        w = abs(lon[1] - lon[0]) if nx > 1 else 1.0
        edge[0], edge[1] = lat[0] - 0.5 * w, lat[0] + 0.5 * w
    edge = [min(90.0, max(-90.0, v)) for v in edge]
    dlam = abs(lon[-1] - lon[0]) / (nx - 1) if nx > 1 else 360.0
    k = math.pi / 180.0
    return ([max(radius_km * math.cos(v * k) * (dlam * k), 0.0) for v in edge],
            [radius_km * abs(edge[j + 1] - edge[j]) * k for j in range(ny)])


def step_shape(sl, e, mask=None, regional=False, areas=None, edges=None):
    """One (timestep, ID): a dict of Python integers and float64 values, or None where the ID has no cell."""
    ny, nx = sl.shape
    ys, xs = np.nonzero(sl == e)
    if ys.size == 0:
        return None
    ys, xs = [int(v) for v in ys], [int(v) for v in xs]
    n = len(ys)
    e_ns = e_ew = border = coast = 0
    length = 0
    for y, x in zip(ys, xs):
        for dy_, dx_ in ((-1, 0), (1, 0), (0, -1), (0, 1)):
            yy, xx = y + dy_, x + dx_
            outside = yy < 0 or yy >= ny
            if dx_:
                if regional:
                    outside = xx < 0 or xx >= nx
                else:
                    xx %= nx
            if not outside and int(sl[yy, xx]) == e:
                continue
            if dy_:
                e_ns += 1
            else:
                e_ew += 1
            if outside:
                border += 1
            elif mask is not None and not mask[yy, xx]:
                coast += 1
            if edges is not None:
                length += edges[1][y if dy_ < 0 else y + 1] if dy_ else edges[2][y]
    wrapped = (not regional) and any(x < 100 for x in xs) and any(x >= nx - 100 for x in xs)
    xp = [x - nx if (wrapped and x > nx // 2) else x for x in xs]
    sy, sx = sum(ys), sum(xp)
    cx = float(Fraction(sx, n))
    if cx < 0:
        cx = cx + nx
    height, width = max(ys) - min(ys) + 1, max(xp) - min(xp) + 1
    out = {"cells": n, "bbox_y0": min(ys), "bbox_x0": min(xp) % nx, "bbox_height": height, "bbox_width": width,
           "edges_ns": e_ns, "edges_ew": e_ew, "border_edges": border, "coast_edges": coast,
           "centroid_y": float(Fraction(sy, n)), "centroid_x": cx, "extent": float(Fraction(n, height * width)),
           "coast_share": float(Fraction(coast, e_ns + e_ew))}
    area = Fraction(n) if areas is None else Fraction(sum(areas[1][y * nx + x] for y, x in zip(ys, xs))) / Fraction(2) ** areas[0]
    perim = Fraction(e_ns + e_ew) if edges is None else Fraction(length) / Fraction(2) ** edges[0]
    out["area"], out["perimeter"] = float(area), float(perim)
    out["compactness"] = 4.0 * math.pi * out["area"] / (out["perimeter"] * out["perimeter"]) if perim > 0 else math.nan
    vyy = Fraction(sum(y * y for y in ys), n) - Fraction(sy, n) ** 2
    vxx = Fraction(sum(x * x for x in xp), n) - Fraction(sx, n) ** 2
    vxy = Fraction(sum(x * y for x, y in zip(xp, ys)), n) - Fraction(sx, n) * Fraction(sy, n)
    disc = (vxx - vyy) ** 2 + 4 * vxy ** 2
    root = math.sqrt(disc)
    l1 = (float(vxx + vyy) + root) / 2.0
    if l1 > 0:
        l2 = float(vxx * vyy - vxy ** 2) / l1
        out["axis_major_length"], out["axis_minor_length"] = 4.0 * math.sqrt(l1), 4.0 * math.sqrt(max(l2, 0.0))
        out["eccentricity"] = math.sqrt(min(root / l1, 1.0))  # 1 - l2 / l1 = (l1 - l2) / l1
        out["orientation"] = 0.5 * math.atan2(float(2 * vxy), float(vxx - vyy))
    else:
        out["axis_major_length"] = out["axis_minor_length"] = out["eccentricity"] = out["orientation"] = 0.0
    return out


def _distance(a, b, nx, regional, lat, lon):
    (y1, x1), (y2, x2) = a, b
    if lat is None:
        dy, dx = y2 - y1, abs(x2 - x1)
        if not regional:
            dx = min(dx, nx - dx)
        return math.sqrt(dy * dy + dx * dx)

    def place(cy, cx):
        i0 = min(max(int(math.floor(cy)), 0), len(lat) - 1)
        i1 = min(i0 + 1, len(lat) - 1)
        j0 = min(max(int(math.floor(cx)), 0), len(lon) - 1)
        j1 = (j0 + 1) % len(lon)
        d = float(lon[j1]) - float(lon[j0])
        d = d - 360.0 * round(d / 360.0)
        return float(lat[i0]) + (cy - i0) * (float(lat[i1]) - float(lat[i0])), float(lon[j0]) + (cx - j0) * d

    k = math.pi / 180.0
    (la1, lo1), (la2, lo2) = place(y1, x1), place(y2, x2)
    p1, p2 = la1 * k, la2 * k
    s1, s2 = math.sin((p2 - p1) / 2.0), math.sin(((lo2 - lo1) * k) / 2.0)
    h = s1 * s1 + math.cos(p1) * math.cos(p2) * (s2 * s2)
    return 2.0 * 6371.0 * math.asin(min(1.0, math.sqrt(h)))


def event_shapes(ids, mask=None, cell_areas=None, edge_lengths=None, lat=None, lon=None, regional_mode=False):
    """``(steps, events)``: ``steps[(t, e)]`` the dict of :func:`step_shape`, ``events[e]`` the per-event dict, e = 1 .. max."""
    ids = np.asarray(ids)
    T, ny, nx = ids.shape
    N = int(ids.max()) if ids.size else 0
    areas = None
    if cell_areas is not None:
        a = np.asarray(cell_areas, np.float64)
        if a.shape == (ny,) and nx > 1:
            a = np.repeat(a[:, None], nx, axis=1)
        areas = quantise_areas(a.reshape(ny, nx))
    edges = None if edge_lengths is None else quantise_edges(edge_lengths[0], edge_lengths[1], nx)
    steps, events = {}, {}
    for t in range(T):
        for e in (int(v) for v in np.unique(ids[t]) if v > 0):
            steps[(t, e)] = step_shape(ids[t], e, mask, regional_mode, areas, edges)
    for e in range(1, N + 1):
        ts = sorted(t for (t, k) in steps if k == e)
        ev = {"event_duration": len(ts)}
        rows = [steps[(t, e)] for t in ts]
        ev["event_cells_max"] = max((r["cells"] for r in rows), default=0)
        ev["event_time_of_max_cells"] = next((t for t, r in zip(ts, rows) if r["cells"] == ev["event_cells_max"]), None)
        ev["event_height_max"] = max((r["bbox_height"] for r in rows), default=0)
        ev["event_width_max"] = max((r["bbox_width"] for r in rows), default=0)
        ev["event_coast_steps"] = sum(1 for r in rows if r["coast_edges"] > 0)
        if not rows:
            for k in EVENT_FLOAT_KEYS:
                ev[k] = math.nan
            events[e] = ev
            continue
        ev["event_perimeter_max"] = max(r["perimeter"] for r in rows)
        acc_c = acc_e = 0.0
        for r in rows:  # ascending time
            acc_c += r["compactness"]
            acc_e += r["eccentricity"]
        ev["event_compactness_mean"], ev["event_eccentricity_mean"] = acc_c / len(rows), acc_e / len(rows)
        ev["event_coast_share"] = float(Fraction(sum(r["coast_edges"] for r in rows),
                                                 sum(r["edges_ns"] + r["edges_ew"] for r in rows)))
        pts = [(r["centroid_y"], r["centroid_x"]) for r in rows]
        path = 0.0
        for a, b in zip(pts[:-1], pts[1:]):
            path += _distance(a, b, nx, regional_mode, lat, lon)
        ev["event_path_length"] = path
        ev["event_displacement"] = _distance(pts[0], pts[-1], nx, regional_mode, lat, lon)
        ev["event_speed_mean"] = path / (len(rows) - 1) if len(rows) > 1 else math.nan
        events[e] = ev
    return steps, events


def compare(ds, steps, events, T, per_timestep=True, rtol=1e-12, tvals=None):
    """Assert that the Dataset of ``marex_amd.event_shapes`` equals the oracle: integers with ==, floats within ``rtol``
    relative (absolute for the orientation), NaN where NaN."""
    N = len(events)
    assert np.asarray(ds["ID"].values).tolist() == list(range(1, N + 1))

    def close(got, exp, name, where):
        if math.isnan(exp):
            assert math.isnan(got), (name, where, got, exp)
        elif name == "orientation":
            assert abs(got - exp) <= rtol, (name, where, got, exp)
        else:
            assert abs(got - exp) <= rtol * abs(exp), (name, where, got, exp)

    if per_timestep:
        arrays = {k: np.asarray(ds[k].values) for k in INT_KEYS + FLOAT_KEYS}
        for k in INT_KEYS:
            assert arrays[k].dtype.kind == "i" and arrays[k].shape == (T, N), k
        for t in range(T):
            for e in range(1, N + 1):
                r = steps.get((t, e))
                if r is None:
                    for k in INT_KEYS:
                        assert int(arrays[k][t, e - 1]) == (-1 if k in ("bbox_y0", "bbox_x0") else 0), (k, t, e)
                    for k in FLOAT_KEYS:
                        assert math.isnan(arrays[k][t, e - 1]), (k, t, e)
                    continue
                for k in INT_KEYS:
                    assert int(arrays[k][t, e - 1]) == r[k], (k, t, e, int(arrays[k][t, e - 1]), r[k])
                for k in FLOAT_KEYS:
                    close(float(arrays[k][t, e - 1]), r[k], k, (t, e))
    else:
        assert "cells" not in ds.data_vars
    tvals = np.arange(T) if tvals is None else np.asarray(tvals)
    for e in range(1, N + 1):
        ev = events[e]
        for k in EVENT_INT_KEYS:
            got = np.asarray(ds[k].values)[e - 1]
            if k == "event_time_of_max_cells":
                if ev[k] is None:
                    assert got != got, (k, e)  # NaN / NaT
                else:
                    assert got == tvals[ev[k]], (k, e, got, tvals[ev[k]])
                continue
            assert int(got) == ev[k], (k, e, got, ev[k])
        for k in EVENT_FLOAT_KEYS:
            close(float(np.asarray(ds[k].values)[e - 1]), ev[k], k, e)
