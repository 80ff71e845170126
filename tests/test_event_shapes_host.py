"""event_shapes on the host: the brute-force oracle and the public path (validation, windows, slot plan, host finish, on a
NumPy stand-in for the engine) against hand-computed shapes, the seam objects of test_object_props_host.py restated for the
bounding box and the second moments, the Python-integer branch of the host finish, and every refusal.  No GPU needed."""
import math
import os
import sys

import numpy as np
import pytest

import marex_amd
import marex_amd._stream as ms
import marex_amd.shapes as sh
from marex_amd.engine import HotPath
from marex_amd.exceptions import ConfigurationError, DataValidationError, TrackingError
from marex_amd.xr_compat import DataArray

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import event_shapes_oracle as so  # noqa: E402
from event_shapes_host_engine import HostEngine  # noqa: E402


@pytest.fixture
def host_engine(monkeypatch):
    import marex_amd.detect as det

    eng = HostEngine()
    monkeypatch.setattr(det, "get_engine", lambda device=0: eng)
    monkeypatch.setattr(ms, "_free_bytes", lambda e: 1 << 30)
    return eng


def _one(ids2d, **kw):
    """The Dataset and the oracle row of the single event 1 of a single slice (repeated over two steps)."""
    ids = np.stack([ids2d, ids2d]).astype(np.int32)
    ds = marex_amd.event_shapes(ids, **kw)
    steps, events = so.event_shapes(ids, **kw)
    so.compare(ds, steps, events, 2)
    return {k: np.asarray(ds[k].values)[0, 0] for k in so.INT_KEYS + so.FLOAT_KEYS}, steps[(0, 1)]


def test_single_cell_in_a_periodic_grid(host_engine):
    g = np.zeros((3, 5), np.int32)
    g[1, 2] = 1
    got, exp = _one(g)
    assert (got["edges_ns"], got["edges_ew"], got["border_edges"], got["coast_edges"], got["perimeter"]) == (2, 2, 0, 0, 4.0)
    assert exp["edges_ns"] == 2 and exp["edges_ew"] == 2
    for k in ("axis_major_length", "axis_minor_length", "eccentricity", "orientation"):
        assert got[k] == 0.0 and exp[k] == 0.0
    assert (got["bbox_y0"], got["bbox_x0"], got["bbox_height"], got["bbox_width"], got["extent"]) == (1, 2, 1, 1, 1.0)
    assert got["compactness"] == 4 * math.pi / 16


# Below 200 columns every object has a cell in both 100-column bands of calculate_centroid's rule and counts as wrapped; the
# hand-computed shapes stand in the middle of a 240-column grid, in neither band.
def test_two_by_three_rectangle(host_engine):
    g = np.zeros((5, 240), np.int32)
    g[1:3, 110:113] = 1
    got, exp = _one(g)
    assert got["edges_ns"] + got["edges_ew"] == 10 and (got["edges_ns"], got["edges_ew"]) == (6, 4)
    assert got["extent"] == 1.0 and got["cells"] == 6
    assert got["axis_major_length"] == pytest.approx(4 * math.sqrt(2 / 3), rel=1e-15)  # vxx = 2/3
    assert got["axis_minor_length"] == pytest.approx(2.0, rel=1e-15)                   # vyy = 1/4
    assert got["eccentricity"] == pytest.approx(math.sqrt(0.625), rel=1e-15)
    assert got["orientation"] == 0.0
    assert exp["axis_minor_length"] == pytest.approx(2.0, rel=1e-15) and exp["orientation"] == 0.0
    g[:] = 0
    g[1:4, 110:112] = 1  # the long side along y: a quarter turn
    assert _one(g)[0]["orientation"] == pytest.approx(math.pi / 2, abs=1e-15)
    small = np.zeros((5, 7), np.int32)
    small[1:3, 2:5] = 1  # on 7 columns the rule wraps it: column 4 stands at -3, the box is 7 wide
    assert _one(small)[0]["bbox_width"] == 7 and _one(small, regional_mode=True)[0]["bbox_width"] == 3


def test_diagonal_of_single_cells(host_engine):
    g = np.zeros((6, 240), np.int32)
    for k in range(4):
        g[1 + k, 110 + k] = 1
    got, exp = _one(g)
    assert got["axis_minor_length"] == 0.0 and got["eccentricity"] == 1.0
    assert got["orientation"] == pytest.approx(math.pi / 4, abs=1e-15)
    assert got["edges_ns"] == 8 and got["edges_ew"] == 8 and got["extent"] == 0.25
    g2 = g[:, ::-1].copy()  # the other diagonal: from +x toward -y
    assert _one(g2)[0]["orientation"] == pytest.approx(-math.pi / 4, abs=1e-15)


@pytest.mark.parametrize("nx", [5, 150, 360])
def test_full_row_periodic_and_regional(host_engine, nx):
    g = np.zeros((3, nx), np.int32)
    g[1] = 1
    got, _ = _one(g)
    assert (got["edges_ew"], got["edges_ns"], got["border_edges"], got["bbox_width"], got["bbox_x0"]) == (0, 2 * nx, 0, nx, nx // 2 + 1)
    reg, _ = _one(g, regional_mode=True)
    assert (reg["edges_ew"], reg["edges_ns"], reg["border_edges"], reg["bbox_width"], reg["bbox_x0"]) == (2, 2 * nx, 2, nx, 0)
    top = np.zeros((3, nx), np.int32)
    top[0] = 1
    assert _one(top)[0]["border_edges"] == nx and _one(top, regional_mode=True)[0]["border_edges"] == nx + 2


def test_nx_one_and_two(host_engine):
    g = np.zeros((4, 1), np.int32)
    g[1:3, 0] = 1
    got, _ = _one(g)  # its own east and west neighbour: no east / west side
    assert (got["edges_ns"], got["edges_ew"], got["border_edges"], got["bbox_width"]) == (2, 0, 0, 1)
    reg, _ = _one(g, regional_mode=True)
    assert (reg["edges_ns"], reg["edges_ew"], reg["border_edges"]) == (2, 4, 4)
    g = np.zeros((3, 2), np.int32)
    g[1, 0] = 1
    got, _ = _one(g)  # both sides face the same cell: both counted
    assert (got["edges_ns"], got["edges_ew"], got["border_edges"]) == (2, 2, 0)
    reg, _ = _one(g, regional_mode=True)
    assert (reg["edges_ns"], reg["edges_ew"], reg["border_edges"]) == (2, 2, 1)
    g[1, 1] = 1
    assert _one(g)[0]["edges_ew"] == 0 and _one(g, regional_mode=True)[0]["edges_ew"] == 2


# the seam objects of HAND_CENTROIDS (tests/test_object_props_host.py): (nx, columns in one row), restated by hand as
# (centroid_x, bbox_x0, bbox_width, variance of x'): wrapped where a column < 100 and a column >= nx - 100 exist; then the
# columns > nx // 2 stand at column - nx
HAND_SEAM = [
    (360, (0, 1, 2, 359), 0.5, 359, 4, 1.25),         # x' = 0, 1, 2, -1
    (360, (0, 1, 358, 359), 359.5, 358, 4, 1.25),     # x' = 0, 1, -2, -1
    (360, (100, 200), 150.0, 100, 101, 2500.0),       # in neither band: plain
    (1, (0,), 0.0, 0, 1, 0.0),
    (50, (0, 49), 49.5, 49, 2, 0.25),                 # x' = 0, -1
    (50, (10, 20), 15.0, 10, 11, 25.0),               # both bands, nothing right of 25
    (50, (20, 30), 0.0, 30, 41, 400.0),               # x' = 20, -20
    (100, (0, 99), 99.5, 99, 2, 0.25),
    (150, (10, 140), 0.0, 140, 21, 100.0),            # x' = 10, -10
    (150, (76,), 76.0, 76, 1, 0.0),
    (199, (0, 198), 198.5, 198, 2, 0.25),
    (199, (98, 100), 198.5, 100, 198, 9702.25),       # x' = 98, -99: 197 apart
    (200, (10, 150), 180.0, 150, 61, 900.0),          # x' = 10, -50
    (200, (99, 100), 99.5, 99, 2, 0.25),              # 100 > 100 is false: plain
    (201, (99, 101), 200.5, 101, 200, 9900.25),       # x' = 99, -100: 199 apart
    (201, (99, 100), 99.5, 99, 2, 0.25),
]


@pytest.mark.parametrize("nx,cols,cx,x0,width,var", HAND_SEAM)
def test_seam_objects_bbox_and_second_moments(host_engine, nx, cols, cx, x0, width, var):
    g = np.zeros((3, nx), np.int32)
    g[1, list(cols)] = 1
    got, exp = _one(g)
    assert (got["centroid_y"], got["centroid_x"], got["bbox_x0"], got["bbox_width"]) == (1.0, cx, x0, width)
    assert (exp["centroid_x"], exp["bbox_x0"], exp["bbox_width"]) == (cx, x0, width)
    assert got["axis_major_length"] == pytest.approx(4 * math.sqrt(var), rel=1e-15) and got["axis_minor_length"] == 0.0
    reg, _ = _one(g, regional_mode=True)  # the plain mean, the plain box
    assert reg["centroid_x"] == float(np.mean(cols)) and reg["bbox_x0"] == min(cols) and reg["bbox_width"] == max(cols) - min(cols) + 1


def _field(T, ny, nx, seed, n_ev=5):
    rng = np.random.default_rng(seed)
    ids = np.zeros((T, ny, nx), np.int32)
    for e in range(1, n_ev + 1):
        t0, t1 = sorted(rng.integers(0, T, 2))
        y, x = rng.integers(0, ny), rng.integers(0, nx)
        for t in range(t0, t1 + 1):
            if rng.random() < 0.15 and t0 < t < t1:
                continue  # absent inside its span
            h, w = rng.integers(1, max(2, ny // 2)), rng.integers(1, max(2, nx // 2))
            yy = (y + np.arange(h)) % ny
            xx = (x + np.arange(w)) % nx
            blob = rng.random((h, w)) < 0.8
            sub = ids[t][np.ix_(yy, xx)]
            ids[t][np.ix_(yy, xx)] = np.where(blob, e, sub)
            x = (x + rng.integers(-2, 3)) % nx
    return ids


@pytest.mark.parametrize("regional", [False, True])
@pytest.mark.parametrize("shape", [(7, 6, 9), (5, 1, 30), (5, 12, 1), (4, 3, 2), (6, 5, 150), (3, 4, 201)])
def test_public_path_equals_the_oracle(host_engine, shape, regional):
    T, ny, nx = shape
    ids = _field(T, ny, nx, 100 + nx)
    rng = np.random.default_rng(7)
    mask = rng.random((ny, nx)) > 0.3
    lat, lon = np.linspace(-60, 60, ny) if ny > 1 else np.array([10.0]), np.arange(nx) * (360.0 / nx)
    areas = 10.0 ** rng.uniform(-3, 3, (ny, nx))
    edges = (10.0 ** rng.uniform(-3, 3, ny + 1), 10.0 ** rng.uniform(-3, 3, ny))
    for kw in (dict(), dict(mask=mask), dict(mask=mask, cell_areas=areas, edge_lengths=edges, lat=lat, lon=lon)):
        steps, events = so.event_shapes(ids, regional_mode=regional, **kw)
        base = marex_amd.event_shapes(ids, regional_mode=regional, **kw)
        so.compare(base, steps, events, T)
        for b in (1, 3):
            ds = marex_amd.event_shapes(ids, regional_mode=regional, block_steps=b, **kw)
            for k in base.data_vars:
                assert np.array_equal(np.asarray(ds[k].values), np.asarray(base[k].values), equal_nan=True), (k, b)
        lean = marex_amd.event_shapes(ids, regional_mode=regional, per_timestep=False, **kw)
        so.compare(lean, steps, events, T, per_timestep=False)
    assert ("event_shapes", 0, T) in host_engine.calls and (T <= 3 or ("event_shapes", 3, min(3, T - 3)) in host_engine.calls)


def test_time_names_dates_and_an_empty_field(host_engine):
    ids = _field(6, 5, 8, 3)
    tv = np.arange(6).astype("datetime64[D]").astype("datetime64[ns]")
    da = DataArray(ids, dims=("day", "lat", "lon"), coords={"day": ("day", tv)})
    ds = marex_amd.event_shapes(da)
    steps, events = so.event_shapes(ids)
    so.compare(ds, steps, events, 6, tvals=tv)
    assert ds["cells"].dims == ("day", "ID") and ds.attrs["distance_units"] == "cells" and ds.attrs["perimeter_units"] == "sides"
    empty = marex_amd.event_shapes(np.zeros((3, 4, 5), np.int32))
    assert np.asarray(empty["cells"].values).shape == (3, 0) and np.asarray(empty["event_duration"].values).shape == (0,)


def test_grid_edge_lengths():
    lat, lon = np.array([-89.5, 0.0, 45.0, 89.5]), np.arange(8) * 45.0
    ns, ew = marex_amd.grid_edge_lengths(lat, lon)
    ns_o, ew_o = so.grid_edge_lengths(list(lat), list(lon))
    assert ns.shape == (5,) and ew.shape == (4,)
    assert np.allclose(ns, ns_o, rtol=1e-14, atol=1e-9) and np.allclose(ew, ew_o, rtol=1e-14)
    k = math.pi / 180
    assert ns[2] == pytest.approx(6371.0 * math.cos(22.5 * k) * 45 * k, rel=1e-14)  # the interface midway between 0 and 45
    assert ns[0] == pytest.approx(0.0, abs=1e-9) and ns[4] == pytest.approx(0.0, abs=1e-9)  # clipped to the poles
    assert ew[1] == pytest.approx(6371.0 * (22.5 + 44.75) * k, rel=1e-14)
    e, ns_q, ew_q = sh.edge_weight_tables((ns, ew), 4, 8)
    eo, ns_qo, ew_qo = so.quantise_edges(ns, ew, 8)
    assert (e, ns_q.tolist(), ew_q.tolist()) == (eo, ns_qo, ew_qo)
    assert 8 * int(ns_q.sum()) + 9 * int(ew_q.sum()) < 2**62


def test_host_finish_takes_python_integers_where_int64_would_wrap():
    """Synthetic sums with n sum(x^2) >= 2^63: a 3 x 30000 block of cells at columns 30000 .. 59999 of a 65536-wide grid,
    the sums in closed form; the axes follow from the exact variances (w^2 - 1) / 12 and (h^2 - 1) / 12."""
    h, w, xa, ya, nx = 3, 30000, 30000, 5, 65536
    n = h * w
    s1 = lambda a, m: m * a + m * (m - 1) // 2                                    # noqa: E731 -- sum of a .. a + m - 1
    s2 = lambda a, m: m * a * a + a * m * (m - 1) + (m - 1) * m * (2 * m - 1) // 6  # noqa: E731 -- sum of squares
    mom = np.zeros((1, 16), np.int64)
    mom[0, :10] = [n, w * s1(ya, h), h * s1(xa, w), h * (w - (nx // 2 + 1 - xa)), 0, w * s2(ya, h), h * s2(xa, w),
                   s1(xa, w) * s1(ya, h), 0, 0]
    assert n * int(mom[0, 6]) >= 2**63
    mom[0, 10:12] = [2 * w, 2 * h]
    box = np.array([[ya, ya + h - 1, xa, nx // 2, nx // 2 + 1, xa + w - 1]], np.int32)
    p = {"T": 1, "ny": 100, "nx": nx, "area": None, "edges": None, "lat": None, "lon": None}
    tmin, off = np.array([0, 0], np.int64), np.array([0, 0, 1], np.int64)
    ds = sh._finish(p, 1, tmin, off, mom, box, True, True, "time", np.arange(1))
    one = lambda k: float(np.asarray(ds[k].values)[0, 0])  # noqa: E731
    assert one("axis_major_length") == pytest.approx(4 * math.sqrt((w * w - 1) / 12), rel=1e-14)
    assert one("axis_minor_length") == pytest.approx(4 * math.sqrt((h * h - 1) / 12), rel=1e-12)
    assert one("eccentricity") == pytest.approx(math.sqrt(1 - (h * h - 1) / (w * w - 1)), rel=1e-14)
    assert one("orientation") == 0.0 and one("bbox_width") == w and one("extent") == 1.0
    assert one("centroid_x") == xa + (w - 1) / 2 and one("centroid_y") == ya + 1.0
    tr, root, det, _, _ = sh._exact_axes(*(mom[:, k] for k in (0, 1, 2, 5, 6, 7)))
    nxx, nyy = n * int(mom[0, 6]) - int(mom[0, 2]) ** 2, n * int(mom[0, 5]) - int(mom[0, 1]) ** 2
    assert nxx * nyy >= 2**63  # no int64 holds the determinant
    assert tr[0] == float(nxx + nyy) and det[0] == float(nxx * nyy) and root[0] == pytest.approx(float(nxx - nyy), rel=1e-15)


def test_refusals_come_before_the_device(monkeypatch):
    import marex_amd.detect as det

    def no_gpu(*a, **k):
        raise AssertionError("the validation touched the GPU engine")

    monkeypatch.setattr(det, "get_engine", no_gpu)
    ids = np.zeros((3, 4, 5), np.int32)
    neg = ids.copy()
    neg[1, 2, 3] = -1
    cases = [
        (dict(ID_field=np.zeros((3, 20), np.int32)), ConfigurationError, "shapes are gridded only"),
        (dict(ID_field=ids[0, 0]), DataValidationError, r"ID_field must be \(time, y, x\)"),
        (dict(ID_field=ids.astype(np.float32)), DataValidationError, "Object IDs must be integers"),
        (dict(ID_field=ids > 0), DataValidationError, "Object IDs must be integers"),
        (dict(ID_field=neg), DataValidationError, "Object IDs must be non-negative"),
        (dict(ID_field=np.broadcast_to(np.zeros((), np.int32), (2, 46341, 46341))), TrackingError, "reaches 2\\^31 - 1"),
        (dict(ID_field=np.broadcast_to(np.zeros((), np.int32), (2**31 - 1, 1, 1))), TrackingError, "reaches 2\\^31 - 1"),
        (dict(ID_field=np.broadcast_to(np.zeros((), np.int32), (2, 1, 65537))), TrackingError, "a side above 65536"),
        (dict(mask=np.ones((5, 4), bool)), DataValidationError, "mask does not match"),
        (dict(mask=np.ones((4, 5), np.float32)), DataValidationError, "mask must be boolean"),
        (dict(cell_areas=-np.ones((4, 5))), DataValidationError, "cell_areas must be finite and non-negative"),
        (dict(cell_areas=np.full(20, np.nan)), DataValidationError, "cell_areas must be finite and non-negative"),
        (dict(cell_areas=np.ones(5)), DataValidationError, "cell_areas do not match the spatial shape of ID_field"),
        (dict(cell_areas=np.zeros((4, 5))), DataValidationError, "positive, finite sum"),
        (dict(edge_lengths=np.ones(5)), DataValidationError, "edge_lengths must be a pair"),
        (dict(edge_lengths=(np.ones(4), np.ones(4))), DataValidationError, "edge_lengths do not match the grid"),
        (dict(edge_lengths=(np.ones(5), np.ones(5))), DataValidationError, "edge_lengths do not match the grid"),
        (dict(edge_lengths=(-np.ones(5), np.ones(4))), DataValidationError, "edge_lengths must be finite and non-negative"),
        (dict(edge_lengths=(np.ones(5), np.full(4, np.inf))), DataValidationError, "edge_lengths must be finite and non-negative"),
        (dict(lat=np.arange(4.0)), DataValidationError, "lat and lon come together"),
        (dict(lat=np.arange(5.0), lon=np.arange(4.0)), DataValidationError, "lat and lon must be finite 1-D coordinates"),
    ]
    cases += [(dict(block_steps=b), ConfigurationError, "block_steps must be a positive number of timesteps, 'auto' or None")
              for b in (0, -2, 2.5, True, "all")]
    for kw, cls, msg in cases:
        args = dict(ID_field=ids)
        args.update(kw)
        with pytest.raises(cls, match=msg):
            marex_amd.event_shapes(**args)


def test_event_shapes_is_public():
    assert "event_shapes" in marex_amd.__all__ and marex_amd.event_shapes is sh.event_shapes
    assert "grid_edge_lengths" in marex_amd.__all__ and marex_amd.grid_edge_lengths is sh.grid_edge_lengths
    assert hasattr(marex_amd.tracker, "event_shapes") and hasattr(HotPath, "event_shapes")
    assert "Unsupported" not in (marex_amd.event_shapes.__doc__ or "") and "scikit-image" in marex_amd.event_shapes.__doc__
