"""mesh_event_shapes on the host: the brute-force oracle and the public path (validation, tables, windows, slot plan, host
finish, on a NumPy stand-in for the engine) against hand-computed sides, the date line, a pole, events without area, the
128-bit numerators against Python integers, the bound of the tables, an independent float64 measure of the axes, every
refusal and the dispatch of ``tracker.event_shapes`` on a mesh tracker.  No GPU needed."""
import math
import os
import sys

import numpy as np
import pytest

import marex_amd
import marex_amd._stream as ms
import marex_amd.shapes_mesh as sm
from marex_amd.exceptions import ConfigurationError, DataValidationError, TrackingError
from marex_amd.xr_compat import DataArray

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import mesh_event_shapes_cases as mc  # noqa: E402
import mesh_event_shapes_oracle as so  # noqa: E402
from mesh_event_shapes_host_engine import HostEngine  # noqa: E402
from test_mesh_tracker_host import _small, mesh_tracker  # noqa: E402


@pytest.fixture
def host_engine(monkeypatch):
    import marex_amd.detect as det

    eng = HostEngine()
    monkeypatch.setattr(det, "get_engine", lambda device=0: eng)
    monkeypatch.setattr(ms, "_free_bytes", lambda e: 1 << 30)
    return eng


def check(ids, nbr0, lat, lon, blocks=(), **kw):
    T = ids.shape[0]
    steps, events = so.mesh_event_shapes(ids, nbr0, lat, lon, **kw)
    base = marex_amd.mesh_event_shapes(ids, nbr0 + 1, lat, lon, **kw)
    so.compare(base, steps, events, T)
    for b in blocks:
        other = marex_amd.mesh_event_shapes(ids, nbr0 + 1, lat, lon, block_steps=b, **kw)
        for k in base.data_vars:
            assert np.asarray(other[k].values).tobytes() == np.asarray(base[k].values).tobytes(), k
    return base, steps, events


def _ring12():
    m = _small()
    return m["nb"].astype(np.int32) - 1, m["lat"], m["lon"]


def test_ring_of_twelve_by_hand(host_engine):
    nbr0, lat, lon = _ring12()
    assert np.array_equal(nbr0, mc.ring(12))
    ids = np.zeros((2, 12), np.int32)
    ids[:, 3:6] = 1
    ds, steps, _ = check(ids, nbr0, lat, lon)
    r = steps[(0, 1)]
    # three empty third slots, the side of cell 3 toward 2 and the side of cell 5 toward 6
    assert (r["edges"], r["border_edges"], r["contact_edges"], r["coast_edges"], r["perimeter"]) == (5, 3, 0, 0, 5.0)
    assert int(ds["edges"].values[0, 0]) == 5 and int(ds["border_edges"].values[0, 0]) == 3
    assert float(ds["area"].values[0, 0]) == 3.0 and float(ds["compactness"].values[0, 0]) == 4 * math.pi * 3 / 25
    assert ds.attrs == {"distance_units": "km", "perimeter_units": "sides"}
    ids[:, 6] = 2
    ds, steps, _ = check(ids, nbr0, lat, lon)
    assert steps[(0, 1)]["contact_edges"] == 1 and steps[(0, 2)]["contact_edges"] == 1
    assert list(ds["contact_edges"].values[0]) == [1, 1] and list(ds["edges"].values[0]) == [5, 3]


def test_single_cell_has_no_axes_and_a_path_of_zero(host_engine):
    nbr0, lat, lon = _ring12()
    ids = np.zeros((3, 12), np.int32)
    ids[:, 7] = 1
    ds, steps, events = check(ids, nbr0, lat, lon, cell_areas=np.linspace(1.0, 2.0, 12))
    for k in ("axis_major_length", "axis_minor_length", "eccentricity", "orientation"):
        assert (np.asarray(ds[k].values) == 0.0).all() and steps[(0, 1)][k] == 0.0
    assert float(ds["centroid_lat"].values[0, 0]) == pytest.approx(lat[7], abs=1e-9)
    assert float(ds["event_path_length"].values[0]) == 0.0 and float(ds["event_speed_mean"].values[0]) == 0.0
    assert int(ds["event_duration"].values[0]) == 3


def test_two_touching_events_and_land_under_an_event_cell(host_engine):
    nbr0 = mc.triangular(4, 6)
    lat, lon = mc.geometry(24, 1, grid=(4, 6))
    ids = np.zeros((2, 24), np.int32)
    ids[:, [7, 8]] = 1
    ids[:, [9, 10]] = 2
    mask = np.ones(24, bool)
    mask[8] = False   # land under a cell of event 1: nothing for event 1, coast for the side of event 2 that faces it
    mask[6] = False   # land beside event 1
    ds, steps, _ = check(ids, nbr0, lat, lon, mask=mask, blocks=(1,))
    a, b = steps[(0, 1)], steps[(0, 2)]
    # cell 7 (odd column): left 6, right 8, down 13; cell 8: left 7, right 9, up 2
    assert (a["edges"], a["border_edges"], a["contact_edges"], a["coast_edges"]) == (4, 0, 1, 1)
    # cell 9: left 8, right 10, down 15; cell 10: left 9, right 11, up 4
    assert (b["edges"], b["border_edges"], b["contact_edges"], b["coast_edges"]) == (4, 0, 1, 1)
    assert float(ds["coast_share"].values[0, 0]) == 0.25 and int(ds["event_coast_steps"].values[1]) == 2


def test_a_neighbour_listed_twice_counts_twice_and_lengths_follow_the_slots(host_engine):
    nbr0 = np.array([[1, 0, 1], [1, 0, 1], [-1, -1, 7]], np.int32)  # cell 2's third slot points outside: no neighbour
    lat, lon = np.array([0.0, 1.0, 2.0]), np.array([10.0, 11.0, 12.0])
    ids = np.array([[1, 0, 1]], np.int32)
    with pytest.raises(DataValidationError, match="Invalid neighbour array"):
        marex_amd.mesh_event_shapes(ids, nbr0 + 1, lat, lon)
    nbr0[2, 2] = -1
    el = np.array([[1.0, 2.0, 4.0], [8.0, 16.0, 32.0], [64.0, 128.0, 256.0]])
    ds, steps, _ = check(ids, nbr0, lat, lon, edge_lengths=el)
    assert steps[(0, 1)]["edges"] == 6 and steps[(0, 1)]["border_edges"] == 2
    assert float(ds["perimeter"].values[0, 0]) == 1 + 8 + 64 + 4 + 32 + 256 and ds.attrs["perimeter_units"] == "km"


def test_an_event_across_the_date_line_takes_the_wrapped_arc(host_engine):
    nbr0 = mc.ring(8)
    lat = np.zeros(8)
    lon = np.array([170.0, 175.0, 179.5, -179.0, -172.0, 0.0, 90.0, 185.0])  # 185 folds to -175
    ids = np.zeros((1, 8), np.int32)
    ids[0, [0, 1, 2, 3, 4, 7]] = 1
    ds, steps, _ = check(ids, nbr0, lat, lon)
    assert float(ds["bbox_lon_west"].values[0, 0]) == 170.0 and float(ds["bbox_lon_width"].values[0, 0]) == 18.0
    assert abs(float(ds["centroid_lon"].values[0, 0])) > 170.0
    ids[0, 5] = 1  # with the cell at 0 degrees: the arc across the date line, 0 .. 188, against the direct 359
    ds, _, _ = check(ids, nbr0, lat, lon)
    assert float(ds["bbox_lon_west"].values[0, 0]) == 0.0 and float(ds["bbox_lon_width"].values[0, 0]) == 188.0
    ids[:] = 0
    ids[0, [4, 6]] = 1  # -172 and 90: the direct arc 262 against 360 - 262 = 98 across the date line
    ds, _, _ = check(ids, nbr0, lat, lon)
    assert float(ds["bbox_lon_west"].values[0, 0]) == 90.0 and float(ds["bbox_lon_width"].values[0, 0]) == 98.0
    lon2 = np.array([-90.0, 90.0, 0, 0, 0, 0, 0, 0])
    ids[:] = 0
    ids[0, [0, 1]] = 1  # a tie of 180 degrees goes to the direct arc
    ds, _, _ = check(ids, nbr0, lat, lon2)
    assert float(ds["bbox_lon_west"].values[0, 0]) == -90.0 and float(ds["bbox_lon_width"].values[0, 0]) == 180.0


def test_an_event_over_a_pole_has_defined_values(host_engine):
    C = 13
    nbr0 = mc.ring(C)
    lat = np.array([90.0] + [85.0] * 12)
    lon = np.array([0.0] + list(np.arange(12) * 30.0 - 180.0))
    ids = np.ones((2, C), np.int32)
    ids[1, 3] = 0
    ds, steps, _ = check(ids, nbr0, lat, lon, cell_areas=np.full(C, 2.5))
    for k in ds.data_vars:
        v = np.asarray(ds[k].values)
        if v.dtype.kind == "f" and k != "coast_share":
            assert np.isfinite(v).all(), k
    assert float(ds["centroid_lat"].values[0, 0]) == pytest.approx(90.0, abs=1e-6)
    assert float(ds["eccentricity"].values[0, 0]) < 1e-6 < float(ds["eccentricity"].values[1, 0])
    # twelve of thirteen equal weights on a circle of chord radius sin(5 degrees) around the pole: each variance 0.5 * 12 / 13
    by_hand = 4 * math.sqrt(0.5 * 12 / 13) * math.sin(math.radians(5)) * 6371.0
    assert float(ds["axis_major_length"].values[0, 0]) == pytest.approx(by_hand, rel=1e-9)


def test_cells_without_area_give_nan_axes(host_engine):
    nbr0, lat, lon = _ring12()
    areas = np.ones(12)
    areas[2:5] = 0.0
    ids = np.zeros((2, 12), np.int32)
    ids[0, 2:5] = 1   # S0 == 0
    ids[1, 2:7] = 1
    ds, steps, events = check(ids, nbr0, lat, lon, cell_areas=areas)
    for k in ("axis_major_length", "axis_minor_length", "eccentricity", "orientation"):
        assert np.isnan(ds[k].values[0, 0]) and not np.isnan(ds[k].values[1, 0]), k
    assert float(ds["area"].values[0, 0]) == 0.0 and int(ds["cells"].values[0, 0]) == 3
    assert (float(ds["centroid_lat"].values[0, 0]), float(ds["centroid_lon"].values[0, 0])) == (0.0, 0.0)
    assert float(ds["compactness"].values[0, 0]) == 0.0 and np.isnan(ds["event_eccentricity_mean"].values[0])


def test_numerators_of_128_bits_equal_python_integers():
    rng = np.random.default_rng(5)
    top = 2**62 - 1
    corners = [top, -top, 2**61, -2**61, 2**61 + 1, 2**32, 2**32 - 1, -2**32, 1, 0, -1, 2**53 + 1, 3 * 2**59 + 7]
    rows = [(a, b, c, d) for a in corners for b in corners[:6] for c in corners[:5] for d in corners[:5]]
    rows += [tuple(int(v) for v in rng.integers(-top, top, 4)) for _ in range(3000)]
    rows += [(a, a, a, a) for a in corners] + [(a, a + 1, a + 1, a) for a in (2**61, 2**60 + 12345, 2**40)]  # cancellation
    rows += [(2**61 + k, 2**61 - k, 2**61, 2**61 + 1) for k in range(40)]
    s0, sij, si, sj = (np.array(v, np.int64) for v in zip(*rows))
    got = sm.exact_numerator(s0, sij, si, sj)
    exp = np.array([float(a * b - c * d) for a, b, c, d in rows])
    assert got.dtype == np.float64 and np.array_equal(got, exp)
    assert max(abs(a * b - c * d) for a, b, c, d in rows) > 2**124
    # the one rounding at a tie: 2^60 * 16 (2^53 + 1) = 2^117 + 2^64 lies midway between two float64; one unit decides
    a, b = 2**60, 16 * (2**53 + 1)
    got = sm.exact_numerator(np.array([a, a, a, -a]), np.array([b, b, b, b]), np.array([0, 1, 1, 1]), np.array([0, -1, 1, -1]))
    assert list(got) == [2.0**117, 2.0**117 + 2.0**65, 2.0**117, -(2.0**117)]
    assert list(got) == [float(a * b), float(a * b + 1), float(a * b - 1), float(-a * b + 1)]


def test_every_row_of_the_tables_sums_below_two_to_the_62():
    rng = np.random.default_rng(6)
    for C in (1, 7, 5000):
        areas = 10.0 ** rng.uniform(-3, 3, C)  # six orders of magnitude
        lat, lon = mc.geometry(C, C)
        e, q = sm.mesh_shape_tables(areas, lat, lon)
        assert q.shape == (10, C) and q.dtype == np.int64
        for row in q:
            assert sum(abs(int(v)) for v in row) < 2**62
        assert sum(int(v) for v in q[0]) > 2**60  # and the scale is not wasted
        e2, q2 = so.weight_rows(areas, lat, lon)
        assert e2 == e and all(list(q[k]) == q2[k] for k in range(10))
        el = 10.0 ** rng.uniform(-3, 3, (3, C))
        e_len, lq = sm.mesh_edge_weight_table(el, C)
        assert 2**60 < int(lq.astype(object).sum()) < 2**62 and (e_len, [list(r) for r in lq]) == so.length_rows(el)
    lat_k, lon_k = sm.coordinate_keys(np.array([90.0, -90.0, 0.0]), np.array([180.0, -180.0, 359.9999999]))
    assert list(lat_k) == [90 << 22, -(90 << 22), 0] and list(lon_k[:2]) == [-(180 << 22), -(180 << 22)] and lon_k[2] == 0


@pytest.mark.parametrize("case", ["ring", "triangular", "permuted", "ragged"])
def test_public_path_equals_the_oracle(host_engine, case):
    if case == "ring":
        nbr0, T = mc.ring(37), 9
        lat, lon = mc.geometry(37, 2)
    else:
        nbr0, T = mc.triangular(9, 11), 7
        lat, lon = mc.geometry(99, 3, grid=(9, 11))
        if case == "permuted":
            nbr0, new = mc.permuted(nbr0, 4)
            lat, lon = lat[np.argsort(new)], lon[np.argsort(new)]
        if case == "ragged":
            nbr0 = mc.ragged(nbr0, 5)
    C = nbr0.shape[1]
    ids = mc.make_field(T, nbr0, 7, n_ev=5, big=14)
    base, steps, events = check(ids, nbr0, lat, lon, blocks=(1, 3))
    assert events[2]["event_duration"] == 0 and events[1]["event_duration"] > 0
    assert ("mesh_event_shapes", 3, 3) in host_engine.calls
    check(ids, nbr0, lat, lon, blocks=(2,), **mc.tables(C, 8))
    lean = marex_amd.mesh_event_shapes(ids, nbr0 + 1, lat, lon, per_timestep=False)
    assert "cells" not in lean.data_vars and "event_area_max" in lean.data_vars
    for k in lean.data_vars:
        assert np.asarray(lean[k].values).tobytes() == np.asarray(base[k].values).tobytes(), k


def test_a_labelled_field_keeps_its_time_axis(host_engine):
    nbr0, lat, lon = _ring12()
    ids = np.zeros((3, 12), np.int32)
    ids[1:, 4:6] = 1
    tv = np.arange(3).astype("datetime64[D]").astype("datetime64[ns]")
    ds = marex_amd.mesh_event_shapes(DataArray(ids, dims=("day", "ncells"), coords={"day": ("day", tv)}), nbr0 + 1, lat, lon)
    assert tuple(ds["cells"].dims) == ("day", "ID") and np.asarray(ds["event_time_of_max_area"].values)[0] == tv[1]
    steps, events = so.mesh_event_shapes(ids, nbr0, lat, lon)
    so.compare(ds, steps, events, 3, tvals=tv)
    empty = marex_amd.mesh_event_shapes(np.zeros((3, 12), np.int32), nbr0 + 1, lat, lon)
    assert empty["cells"].values.shape == (3, 0) and empty["event_duration"].values.shape == (0,)


def test_axes_agree_with_a_centred_float64_sum():
    """Independent of the contract's integers: ``sum w (r - m)(r - m)^T / sum w`` from the areas and unit vectors alone,
    its 2 x 2 projection diagonalised by numpy.  The difference is the fixed-point rounding of rows 4 .. 9 (each below
    2^-61 sum(a) per cell, C <= 2^14) and float64 rounding; a missed cell or a wrong row shows at 1 / n or more."""
    rng = np.random.default_rng(11)
    worst = 0.0
    for trial in range(12):
        ny, nx = int(rng.integers(6, 30)), int(rng.integers(6, 30))
        C = ny * nx
        nbr0 = mc.triangular(ny, nx)
        lat, lon = mc.geometry(C, 100 + trial, grid=(ny, nx))
        areas = 10.0 ** rng.uniform(-3, 3, C)
        ids = mc.make_field(4, nbr0, 200 + trial, n_ev=4, big=40)
        steps, _ = so.mesh_event_shapes(ids, nbr0, lat, lon, cell_areas=areas, radius_km=1.0)
        phi, lam = np.radians(lat), np.radians(lon)
        r = np.stack([np.cos(phi) * np.cos(lam), np.cos(phi) * np.sin(lam), np.sin(phi)], 1)
        for (t, e), s in steps.items():
            sel = ids[t] == e
            if sel.sum() < 2:
                continue
            w = areas[sel]
            m = (w[:, None] * r[sel]).sum(0) / w.sum()
            d = r[sel] - m
            cov = (w[:, None, None] * d[:, :, None] * d[:, None, :]).sum(0) / w.sum()
            pc, lc = math.asin(m[2] / np.linalg.norm(m)), math.atan2(m[1], m[0])
            frame = np.array([[-math.sin(lc), math.cos(lc), 0.0],
                              [-math.sin(pc) * math.cos(lc), -math.sin(pc) * math.sin(lc), math.cos(pc)]])
            l2, l1 = np.linalg.eigvalsh(frame @ cov @ frame.T)
            got1, got2 = (s["axis_major_length"] / 4.0) ** 2, (s["axis_minor_length"] / 4.0) ** 2
            worst = max(worst, abs(got1 - l1) / l1, abs(got2 - max(l2, 0.0)) / l1)
    assert 0.0 < worst < 1e-9, worst


def test_refusals(monkeypatch):
    import marex_amd.detect as det

    def no_gpu(*a, **k):
        raise AssertionError("a refusal reached the engine")

    monkeypatch.setattr(det, "get_engine", no_gpu)
    C = 12
    nbr0, lat, lon = _ring12()
    ids = np.zeros((3, C), np.int32)
    neg = ids.copy()
    neg[1, 3] = -1
    V = DataValidationError
    base = dict(ID_field=ids, neighbours=nbr0 + 1, lat=lat, lon=lon)
    cases = [
        (dict(ID_field=np.zeros((3, 4, 5), np.int32)), V, "event_shapes measures grids"),
        (dict(ID_field=np.zeros(5, np.int32)), V, r"ID_field must be \(time, cells\)"),
        (dict(ID_field=ids.astype(np.float32)), V, "Object IDs must be integers"),
        (dict(ID_field=neg), V, "Object IDs must be non-negative"),
        (dict(neighbours=(nbr0 + 1)[:2]), V, "Invalid neighbour array"),
        (dict(neighbours=(nbr0 + 1)[:, :5]), V, "Invalid neighbour array"),
        (dict(neighbours=np.where(nbr0 == 3, C + 1, nbr0 + 1)), V, f"cell numbers up to {C}"),
        (dict(neighbours=(nbr0 + 1) + 0.5), V, "Invalid neighbour array"),
        (dict(neighbours=np.full((3, C), np.nan)), V, "Invalid neighbour array"),
        (dict(lat=None), V, "needs lat and lon"),
        (dict(lon=lon[:5]), V, "one per cell"),
        (dict(lat=np.where(np.arange(C) == 2, np.nan, lat)), V, "finite degrees"),
        (dict(lat=np.where(np.arange(C) == 2, 90.5, lat)), V, r"\|lat\| <= 90"),
        (dict(cell_areas=np.ones(5)), V, "cell_areas must be numbers, one per cell"),
        (dict(cell_areas=-np.ones(C)), V, "cell_areas must be finite and non-negative"),
        (dict(cell_areas=np.zeros(C)), V, "positive, finite sum"),
        (dict(edge_lengths=np.ones(C)), V, r"edge_lengths must be numbers of shape \(3, cells\)"),
        (dict(edge_lengths=-np.ones((3, C))), V, "edge_lengths must be finite and non-negative"),
        (dict(edge_lengths=np.zeros((3, C))), V, "edge_lengths must have a positive, finite sum"),
        (dict(mask=np.ones(5, bool)), V, "mask does not match"),
        (dict(mask=np.ones(C)), V, "mask must be boolean"),
        (dict(radius_km=0.0), V, "radius_km must be positive"),
        (dict(block_steps=0), ConfigurationError, "block_steps must be a positive number"),
    ]
    for kw, cls, msg in cases:
        args = dict(base)
        args.update(kw)
        with pytest.raises(cls, match=msg):
            marex_amd.mesh_event_shapes(**args)
    huge = np.lib.stride_tricks.as_strided(np.zeros(1, np.int32), shape=(2, 2**31 - 1), strides=(0, 0))
    with pytest.raises(TrackingError, match="reaches 2\\^31 - 1"):
        sm._validate(huge, None, None, None, None, None, None, 6371.0, False)
    with pytest.raises(TypeError):
        marex_amd.mesh_event_shapes(ids, nbr0 + 1)  # lat and lon are required


def test_the_grid_function_still_refuses_a_mesh_field_and_points_here():
    with pytest.raises(ConfigurationError, match="shapes are gridded only") as err:
        marex_amd.event_shapes(np.zeros((3, 20), np.int32))
    assert "mesh_event_shapes" in str(err.value.details)
    assert "mesh_event_shapes" in marex_amd.__all__ and marex_amd.mesh_event_shapes is sm.mesh_event_shapes


def test_tracker_event_shapes_dispatches_on_a_mesh_tracker(host_engine):
    m = _small()
    trk = mesh_tracker(m["ev"], m["mask"], m["nb"], m["areas"], m["lat"], m["lon"], tm=np.arange(4) * 10)
    ids = np.zeros((4, 12), np.int32)
    ids[0:3, 2:5] = 1
    ids[2:4, 8:10] = 2
    field = DataArray(ids, dims=("time", "ncells"))
    nbr0 = m["nb"].astype(np.int32) - 1
    steps, events = so.mesh_event_shapes(ids, nbr0, trk.lat, trk.lon, cell_areas=m["areas"], mask=m["mask"])
    ds = trk.event_shapes(field)
    so.compare(ds, steps, events, 4, tvals=np.arange(4) * 10)
    assert tuple(ds["cells"].dims) == ("time", "ID") and ds.attrs["perimeter_units"] == "sides"
    from marex_amd.xr_compat import Dataset

    events_ds = Dataset({"ID_field": field, "ID": DataArray(np.arange(1, 4), dims=("ID",))})
    ds = trk.event_shapes(events_ds, edge_lengths=np.full((3, 12), 2.0), per_timestep=False, block_steps=2)
    assert list(np.asarray(ds["ID"].values)) == [1, 2, 3] and list(ds["event_duration"].values) == [3, 2, 0]
    assert ds.attrs["perimeter_units"] == "km" and float(ds["event_perimeter_max"].values[0]) == 10.0
    with pytest.raises(TypeError, match="unexpected keyword argument 'regional_mode'"):
        trk.event_shapes(field, regional_mode=True)
    events_ds = Dataset({"ID_field": field, "ID": DataArray(np.arange(1, 2), dims=("ID",))})
    with pytest.raises(marex_amd.ProcessingError, match="the events Dataset ends at 1"):
        trk.event_shapes(events_ds)
