"""event_shapes on the device against the brute-force oracle of tests/event_shapes_oracle.py: every integer output with ==,
the derived floats within 1e-12 (relative; absolute for the orientation) -- each float is at most about a dozen correctly
rounded float64 operations on exact integers in the stable form, about 1.3e-15; the margin covers libm differences in sqrt,
atan2 and the haversine.  The shapes are the smallest at which the kernel can go wrong: (70, 67) is two workgroups with
rows straddling the 64-cell pieces and the 1024-cell wave chunks, T = 67 makes a workgroup visit two slices (stride 64)."""
import os
import sys

import numpy as np
import pytest
import torch

import marex_amd
from marex_amd.exceptions import ConfigurationError
from marex_amd.xr_compat import DataArray

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import event_shapes_oracle as so  # noqa: E402
from intensity_cases import blobs  # noqa: E402

pytestmark = pytest.mark.gpu


def make_field(T, ny, nx, seed, n_ev=8, big=12, seam=False):
    """Sparse event numbers (1, 4, 7, ...), drifting ragged blocks that overwrite and so touch each other, steps on which an
    event is absent inside its span, with ``seam`` every block starting within 3 columns of the last one, and the largest
    number in the last cell of the last slice."""
    rng = np.random.default_rng(seed)
    ids = np.zeros((T, ny, nx), np.int32)
    for k in range(n_ev):
        e = 1 + 3 * k
        t0, t1 = sorted(int(v) for v in rng.integers(0, T, 2))
        y = int(rng.integers(0, ny))
        x = int(nx - 1 - rng.integers(0, min(3, nx))) if seam else int(rng.integers(0, nx))
        for t in range(t0, t1 + 1):
            if t0 < t < t1 and rng.random() < 0.2:
                continue
            h, w = int(rng.integers(1, min(big, ny) + 1)), int(rng.integers(1, min(big, nx) + 1))
            yy, xx = np.arange(y, min(ny, y + h)), (x + np.arange(w)) % nx
            keep = rng.random((yy.size, w)) < 0.85
            ids[t][np.ix_(yy, xx)] = np.where(keep, e, ids[t][np.ix_(yy, xx)])
            x = (x + int(rng.integers(-2, 3))) % nx
            y = int(np.clip(y + rng.integers(-1, 2), 0, ny - 1))
    ids[T - 1, ny - 1, nx - 1] = 3 * n_ev + 2
    return ids


def tables(ny, nx, seed):
    rng = np.random.default_rng(seed)
    mask = rng.random((ny, nx)) > 0.25                       # land next to, and under, event cells
    areas = 10.0 ** rng.uniform(-3, 3, (ny, nx))             # six orders of magnitude
    edges = (10.0 ** rng.uniform(-3, 3, ny + 1), 10.0 ** rng.uniform(-3, 3, ny))
    lat = np.linspace(-70, 70, ny) if ny > 1 else np.array([12.5])
    return dict(mask=mask, cell_areas=areas, edge_lengths=edges, lat=lat, lon=(np.arange(nx) + 0.5) * (360.0 / nx))


def same_bits(a, b):
    assert list(a.data_vars) == list(b.data_vars)
    for k in a.data_vars:
        u, v = np.asarray(a[k].values), np.asarray(b[k].values)
        assert u.dtype == v.dtype and u.tobytes() == v.tobytes(), k


def check(ids, blocks=(), resident=False, **kw):
    T = ids.shape[0]
    steps, events = so.event_shapes(ids, **kw)
    base = marex_amd.event_shapes(ids, **kw)
    so.compare(base, steps, events, T)
    for b in blocks:
        same_bits(marex_amd.event_shapes(ids, block_steps=b, **kw), base)
    if resident:
        dev = torch.from_numpy(ids).to("cuda:0")
        same_bits(marex_amd.event_shapes(dev, **kw), base)
        same_bits(marex_amd.event_shapes(dev, block_steps=3, **kw), base)
    return base, steps, events


@pytest.mark.parametrize("regional", [False, True], ids=["periodic", "regional"])
def test_two_workgroups_two_slices_per_workgroup(hot, regional):
    ny, nx, T = 70, 67, 67
    ids = make_field(T, ny, nx, 1, n_ev=10)
    ids[3:6, 8:40, 5:60] = np.where(np.random.default_rng(2).random((3, 32, 55)) < 0.9, 29, ids[3:6, 8:40, 5:60])  # a large event
    ids[10, 0, :] = 30          # a full row on the upper border
    ids[11, :, 0] = 30          # a full column
    ids[12] = 30                # a whole slice
    assert ids.max() == ids[-1, -1, -1] == 32
    base, steps, events = check(ids, blocks=(1, 3), resident=True, regional_mode=regional)
    assert steps[(12, 30)]["edges_ew"] == (2 * ny if regional else 0) and steps[(12, 30)]["edges_ns"] == 2 * nx
    assert events[2]["event_duration"] == 0 and events[1]["event_duration"] > 0  # sparse numbers: an event without a cell
    assert any(events[e]["event_duration"] < max(t for (t, k) in steps if k == e) - min(t for (t, k) in steps if k == e) + 1
               for e in events if events[e]["event_duration"])  # an event absent inside its span
    check(ids, blocks=(3,), regional_mode=regional, **tables(ny, nx, 3))


@pytest.mark.parametrize("regional", [False, True], ids=["periodic", "regional"])
@pytest.mark.parametrize("shape", [(1, 130), (130, 1), (3, 2)])
def test_degenerate_grids(hot, shape, regional):
    ny, nx = shape
    ids = make_field(9, ny, nx, 5 + nx, n_ev=4, big=40)
    check(ids, blocks=(1,), regional_mode=regional)
    check(ids, resident=True, regional_mode=regional, **tables(ny, nx, 4))


@pytest.mark.parametrize("regional", [False, True], ids=["periodic", "regional"])
@pytest.mark.parametrize("nx", [150, 199, 200, 201, 360])
def test_objects_on_the_seam(hot, nx, regional):
    ids = make_field(7, 6, nx, nx, n_ev=5, big=6, seam=True)
    ids[2, 3, [0, 1, nx - 2, nx - 1]] = 16         # HAND_CENTROIDS' straddling rows
    ids[3, 3, [98, 100]] = 16
    ids[4, 3, [10, nx - 50]] = 16
    ids[5, 3, [99, nx // 2 + 1]] = 16
    base, steps, _ = check(ids, blocks=(3,), regional_mode=regional)
    assert steps[(2, 16)]["bbox_width"] == (nx if regional else 4)
    check(ids, regional_mode=regional, **tables(6, nx, 6))


def test_two_events_that_touch_and_land_under_events(hot):
    ids = np.zeros((2, 5, 240), np.int32)
    ids[:, 1:3, 110:113] = 1
    ids[:, 1:4, 113:115] = 2
    mask = np.ones((5, 240), bool)
    mask[0, :] = False
    mask[2, 112] = False  # land under a cell of event 1: nothing for event 1, coast for the side of event 2 that faces it
    ds, steps, _ = check(ids, mask=mask)
    a, b = steps[(0, 1)], steps[(0, 2)]
    assert (a["edges_ns"], a["edges_ew"], b["edges_ns"], b["edges_ew"]) == (6, 4, 4, 6)  # the shared edge counts once for each
    assert a["coast_edges"] == 3 and b["coast_edges"] == 2 + 1  # row 0 above three / two cells, and the west side of (2, 113)
    assert a["axis_minor_length"] == pytest.approx(2.0, rel=1e-15) and a["orientation"] == 0.0


@pytest.mark.parametrize("seed", range(20))
def test_fuzz(hot, seed):
    rng = np.random.default_rng(1000 + seed)
    T = int(rng.integers(1, 71))
    ny = int(rng.integers(1, 60))
    nx = int(rng.integers(1, min(400, 10000 // ny, max(2, 100000 // (T * ny))) + 1))
    ids = make_field(T, ny, nx, seed, n_ev=int(rng.integers(1, 9)), big=int(rng.integers(1, 20)), seam=bool(seed % 3 == 0))
    kw = tables(ny, nx, seed) if seed % 2 else {}
    if seed % 4 == 1:
        kw.pop("lat"), kw.pop("lon")
    check(ids, blocks=(int(rng.integers(1, 6)),), regional_mode=bool(seed % 5 < 2), **kw)


def test_refusals_and_the_lean_dataset(hot):
    with pytest.raises(ConfigurationError, match="shapes are gridded only"):
        marex_amd.event_shapes(torch.zeros((3, 40), dtype=torch.int32, device="cuda:0"))
    ids = make_field(5, 7, 9, 1, n_ev=3)
    lean = marex_amd.event_shapes(ids, per_timestep=False)
    full = marex_amd.event_shapes(ids)
    assert "cells" not in lean.data_vars
    for k in lean.data_vars:
        assert np.asarray(lean[k].values).tobytes() == np.asarray(full[k].values).tobytes(), k


def test_merge_tracker_end_to_end(hot):
    ev = blobs()
    T, ny, nx = ev.shape
    lat, lon = np.linspace(-57.5, 57.5, ny), np.linspace(3.75, 356.25, nx)
    tv = np.arange(T).astype("datetime64[D]").astype("datetime64[ns]")
    mask = np.ones((ny, nx), bool)
    mask[:4] = False  # a coast across the discs' paths
    da = DataArray(ev & mask, dims=("time", "lat", "lon"), coords={"time": ("time", tv), "lat": ("lat", lat), "lon": ("lon", lon)},
                   name="extreme_events")
    trk = marex_amd.tracker(da, DataArray(mask, dims=("lat", "lon")), R_fill=1, T_fill=2, area_filter_quartile=0.2, timechunks=4,
                            coordinate_units="degrees", allow_merging=True)
    events = trk.run()
    field = np.asarray(events["ID_field"].values)
    N = int(events["ID"].values.size)
    assert N >= 3 and field.max() <= N
    ds = trk.event_shapes(events)
    steps, evs = so.event_shapes(field, mask=mask, lat=lat, lon=lon)
    for e in range(int(field.max()) + 1, N + 1):  # trailing events without a cell
        evs[e] = dict({k: 0 for k in so.EVENT_INT_KEYS}, **{k: np.nan for k in so.EVENT_FLOAT_KEYS}, event_time_of_max_cells=None)
    so.compare(ds, steps, evs, T, tvals=tv)
    assert ds.attrs["distance_units"] == "km" and tuple(ds["cells"].dims) == ("time", "ID")
    assert np.array_equal(np.asarray(ds["event_duration"].values), np.asarray(events["presence"].values).sum(0))
    assert np.array_equal(np.asarray(ds["cells"].values) > 0, np.asarray(events["presence"].values))
    assert np.asarray(ds["coast_edges"].values).sum() > 0
    same_bits(trk.event_shapes(events, block_steps=5), ds)
