"""mesh_event_shapes on the device against the brute-force oracle of tests/mesh_event_shapes_oracle.py: every integer output
and every ldexp of one with ==, the derived floats within 1e-12 (relative; the squared axis lengths relative to the squared
major axis; the orientation absolute at 1e-12 tr / root) -- both sides apply about a dozen correctly rounded float64
operations to the same exact integers, the margin covers libm differences.  The shapes are the smallest at which the kernel
can go wrong: a wave walks MSH_ITERS = 16 pieces of 64 cells (1024 cells), a workgroup of four waves MSH_CHUNK = 4096 cells,
loaded MSH_BATCH = 4 pieces at a time, and a workgroup strides over the rows by MSH_TSTRIDE = 64."""
import os
import sys

import numpy as np
import pytest
import torch

import marex_amd
from marex_amd.exceptions import ProcessingError
from marex_amd.shapes_mesh import coordinate_keys, mesh_edge_weight_table, mesh_shape_tables

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import mesh_event_shapes_cases as mc  # noqa: E402
import mesh_event_shapes_oracle as so  # noqa: E402
from mesh_event_shapes_host_engine import HostEngine  # noqa: E402

pytestmark = pytest.mark.gpu


def same_bits(a, b):
    assert list(a.data_vars) == list(b.data_vars)
    for k in a.data_vars:
        u, v = np.asarray(a[k].values), np.asarray(b[k].values)
        assert u.dtype == v.dtype and u.tobytes() == v.tobytes(), k


def check(ids, nbr0, lat, lon, blocks=(), resident=False, **kw):
    T = ids.shape[0]
    steps, events = so.mesh_event_shapes(ids, nbr0, lat, lon, **kw)
    base = marex_amd.mesh_event_shapes(ids, nbr0 + 1, lat, lon, **kw)
    so.compare(base, steps, events, T)
    for b in blocks:
        same_bits(marex_amd.mesh_event_shapes(ids, nbr0 + 1, lat, lon, block_steps=b, **kw), base)
    if resident:
        dev = torch.from_numpy(ids).to("cuda:0")
        same_bits(marex_amd.mesh_event_shapes(dev, nbr0 + 1, lat, lon, **kw), base)
        same_bits(marex_amd.mesh_event_shapes(dev, nbr0 + 1, lat, lon, block_steps=3, **kw), base)
    return base, steps, events


@pytest.mark.parametrize("C", [1, 63, 64, 65, 255, 256, 257, 1023, 1024, 1025, 4095, 4096, 4097])
def test_cells_either_side_of_a_piece_a_batch_a_wave_and_a_workgroup(hot, C):
    nbr0 = mc.ring(C)
    lat, lon = mc.geometry(C, C)
    ids = mc.make_field(3, nbr0, C, n_ev=4, big=min(C, 150))
    ids[1, max(0, C - 130):] = 10  # a run across the last pieces, up to the last cell
    check(ids, nbr0, lat, lon, blocks=(1,))
    check(ids, nbr0, lat, lon, resident=True, **mc.tables(C, C + 1))


@pytest.mark.parametrize("T", [63, 64, 65])
def test_steps_either_side_of_the_row_stride(hot, T):
    nbr0 = mc.ragged(mc.triangular(7, 19), 3)
    lat, lon = mc.geometry(133, 5, grid=(7, 19))
    ids = mc.make_field(T, nbr0, T, n_ev=6, big=25)
    check(ids, nbr0, lat, lon, blocks=(1, 3), resident=True, **mc.tables(133, 6))


@pytest.mark.parametrize("mesh", ["triangular", "permuted", "ragged"])
def test_row_triangular_meshes(hot, mesh):
    ny, nx = (40, 70) if mesh == "triangular" else (59, 70)  # 2800 cells: three waves; 4130: a second workgroup
    C = ny * nx
    nbr0 = mc.triangular(ny, nx)
    lat, lon = mc.geometry(C, 7, grid=(ny, nx))
    if mesh == "permuted":  # neighbours in other waves and workgroups, many events in a 64-cell piece
        nbr0, new = mc.permuted(nbr0, 8)
        lat, lon = lat[np.argsort(new)], lon[np.argsort(new)]
    if mesh == "ragged":
        nbr0 = mc.ragged(nbr0, 9)
    ids = mc.make_field(5, nbr0, 10, n_ev=10, big=120)
    ids[2] = 29  # one event covers a whole slice
    assert ids.max() == ids[-1, -1] == 32
    base, steps, events = check(ids, nbr0, lat, lon, blocks=(1, 3), resident=True)
    assert steps[(2, 29)]["cells"] == C and steps[(2, 29)]["edges"] == steps[(2, 29)]["border_edges"]  # only the mesh's own rim
    assert steps[(2, 29)]["contact_edges"] == 0
    assert events[2]["event_duration"] == 0 and events[1]["event_duration"] > 0  # sparse numbers: an event without a cell
    assert any(events[e]["event_duration"] < max(t for (t, k) in steps if k == e) - min(t for (t, k) in steps if k == e) + 1
               for e in events if events[e]["event_duration"])  # an event absent inside its span
    check(ids, nbr0, lat, lon, blocks=(3,), **mc.tables(C, 11))


def test_an_id_above_the_declared_events_next_to_an_event_and_a_cell_outside_its_span(hot):
    """The engine call itself, against the NumPy stand-in: a value above n_ev is background for the sums and a contact for
    its neighbours; an event outside its declared span is counted in status, not accumulated."""
    C, T = 300, 4
    nbr0 = mc.ring(C)
    lat, lon = mc.geometry(C, 2)
    t = mc.tables(C, 3)
    _, q = mesh_shape_tables(t["cell_areas"], lat, lon)
    _, len_q = mesh_edge_weight_table(t["edge_lengths"], C)
    lat_k, lon_k = coordinate_keys(lat, lon)
    ids = np.zeros((T, C), np.int32)
    ids[:, 60:70] = 1
    ids[1:3, 70:80] = 2
    ids[:, 80:90] = 7     # above n_ev = 2, beside event 2
    ids[0, 59] = 2**31 - 1
    tmin, tmax = np.array([2**31 - 1, 0, 1]), np.array([-1, 3, 2])
    dev = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(hot.device)  # noqa: E731
    args = dict(mask=t["mask"].view(np.uint8), len_q=len_q, lat_k=lat_k, lon_k=lon_k)
    got = hot.mesh_event_shapes(dev(ids), dev(nbr0), dev(q), tmin, tmax, **{k: dev(v) for k, v in args.items()})
    exp = HostEngine().mesh_event_shapes(torch.from_numpy(ids), torch.from_numpy(nbr0), torch.from_numpy(q), tmin, tmax,
                                         **{k: torch.from_numpy(np.ascontiguousarray(v)) for k, v in args.items()})
    assert np.array_equal(got["mom"], exp["mom"]) and np.array_equal(got["box"], exp["box"])
    # contacts: event 1 faces the huge value at step 0 and event 2 at step 1; event 2 (slots 4, 5) faces event 1 and the 7s
    assert got["mom"][0, 15] == 1 and got["mom"][1, 15] == 1 and got["mom"][4, 15] == 2
    plain = hot.mesh_event_shapes(dev(ids), dev(nbr0), dev(q), tmin, tmax)
    assert np.array_equal(plain["mom"][:, :13], exp["mom"][:, :13]) and (plain["mom"][:, 13:15] == 0).all()
    assert (plain["box"][:, 0::2] == 2**31 - 1).all() and (plain["box"][:, 1::2] == -2**31).all()
    with pytest.raises(ProcessingError, match="20 cells belong to an event outside its declared span"):
        hot.mesh_event_shapes(dev(ids), dev(nbr0), dev(q), tmin, np.array([-1, 1, 2]))  # event 1 declared for steps 0 .. 1
    with pytest.raises(ProcessingError, match="nbr must be a contiguous"):
        hot.mesh_event_shapes(dev(ids), dev(nbr0[:2]), dev(q), tmin, tmax)
    with pytest.raises(ProcessingError, match="lat_k and lon_k come together"):
        hot.mesh_event_shapes(dev(ids), dev(nbr0), dev(q), tmin, tmax, lat_k=dev(lat_k))


@pytest.mark.parametrize("seed", range(20))
def test_fuzz(hot, seed):
    rng = np.random.default_rng(3000 + seed)
    T = int(rng.integers(1, 71))
    kind = seed % 3
    if kind == 0:
        C = int(rng.integers(1, 4200))
        nbr0, grid = mc.ring(C), None
    else:
        ny = int(rng.integers(1, 60))
        nx = int(rng.integers(1, max(2, min(200, 4200 // ny))))
        C, grid = ny * nx, (ny, nx)
        nbr0 = mc.triangular(ny, nx)
        if kind == 2:
            nbr0 = mc.ragged(mc.permuted(nbr0, seed)[0], seed)
    lat, lon = mc.geometry(C, seed, grid=grid if kind == 1 else None)
    ids = mc.make_field(T, nbr0, seed, n_ev=int(rng.integers(1, 9)), big=int(rng.integers(1, 60)))
    kw = mc.tables(C, seed) if seed % 2 else {}
    if seed % 4 == 1:
        kw.pop("mask")
    check(ids, nbr0, lat, lon, blocks=(int(rng.integers(1, 6)),), resident=bool(seed % 5 == 0), **kw)


def test_mesh_merge_tracker_end_to_end(hot):
    from test_gpu_mesh_events import _host_mask, _remapped, _run_fixture_tracker
    from test_mesh_merge_host import load_merging_fixture

    f = load_merging_fixture()
    trk = _run_fixture_tracker(f, _host_mask(f), 5)
    events, _ = trk.run(return_merges=True)
    N = int(events["ID"].values.size)
    assert N == 11
    ds = trk.event_shapes(events)
    pres = np.asarray(events["presence"].values)
    assert np.array_equal(np.asarray(ds["cells"].values) > 0, pres)
    assert np.array_equal(np.asarray(ds["event_duration"].values), pres.sum(0))
    area = np.asarray(ds["area"].values).astype(np.float32)
    assert np.array_equal(area[pres], np.asarray(events["area"].values)[pres])
    cen = _remapped(np.stack([np.asarray(ds["centroid_lat"].values), np.asarray(ds["centroid_lon"].values)]).astype(np.float32),
                    f["lon"])
    assert np.array_equal(cen[:, pres], np.asarray(events["centroid"].values)[:, pres])
    field = np.asarray(events["ID_field"].values)
    steps, evs = so.mesh_event_shapes(field, f["nb0"], trk.lat, trk.lon, cell_areas=f["areas"], mask=f["mask"], n_events=N)
    so.compare(ds, steps, evs, field.shape[0], tvals=f["time"])
    assert tuple(ds["cells"].dims) == ("time", "ID") and ds.attrs["distance_units"] == "km"
    same_bits(trk.event_shapes(events, block_steps=7), ds)
