"""GPU parity: the basic tracker (marEx.tracker(..., allow_merging=False).run(), track.py:1162-1497) and its 3-D labelling
(track.py:2006-2048) against the host oracle of tests/track_oracle.py -- ID fields bit-identical, attrs exact."""
import os
import sys

import numpy as np
import pytest
import torch

import marex_amd
import marex_amd.track_pre as tp
from marex_amd import zarr_io
from marex_amd.xr_compat import DataArray

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import track_oracle as tor  # noqa: E402
from test_track_host import FIX, REFERENCE_ROWS, load_fixture  # noqa: E402

pytestmark = pytest.mark.gpu

ATTR_ORDER = ["allow_merging", "N_objects_prefiltered", "N_objects_filtered", "N_events_final", "R_fill", "T_fill",
              "area_filter_quartile", "area_threshold (cells)", "accepted_area_fraction", "preprocessed_area_fraction"]


def _label(hot, x, wrap=True, connect_t=True):
    T, ny, nx = x.shape
    r = hot.label_objects_3d(torch.from_numpy(np.ascontiguousarray(x).reshape(T, -1).astype(np.uint8)).to(hot.device), ny, nx,
                             wrap_x=wrap, connect_t=connect_t)
    hot.sync()
    n = int(r["n"].item())
    return r["ids"].cpu().numpy().reshape(T, ny, nx), n, r["areas"][:n].cpu().numpy()


def _check_label(hot, x, wrap, what=""):
    exp, n = tor.label_3d(x, wrap_x=wrap)
    got, m, areas = _label(hot, x, wrap)
    assert m == n, (what, m, n)
    assert np.array_equal(got, exp), what
    assert np.array_equal(areas, np.bincount(exp.reshape(-1), minlength=n + 1)[1:]), what


def _fixture_da(ev, lat, lon, tm, dims=("time", "lat", "lon"), names=("time", "lat", "lon")):
    return DataArray(ev, dims=dims, coords={names[0]: (dims[0], tm), names[1]: (dims[1], lat), names[2]: (dims[2], lon)},
                     attrs={"source": "extremes_gridded.zarr"})


@pytest.mark.parametrize("params,expected", REFERENCE_ROWS)
def test_tracker_on_the_reference_fixture(hot, params, expected):
    R, Tf, q, poles = params
    ev, mask, lat, lon, tm = load_fixture(poles)
    ds = marex_amd.tracker(_fixture_da(ev, lat, lon, tm), DataArray(mask, dims=("lat", "lon")), R_fill=R, T_fill=Tf,
                           area_filter_quartile=q, allow_merging=False, quiet=True).run()
    ids = ds["ID_field"].values
    n0, n1, nev, frac = expected
    at = ds.attrs
    assert (at["N_objects_prefiltered"], at["N_objects_filtered"], at["N_events_final"]) == (n0, n1, nev)
    assert round(at["preprocessed_area_fraction"], 4) == frac
    assert list(at)[:len(ATTR_ORDER)] == ATTR_ORDER and at["source"] == "extremes_gridded.zarr"
    exp_ids, exp_attrs = tor.run(ev, mask, R, Tf, q)
    assert at == dict(exp_attrs, source="extremes_gridded.zarr")
    assert ids.dtype == np.int32 and tuple(ds["ID_field"].dims) == ("time", "lat", "lon")
    assert np.array_equal(ids, exp_ids)
    assert int(ids.max()) == at["N_events_final"] and int(ids.min()) == 0
    assert np.array_equal(np.asarray(ds["ID_field"].coords["lat"].values), lat)
    assert np.array_equal(np.asarray(ds["ID_field"].coords["lon"].values), lon)


def test_custom_dimension_and_coordinate_names(hot):
    """test_gridded_tracking.py:322-412, no-merge half: (t, y, x) / (T, latitude, longitude) give the same events."""
    ev, mask, lat, lon, tm = load_fixture(True)
    kw = dict(area_filter_quartile=0.5, R_fill=4, T_fill=0, allow_merging=False, quiet=True)
    std = marex_amd.tracker(_fixture_da(ev, lat, lon, tm), DataArray(mask, dims=("lat", "lon")), **kw).run()
    cus = marex_amd.tracker(_fixture_da(ev, lat, lon, tm, dims=("t", "y", "x"), names=("T", "latitude", "longitude")),
                            DataArray(mask, dims=("y", "x")), dimensions={"time": "t", "x": "x", "y": "y"},
                            coordinates={"time": "T", "x": "longitude", "y": "latitude"}, **kw).run()
    assert tuple(cus["ID_field"].dims) == ("t", "y", "x")
    for c in ("T", "latitude", "longitude"):
        assert c in cus.coords, c
    assert "t" not in cus.coords
    assert np.array_equal(np.asarray(cus.coords["T"].values), tm)
    assert np.array_equal(cus["ID_field"].values, std["ID_field"].values)
    assert cus.attrs == std.attrs


def test_transposed_input_is_tracked_in_time_lat_lon_order(hot):
    ev, mask, lat, lon, tm = load_fixture(False)
    kw = dict(area_filter_quartile=0.5, R_fill=2, T_fill=2, allow_merging=False)
    a = marex_amd.tracker(_fixture_da(ev, lat, lon, tm), DataArray(mask, dims=("lat", "lon")), **kw).run()
    evt = DataArray(np.ascontiguousarray(ev.transpose(0, 2, 1)), dims=("time", "lon", "lat"),
                    coords={"time": ("time", tm), "lat": ("lat", lat), "lon": ("lon", lon)}, attrs={"source": "extremes_gridded.zarr"})
    b = marex_amd.tracker(evt, DataArray(np.ascontiguousarray(mask.T), dims=("lon", "lat")), **kw).run()
    assert np.array_equal(a["ID_field"].values, b["ID_field"].values) and a.attrs == b.attrs


def test_device_resident_input_gives_the_same_dataset(hot):
    """The extreme mask decoded in HBM (zarr_io.read_array_to_device) is tracked without a host copy of the field."""
    from marex_amd.zarr_io import DeviceDataArray

    ev, mask, lat, lon, tm = load_fixture(False)
    kw = dict(area_filter_quartile=0.5, R_fill=2, T_fill=4, allow_merging=False)
    host = marex_amd.tracker(_fixture_da(ev, lat, lon, tm), DataArray(mask, dims=("lat", "lon")), **kw).run()
    dev = zarr_io.read_array_to_device(os.path.join(FIX, "extreme_events"), hot)
    assert dev.is_cuda
    for t in (dev.to(torch.bool), dev.to(torch.uint8)):
        da = DeviceDataArray(t, ("time", "lat", "lon"), {"time": tm, "lat": lat, "lon": lon}, attrs={"source": "extremes_gridded.zarr"})
        got = marex_amd.tracker(da, DataArray(mask, dims=("lat", "lon")), **kw).run()
        assert np.array_equal(got["ID_field"].values, host["ID_field"].values)
        assert got.attrs == host.attrs
    mini = DataArray(dev.to(torch.bool), dims=("time", "lat", "lon"), coords={"time": tm, "lat": lat, "lon": lon},
                     attrs={"source": "extremes_gridded.zarr"})
    got = marex_amd.tracker(mini, DataArray(mask, dims=("lat", "lon")), **kw).run()
    assert np.array_equal(got["ID_field"].values, host["ID_field"].values)


def test_to_zarr_round_trips_the_id_field(hot, tmp_path):
    ev, mask, lat, lon, tm = load_fixture(True)
    ds = marex_amd.tracker(_fixture_da(ev, lat, lon, tm), DataArray(mask, dims=("lat", "lon")), R_fill=4, T_fill=0,
                           area_filter_quartile=0.5, allow_merging=False).run()
    store = str(tmp_path / "events.zarr")
    ds.to_zarr(store, mode="w")
    back = zarr_io.read_array(os.path.join(store, "ID_field"))
    assert back.dtype == np.int32 and np.array_equal(back, ds["ID_field"].values)
    assert zarr_io.array_attrs(store)["N_events_final"] == ds.attrs["N_events_final"]
    assert np.array_equal(zarr_io.read_array(os.path.join(store, "lat")), lat)


def test_identify_objects_both_connectivities(hot):
    ev, mask, lat, lon, tm = load_fixture(False)
    trk = marex_amd.tracker(_fixture_da(ev, lat, lon, tm), DataArray(mask, dims=("lat", "lon")), R_fill=2, allow_merging=False)
    x = ev & mask
    da = _fixture_da(x, lat, lon, tm)
    ids3, none, n3 = trk.identify_objects(da, time_connectivity=True)
    exp3, m3 = tor.label_3d(x)
    assert none is None and n3 == m3 and np.array_equal(ids3.values, exp3)
    ids2, _, n2 = trk.identify_objects(da, time_connectivity=False)
    lab2, k2 = tp.identify_objects_2d(x)
    assert n2 == k2 and _same_partition(ids2.values, lab2)
    assert np.array_equal(np.unique(ids2.values), np.arange(n2 + 1))
    # per-timestep IDs in scan order: the first object of every step has a larger ID than all objects of earlier steps
    firsts = [ids2.values[t][ids2.values[t] > 0].min() for t in range(x.shape[0]) if x[t].any()]
    assert firsts == sorted(firsts)


def _same_partition(a, b):
    if not np.array_equal(a > 0, b > 0):
        return False
    fa, fb = a[a > 0], b[b > 0]
    pairs = np.unique(np.stack([fa, fb], axis=1), axis=0)
    return pairs.shape[0] == np.unique(fa).size == np.unique(fb).size


@pytest.mark.parametrize("wrap", [True, False])
def test_labeller_fuzz(hot, wrap):
    rng = np.random.default_rng(20 + wrap)
    shapes = [(7, 19, 70), (5, 33, 130), (3, 64, 64), (1, 40, 90), (9, 1, 150), (12, 30, 1), (11, 25, 2), (6, 3, 3), (1, 1, 1),
              (2, 1, 1), (40, 1, 1)]
    for shape in shapes:
        for dens in (0.01, 0.05, 0.2, 0.4, 0.6, 0.8, 0.95):
            x = rng.random(shape) < dens
            _check_label(hot, x, wrap, (shape, dens))
        _check_label(hot, np.zeros(shape, bool), wrap, (shape, "empty"))
        _check_label(hot, np.ones(shape, bool), wrap, (shape, "full"))
    # seam-heavy: the two edge columns dense, the interior sparse
    for shape in ((8, 20, 66), (4, 7, 5)):
        x = rng.random(shape) < 0.05
        x[:, :, 0] |= rng.random(shape[:2]) < 0.5
        x[:, :, -1] |= rng.random(shape[:2]) < 0.5
        _check_label(hot, x, wrap, (shape, "seam"))


@pytest.mark.parametrize("wrap", [True, False])
def test_labeller_diagonal_in_time_only(hot, wrap):
    """A lattice whose cells never touch inside a timestep: only the (dt, dy, dx) = (1, +-1, +-1) links connect."""
    T, ny, nx = 10, 12, 70
    t, y, x = np.meshgrid(np.arange(T), np.arange(ny), np.arange(nx), indexing="ij")
    lat = ((y % 2) == (t % 2)) & ((x % 2) == (t % 2))
    assert tp.identify_objects_2d(lat, regional_mode=True)[1] == lat.sum()  # no link inside a step
    _check_label(hot, lat, wrap, "lattice")
    assert tor.label_3d(lat, wrap_x=wrap)[1] == 1


@pytest.mark.parametrize("dy", [0, 1, -1])
def test_labeller_helix_closing_through_the_seam(hot, dy):
    """One cell per step, one column further east each step: the path crosses x = nx - 1 -> 0 only from t-1 to t."""
    T, ny, nx = 30, 9, 8
    x = np.zeros((T, ny, nx), bool)
    for t in range(T):
        x[t, 4 + dy * (t % 2), t % nx] = True
    for wrap in (True, False):
        exp, n = tor.label_3d(x, wrap_x=wrap)
        assert n == (1 if wrap else (T + nx - 1) // nx)
        _check_label(hot, x, wrap, ("helix", dy, wrap))


def test_labeller_moderate_blobby_field(hot):
    """120 x 360 x 720 smoothed-noise blobs: many components across wave, workgroup and root-tile boundaries."""
    from scipy import ndimage as ndi

    rng = np.random.default_rng(4)
    T, ny, nx = 120, 360, 720
    f = ndi.gaussian_filter(rng.normal(0, 1, (T, ny, nx)).astype(np.float32), sigma=(1.0, 3.0, 4.0), mode="wrap")
    for q in (0.95, 0.7):
        x = f > np.quantile(f[::4, ::4, ::4], q)
        for wrap in (True, False):
            _check_label(hot, x, wrap, ("blobs", q, wrap))
