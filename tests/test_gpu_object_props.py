"""GPU parity: the tracker's object stages on the device (calculate_object_properties, check_overlap_slice,
find_overlapping_objects; marEx/track.py:2109-2504) against the host oracle of tests/objects_oracle.py -- IDs, order,
area and centroid bit-identical, overlap tables exact."""
import os
import sys

import numpy as np
import pytest
import torch

import marex_amd
from marex_amd.exceptions import DataValidationError
from marex_amd.xr_compat import DataArray

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import objects_oracle as oo  # noqa: E402
from test_track_host import REFERENCE_ROWS, load_fixture  # noqa: E402

pytestmark = pytest.mark.gpu

NX_LIST = [1, 50, 100, 150, 199, 200, 201, 360]


def _tracker(regional_mode=False, **kw):
    ev = np.zeros((2, 3, 4), dtype=bool)
    ev[0, 1, 1] = True
    da = DataArray(ev, dims=("time", "lat", "lon"), coords={"time": np.arange(2), "lat": np.arange(3.0), "lon": np.arange(4.0)})
    return marex_amd.tracker(da, DataArray(np.ones((3, 4), dtype=bool), dims=("lat", "lon")), R_fill=0, allow_merging=False,
                             regional_mode=regional_mode, **kw)


def _check_props(trk, ids, what="", field=None):
    """calculate_object_properties(field or ids, ["area", "centroid"]) == the oracle of ``ids`` ((T, y, x) or (y, x))."""
    ds = trk.calculate_object_properties(ids if field is None else field, ["area", "centroid"])
    eid, earea, ec = oo.object_properties(ids, trk.regional_mode)
    gid = np.asarray(ds["ID"].values)
    assert gid.dtype == np.int64 and np.array_equal(gid, eid), what
    area = np.asarray(ds["area"].values)
    assert area.dtype == np.float64 and np.array_equal(area, earea), what
    c = np.asarray(ds["centroid"].values)
    assert c.dtype == np.float64 and c.shape == (2, eid.size) and tuple(ds["centroid"].dims) == ("component", "ID"), what
    assert np.array_equal(c, ec), (what, np.argwhere(c != ec)[:5])
    return ds


def _check_overlaps(trk, ids, what="", field=None):
    got = trk.find_overlapping_objects(ids if field is None else field)
    exp = oo.find_overlapping_objects(ids)
    assert got.dtype == np.int32 and got.shape == exp.shape and np.array_equal(got, exp), what
    return got


def _fixture_da(x, lat, lon, tm):
    return DataArray(x, dims=("time", "lat", "lon"), coords={"time": ("time", tm), "lat": ("lat", lat), "lon": ("lon", lon)})


@pytest.mark.parametrize("params,expected", REFERENCE_ROWS)
def test_reference_fixture_objects_and_events(hot, params, expected):
    """Per-timestep objects (identify_objects(time_connectivity=False) of the pre-processed mask) and the events of
    run(): properties and overlaps exact, then the threshold on the per-timestep objects as in track_objects."""
    R, Tf, q, poles = params
    ev, mask, lat, lon, tm = load_fixture(poles)
    trk = marex_amd.tracker(_fixture_da(ev, lat, lon, tm), DataArray(mask, dims=("lat", "lon")), R_fill=R, T_fill=Tf,
                            area_filter_quartile=q, allow_merging=False)
    pre, _ = trk.run_preprocess()
    objs, _, n = trk.identify_objects(pre, time_connectivity=False)
    ids = objs.values
    props = _check_props(trk, ids, ("objects", params), field=objs)
    assert props["ID"].values.size == n and np.unique(props["ID"].values).size == n
    ovl = _check_overlaps(trk, ids, ("objects", params), field=objs)
    kept = trk.enforce_overlap_threshold(ovl, props)
    assert np.array_equal(kept, oo.enforce_overlap_threshold(ovl, props["ID"].values, props["area"].values, 0.5))
    events = trk.run()["ID_field"]
    assert int(events.values.max()) == expected[2]
    _check_props(trk, events.values, ("events", params), field=events)
    _check_overlaps(trk, events.values, ("events", params), field=events)
    default = trk.calculate_object_properties(events)
    assert "area" in default and "centroid" not in default


@pytest.mark.parametrize("regional_mode", [False, True])
def test_fuzz_shapes_and_densities(hot, regional_mode):
    rng = np.random.default_rng(40 + regional_mode)
    trk = _tracker(regional_mode)
    shapes = [(1, 7, 50), (4, 1, 360), (3, 9, 1), (2, 1, 1)] + [(3, 11, nx) for nx in NX_LIST] + [(5, 70, 131)]
    for shape in shapes:
        for dens in (0.0, 0.02, 0.3, 0.8, 1.0):
            k = max(1, int(rng.integers(1, 30)))
            ids = np.where(rng.random(shape) < dens, rng.integers(1, k + 1, shape), 0).astype(np.int32)
            _check_props(trk, ids, (shape, dens))
            _check_overlaps(trk, ids, (shape, dens))


@pytest.mark.parametrize("regional_mode", [False, True])
def test_seam_straddling_blobs(hot, regional_mode):
    trk = _tracker(regional_mode)
    for nx in NX_LIST + [1440]:
        ids = np.zeros((3, 12, nx), np.int32)
        for t in range(3):
            w = 1 + 3 * t
            cols = np.r_[0:min(w, nx), max(0, nx - 2 * w):nx]
            ids[t, 2:6][:, cols] = 5 + t                   # across the seam; its mean goes negative for t > 0
            ids[t, 7:9, : min(nx, 2 + t)] = 9               # touches the left band only ...
            ids[t, 9, nx - 1] = 9                           # ... and the right band with one cell
        _check_props(trk, ids, nx)
        _check_overlaps(trk, ids, nx)


def test_permuted_gapped_and_large_ids(hot):
    rng = np.random.default_rng(5)
    trk = _tracker()
    base = np.where(rng.random((6, 40, 90)) < 0.4, rng.integers(1, 60, (6, 40, 90)), 0)
    for table in (rng.permutation(np.arange(1, 61)),
                  np.sort(rng.choice(np.arange(1, 10**6), 60, replace=False)),
                  2**31 - 2 - np.arange(60) * 7,
                  np.r_[1, 2**31 - 2, rng.integers(3, 2**31 - 3, 58)]):
        lut = np.r_[0, table].astype(np.int64)
        ids = lut[base].astype(np.int32)
        _check_props(trk, ids, int(table.max()))
        _check_overlaps(trk, ids, int(table.max()))


def test_id_reappearing_after_a_gap_and_empty_slices(hot):
    trk = _tracker()
    ids = np.zeros((7, 10, 30), np.int32)
    ids[0, 2:4, 3:8] = 4
    ids[1, 2:5, 4:9] = 4       # slices 2, 3 empty
    ids[4, 0:2, 0:30] = 4      # the same ID three steps later, across the whole row
    ids[4, 5:7, 5:7] = 2
    ids[5, 5:7, 6:8] = 4
    ids[6, 1:3, 28:30] = 3
    ds = _check_props(trk, ids, "gap")
    assert ds["ID"].values.tolist() == [4, 4, 2, 4, 4, 3]
    ovl = _check_overlaps(trk, ids, "gap")
    assert ovl.tolist() == [[2, 4, 2], [4, 4, 8]]
    zero = np.zeros((5, 8, 9), np.int32)
    ds = trk.calculate_object_properties(zero, ["area", "centroid"])
    assert ds["ID"].values.size == 0 and ds["area"].values.size == 0 and ds["centroid"].values.shape == (2, 0)
    assert trk.find_overlapping_objects(zero).shape == (0, 3)
    assert trk.find_overlapping_objects(zero).dtype == np.int32


def test_two_dimensional_field_and_check_overlap_slice(hot):
    rng = np.random.default_rng(6)
    trk = _tracker()
    a = np.where(rng.random((30, 200)) < 0.5, rng.integers(1, 9, (30, 200)), 0).astype(np.int32)
    b = np.where(rng.random((30, 200)) < 0.5, rng.integers(1, 9, (30, 200)), 0).astype(np.int32)
    _check_props(trk, a, "2-D")
    _check_props(trk, a, "2-D transposed", field=DataArray(np.ascontiguousarray(a.T), dims=("lon", "lat")))
    got = trk.check_overlap_slice(a, b)
    assert got.dtype == np.int32 and np.array_equal(got, oo.check_overlap_slice(a, b))
    assert np.array_equal(trk.check_overlap_slice(torch.from_numpy(a).to(hot.device), b), got)
    assert trk.check_overlap_slice(a, np.zeros_like(b)).shape == (0, 3)
    assert trk.find_overlapping_objects(a).shape == (0, 3)   # one slice: nothing after it


def test_device_input_equals_host_input(hot):
    from marex_amd.zarr_io import DeviceDataArray

    rng = np.random.default_rng(7)
    trk = _tracker()
    ids = np.where(rng.random((5, 30, 70)) < 0.3, rng.integers(1, 40, (5, 30, 70)), 0).astype(np.int32)
    host = trk.calculate_object_properties(ids, ["centroid"])
    for dt in (torch.int32, torch.int64, torch.int16):
        t = torch.from_numpy(ids).to(hot.device).to(dt)
        for field in (DeviceDataArray(t, ("time", "lat", "lon"), {"time": np.arange(5)}),
                      DataArray(t.permute(2, 0, 1), dims=("lon", "time", "lat"))):
            dev = trk.calculate_object_properties(field, ["centroid"])
            assert np.array_equal(dev["ID"].values, host["ID"].values) and np.array_equal(dev["centroid"].values, host["centroid"].values)
            assert np.array_equal(trk.find_overlapping_objects(field), oo.find_overlapping_objects(ids))
    with pytest.raises(DataValidationError, match="non-negative"):
        trk.calculate_object_properties(torch.from_numpy(-ids - 1).to(hot.device))
    with pytest.raises(DataValidationError, match="fit int32"):
        trk.find_overlapping_objects(torch.full((2, 3, 4), 2**31, dtype=torch.int64, device=hot.device))


def test_hash_stress_every_cell_its_own_id(hot):
    trk = _tracker()
    T, ny, nx = 3, 64, 300
    ids = np.arange(1, T * ny * nx + 1, dtype=np.int32).reshape(T, ny, nx)
    _check_props(trk, ids, "stress")
    ovl = _check_overlaps(trk, ids, "stress")
    assert ovl.shape == ((T - 1) * ny * nx, 3) and (ovl[:, 2] == 1).all()
    shuf = np.random.default_rng(9).permutation(ids.reshape(-1)).reshape(T, ny, nx)
    _check_overlaps(trk, shuf, "stress shuffled")


def test_medium_blobby_field(hot):
    """200 x 720 x 1440 smoothed-noise blobs: per-timestep objects and events of the device labeller."""
    from scipy import ndimage as ndi

    rng = np.random.default_rng(10)
    T, ny, nx = 200, 720, 1440
    f = ndi.gaussian_filter(rng.normal(0, 1, (T, ny // 2, nx // 2)).astype(np.float32), sigma=(1.0, 3.0, 4.0), mode="wrap")
    x = np.repeat(np.repeat(f > np.quantile(f[::4, ::4, ::4], 0.9), 2, axis=1), 2, axis=2)
    trk = _tracker()
    da = DataArray(x, dims=("time", "lat", "lon"), coords={"time": np.arange(T)})
    for tc in (False, True):
        objs, _, n = trk.identify_objects(da, time_connectivity=tc)
        ids = objs.values
        _check_props(trk, ids, ("medium", tc), field=objs)
        _check_overlaps(trk, ids, ("medium", tc), field=objs)
