"""GPU parity: the tracker's stages on an unstructured mesh (run_preprocess, compute_area, identify_objects,
unique_ids_in_time, calculate_object_properties, check_overlap_slice, find_overlapping_objects, enforce_overlap_threshold;
marEx/track.py:1283-1351, 1499-1518, 1932-2005, 2135-2323, 2396-2552, 2762-2764) against the NumPy oracle of
tests/mesh_objects_oracle.py -- IDs and order exact, areas, centroids and overlap areas bit-identical."""
import os
import sys

import numpy as np
import pytest
import torch

from marex_amd.exceptions import ConfigurationError, TrackingError
from marex_amd.xr_compat import DataArray

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import mesh_objects_oracle as mo  # noqa: E402
from test_mesh_tracker_host import load_mesh_fixture, mesh_tracker  # noqa: E402

pytestmark = pytest.mark.gpu

# (R_fill, T_fill, quartile, absolute) -> area threshold, clusters in the percentile, clusters kept, cells kept: computed with
# the oracle's mesh functions and a scipy temporal closing (recomputed below, pinned here)
FIXTURE_ROWS = [
    ((3, 2, 0.5, None), (83.0, 14, 7, 717)),
    ((1, 2, None, 5), (5.0, 31, 31, 1586)),
    ((1, 2, 0.25, None), (78.25, 14, 10, 953)),
    ((2, 4, 0.5, None), (85.0, 15, 7, 724)),
]


def _tri_mesh(rng, C):
    """A random 3-regular-ish neighbour table: cells on a ring with one random chord each, some neighbours missing,
    some listed from one end only (the reference treats listed pairs as undirected for clustering)."""
    nb = np.full((3, C), -1, dtype=np.int32)
    nb[0] = (np.arange(C) + 1) % C
    nb[1] = (np.arange(C) - 1) % C
    nb[2] = rng.integers(0, C, C)
    nb[2][rng.random(C) < 0.2] = -1
    nb[1][rng.random(C) < 0.05] = -1
    return nb


def _mesh(rng, C, land=0.1):
    nb0 = _tri_mesh(rng, C)
    mask = rng.random(C) >= land
    mask[rng.integers(0, C)] = True
    return {"nb0": nb0, "mask": mask, "lat": np.degrees(np.arcsin(rng.uniform(-1, 1, C))), "lon": rng.uniform(-180, 180, C),
            "areas": (10.0 ** rng.uniform(5, 8, C)).astype(np.float32)}


def _tracker(m, ev, **kw):
    return mesh_tracker(ev, m["mask"], m["nb0"] + 1, m["areas"], m["lat"], m["lon"], **kw)


def _tables(m):
    return mo.weight_tables(m["areas"], m["lat"], m["lon"])


def _same_bits(a, b):
    a, b = np.asarray(a), np.asarray(b)
    return a.dtype == b.dtype and a.shape == b.shape and a.tobytes() == b.tobytes()


def _check_props(trk, ids, q, e, what="", field=None):
    ds = trk.calculate_object_properties(ids if field is None else field, ["area", "centroid"])
    _, eid, _, earea, ecen = mo.object_properties(ids, q, e)
    gid = np.asarray(ds["ID"].values)
    assert gid.dtype == np.int64 and np.array_equal(gid, eid), what
    area, cen = np.asarray(ds["area"].values), np.asarray(ds["centroid"].values)
    assert area.dtype == np.float32 and _same_bits(area, earea), (what, np.argwhere(area != earea)[:5])
    assert cen.dtype == np.float32 and tuple(ds["centroid"].dims) == ("component", "ID") and _same_bits(cen, ecen), \
        (what, np.argwhere(cen != ecen)[:5])
    return ds


def _check_overlaps(trk, ids, q, e, what="", field=None):
    got = trk.find_overlapping_objects(ids if field is None else field)
    exp = mo.find_overlapping_objects(ids, q, e)
    assert got.dtype == np.float32 and got.shape == exp.shape and _same_bits(got, exp), what
    return got


@pytest.mark.parametrize("params,expected", FIXTURE_ROWS)
def test_reference_fixture_preprocess_and_object_stages(hot, params, expected):
    R, Tf, quart, absolute = params
    f = load_mesh_fixture()
    assert f["ev"].shape == (100, 405) and int(f["ev"].sum()) == 1557 and f["mask"].all()
    nb0 = f["nb"].astype(np.int32) - 1
    e, q = mo.weight_tables(f["areas"], f["lat"], f["lon"])
    trk = mesh_tracker(f["ev"], f["mask"], f["nb"], f["areas"], f["lat"], f["lon"], tm=f["time"], R_fill=R, T_fill=Tf,
                       area_filter_quartile=quart, area_filter_absolute=absolute, allow_merging=True, overlap_threshold=0.5)
    epre, estats = mo.run_preprocess(f["ev"], f["mask"], nb0, q, e, R, Tf, 0.5 if quart is None else quart, absolute)
    assert (estats[3], estats[1], estats[2], int(epre.sum())) == expected
    if params == FIXTURE_ROWS[0][0]:  # the reference's own ranges, tests/test_unstructured_tracking.py:351-352
        assert abs(estats[1] - 15) <= 5 and abs(estats[2] - 8) <= 2
    pre, stats = trk.run_preprocess()
    assert torch.is_tensor(pre.device_tensor) and pre.device_tensor.is_cuda and tuple(pre.dims) == ("time", "ncells")
    assert np.array_equal(pre.values.astype(bool), epre)
    assert tuple(stats) == tuple(estats), (stats, estats)

    area = trk.compute_area(pre)
    assert area.values.dtype == np.float64 and tuple(area.dims) == ("time",) and _same_bits(area.values, mo.compute_area(epre, q, e))
    objs, none, placeholder = trk.identify_objects(pre, time_connectivity=False)
    eids = mo.identify_objects(epre, f["mask"], nb0)
    assert none is None and placeholder == 1 and objs.values.dtype == np.int32 and np.array_equal(objs.values, eids)
    uniq = trk.unique_ids_in_time(objs)
    euniq = mo.unique_ids_in_time(eids)
    assert uniq.values.dtype == np.int32 and np.array_equal(uniq.values, euniq)
    from oracle import marex_oracle as orc
    assert np.array_equal(euniq, orc.label_objects_mesh(epre, f["mask"], nb0))   # the oracle's own unique-in-time form
    props = _check_props(trk, euniq, q, e, params, field=uniq)
    assert np.unique(props["ID"].values).size == props["ID"].values.size == int(euniq.max())
    ovl = _check_overlaps(trk, euniq, q, e, params, field=uniq)
    assert len(ovl) > 0
    for thr in (0.5, 0.9, 0.99):
        trk.overlap_threshold = thr
        kept = trk.enforce_overlap_threshold(ovl, props)
        assert kept.dtype == np.float32 and _same_bits(kept, mo.enforce_overlap_threshold(ovl, props["ID"].values, props["area"].values, thr))
    assert len(trk.enforce_overlap_threshold(ovl[:, [1, 0, 2]] + np.float32([10**6, 0, 0]), props)) == 0   # unknown IDs are dropped
    default = trk.calculate_object_properties(uniq)
    assert "area" in default and "centroid" not in default
    with pytest.raises(ConfigurationError, match="Unsupported object properties"):
        trk.calculate_object_properties(uniq, ["perimeter"])


@pytest.mark.parametrize("C", [1, 63, 64, 65, 405, 5000, 70001])
def test_random_meshes(hot, C):
    rng = np.random.default_rng(200 + C)
    m = _mesh(rng, C)
    e, q = _tables(m)
    for T in ((1, 2, 7) if C < 70001 else (3,)):
        for dens in ((0.02, 0.3, 0.6, 0.95) if C < 70001 else (0.1, 0.95)):
            x = rng.random((T, C)) < dens
            trk = _tracker(m, x, R_fill=0, T_fill=0)
            what = (C, T, dens)
            assert _same_bits(trk.compute_area(x).values, mo.compute_area(x, q, e)), what
            objs, _, _ = trk.identify_objects(x, time_connectivity=False)
            eids = mo.identify_objects(x, m["mask"], m["nb0"])
            assert np.array_equal(objs.values, eids), what
            euniq = mo.unique_ids_in_time(eids)
            assert np.array_equal(trk.unique_ids_in_time(objs).values, euniq), what
            for ids in (eids, euniq.astype(np.int32)):     # IDs that repeat in every timestep, and unique ones
                _check_props(trk, ids, q, e, what)
                _check_overlaps(trk, ids, q, e, what)
            if T >= 2:
                got = trk.check_overlap_slice(eids[0], eids[1])
                assert got.dtype == np.float32 and _same_bits(got, mo.check_overlap_slice(eids[0], eids[1], q, e)), what


def test_sparse_ids_event_fields_and_single_slices(hot):
    rng = np.random.default_rng(7)
    C, T = 3001, 6
    m = _mesh(rng, C, land=0.0)
    e, q = _tables(m)
    trk = _tracker(m, np.zeros((T, C), bool), R_fill=0, T_fill=0)
    base = np.where(rng.random((T, C)) < 0.5, rng.integers(1, 40, (T, C)), 0)
    runs = np.repeat(rng.integers(0, 12, (T, C // 50 + 1)), 50, axis=1)[:, :C]          # long runs of equal IDs: an event field
    for table in (np.arange(1, 41), rng.permutation(np.arange(1, 41)), np.sort(rng.choice(np.arange(1, 2**24 - 1), 40, replace=False)),
                  2**24 - 1 - np.arange(40) * 7):
        lut = np.r_[0, table].astype(np.int64)
        for field in (base, runs):
            ids = lut[field].astype(np.int32)
            _check_props(trk, ids, q, e, int(table.max()))
            _check_overlaps(trk, ids, q, e, int(table.max()))
            got = trk.check_overlap_slice(ids[2], ids[3])
            assert _same_bits(got, mo.check_overlap_slice(ids[2], ids[3], q, e))
    ids = lut[base].astype(np.int32)
    one = trk.calculate_object_properties(ids[1], ["area", "centroid"])                      # a single 1-D slice
    _, eid, _, earea, ecen = mo.object_properties(ids[1], q, e)
    assert np.array_equal(one["ID"].values, eid) and _same_bits(one["area"].values, earea) and _same_bits(one["centroid"].values, ecen)
    big = 2**31 - 2 - np.arange(40) * 5                                                     # properties take any int32 ID
    _check_props(trk, np.r_[0, big][base].astype(np.int32), q, e, "large IDs")
    zero = np.zeros((T, C), np.int32)
    ds = trk.calculate_object_properties(zero, ["area", "centroid"])
    assert ds["ID"].values.size == 0 and ds["area"].values.dtype == np.float32 and ds["centroid"].values.shape == (2, 0)
    for empty in (trk.find_overlapping_objects(zero), trk.check_overlap_slice(zero[0], ids[0]), trk.find_overlapping_objects(ids[:1]),
                  trk.enforce_overlap_threshold(np.zeros((0, 3), np.float32), ds)):
        assert empty.shape == (0, 3) and empty.dtype == np.float32


def test_label_block_steps_gives_the_same_objects(hot):
    rng = np.random.default_rng(8)
    C, T = 2000, 11
    m = _mesh(rng, C)
    x = rng.random((T, C)) < 0.4
    whole, _, _ = _tracker(m, x, R_fill=0, T_fill=0).identify_objects(x, time_connectivity=False)
    for steps in (3, 1, 11, 20):
        blocked, _, _ = _tracker(m, x, R_fill=0, T_fill=0, label_block_steps=steps).identify_objects(x, time_connectivity=False)
        assert np.array_equal(blocked.values, whole.values), steps
    assert np.array_equal(whole.values, mo.identify_objects(x, m["mask"], m["nb0"]))


def test_device_resident_input_equals_host_input(hot):
    from marex_amd.zarr_io import DeviceDataArray

    rng = np.random.default_rng(9)
    C, T = 4100, 9
    m = _mesh(rng, C)
    x = (rng.random((T, C)) < 0.35)
    x[3] = False
    coords = {"time": np.arange(T), "lat": m["lat"], "lon": m["lon"]}
    kw = dict(R_fill=1, T_fill=2, area_filter_quartile=None, area_filter_absolute=6, unstructured_grid=True,
              dimensions={"x": "ncells"}, coordinates={"x": "lon", "y": "lat"}, coordinate_units="degrees",
              neighbours=DataArray(m["nb0"] + 1, dims=("nv", "ncells")), cell_areas=DataArray(m["areas"], dims=("ncells",)))
    import marex_amd
    host = _tracker(m, x, R_fill=1, T_fill=2, area_filter_quartile=None, area_filter_absolute=6)
    hpre, hstats = host.run_preprocess()
    hobjs = host.identify_objects(hpre, False)[0]
    huniq = host.unique_ids_in_time(hobjs)
    hprops = host.calculate_object_properties(huniq, ["area", "centroid"])
    hovl = host.find_overlapping_objects(huniq)
    for dt in (torch.bool, torch.uint8):
        xd = torch.from_numpy(x).to(hot.device).to(dt)
        dev = marex_amd.tracker(DeviceDataArray(xd, ("time", "ncells"), coords), DataArray(m["mask"], dims=("ncells",)), **kw)
        pre, stats = dev.run_preprocess()
        assert tuple(stats) == tuple(hstats) and torch.equal(pre.device_tensor, hpre.device_tensor)
        assert _same_bits(dev.compute_area(pre).values, host.compute_area(hpre.values.astype(bool)).values)
        objs = dev.identify_objects(pre, False)[0]
        assert np.array_equal(objs.values, hobjs.values)
        ids_d = torch.from_numpy(huniq.values).to(hot.device)
        for field in (ids_d, ids_d.to(torch.int64), DataArray(ids_d.t().contiguous(), dims=("ncells", "time"))):
            assert np.array_equal(dev.unique_ids_in_time(torch.from_numpy(hobjs.values).to(hot.device)).values, huniq.values)
            p = dev.calculate_object_properties(field, ["area", "centroid"])
            assert np.array_equal(p["ID"].values, hprops["ID"].values) and _same_bits(p["area"].values, hprops["area"].values)
            assert _same_bits(p["centroid"].values, hprops["centroid"].values)
            assert _same_bits(dev.find_overlapping_objects(field), hovl)


def test_two_runs_return_identical_bytes(hot):
    rng = np.random.default_rng(10)
    C, T = 50000, 8
    m = _mesh(rng, C, land=0.0)
    trk = _tracker(m, np.zeros((T, C), bool), R_fill=0, T_fill=0)
    ids = np.repeat(rng.integers(0, 6, (T, C // 500)), 500, axis=1).astype(np.int32)   # few large objects: many adders per sum
    ids[rng.random((T, C)) < 0.1] = 0
    d = torch.from_numpy(ids).to(hot.device)
    first = trk.calculate_object_properties(d, ["area", "centroid"]), trk.find_overlapping_objects(d)
    for _ in range(3):
        p, o = trk.calculate_object_properties(d, ["area", "centroid"]), trk.find_overlapping_objects(d)
        assert _same_bits(p["area"].values, first[0]["area"].values) and _same_bits(p["centroid"].values, first[0]["centroid"].values)
        assert _same_bits(o, first[1])
    e, q = _tables(m)
    _check_props(trk, ids, q, e, "large objects")
    _check_overlaps(trk, ids, q, e, "large objects")


def test_a_pair_that_persists_adds_up_beyond_64_bits(hot):
    """One event over the whole mesh for 40 timesteps: its overlap with itself is 39 times the area of the mesh, 39 * 2^60
    and more in fixed point.  The sum over time is kept in two words on the device and stays exact."""
    rng = np.random.default_rng(13)
    C, T = 9000, 40
    m = _mesh(rng, C, land=0.0)
    e, q = _tables(m)
    assert 39 * int(q[0].sum()) > 2**64
    trk = _tracker(m, np.zeros((T, C), bool), R_fill=0, T_fill=0)
    ids = np.full((T, C), 7, np.int32)
    ids[:, ::3] = 2
    ids[T // 2:, 5::7] = 0
    got = _check_overlaps(trk, ids, q, e, "persisting pairs")
    assert got[:, :2].tolist() == [[2.0, 2.0], [7.0, 7.0]] and np.isfinite(got).all()
    assert got[1, 2] > np.float32(20 * 0.5 * float(np.sum(m["areas"], dtype=np.float64)))


def test_ids_of_2_24_are_refused_by_the_overlap_methods(hot):
    rng = np.random.default_rng(11)
    m = _mesh(rng, 64, land=0.0)
    trk = _tracker(m, np.zeros((2, 64), bool), R_fill=0, T_fill=0)
    ids = np.zeros((2, 64), np.int32)
    ids[0, 5], ids[1, 5] = 3, 2**24
    with pytest.raises(TrackingError, match="2\\^24"):
        trk.find_overlapping_objects(ids)
    with pytest.raises(TrackingError, match="2\\^24"):
        trk.check_overlap_slice(ids[0], ids[1])
    ids[1, 5] = 2**24 - 1
    assert trk.find_overlapping_objects(ids)[:, :2].tolist() == [[3.0, float(2**24 - 1)]]
    assert trk.calculate_object_properties(np.where(ids > 3, 2**24, ids))["ID"].values.tolist() == [3, 2**24]


def test_unique_ids_overflow_is_refused(hot):
    rng = np.random.default_rng(12)
    m = _mesh(rng, 64, land=0.0)
    trk = _tracker(m, np.zeros((3, 64), bool), R_fill=0, T_fill=0)
    ids = np.zeros((3, 64), np.int32)
    ids[:, 0] = 2**30
    with pytest.raises(TrackingError, match="2\\^31 - 2 objects"):
        trk.unique_ids_in_time(ids)
    ids[:, 0] = (2**30, 2**30 - 2, 0)     # 2^31 - 2 objects: the largest ID int32 labelling allows
    out = trk.unique_ids_in_time(ids).values
    assert out[:, 0].tolist() == [2**30, 2**31 - 2, 0] and int(out.max()) == 2**31 - 2
    ids[2, 7] = 1                         # one object more would be ID 2^31 - 1
    with pytest.raises(TrackingError, match="2\\^31 - 2 objects"):
        trk.unique_ids_in_time(ids)
