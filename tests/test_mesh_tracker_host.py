"""The mesh tracker on the host: the constructor's validation before any GPU call, the fixed-point weight tables against the
oracle, the distance of the arithmetic contract from the reference's float32 ``np.add.at`` sums (it must lie inside their
rounding bound), and the stages that are not built -- no GPU needed."""
import os
import sys

import numpy as np
import pytest

import marex_amd
from marex_amd import zarr_io
from marex_amd.exceptions import ConfigurationError, DataValidationError
from marex_amd.track import mesh_weight_tables
from marex_amd.xr_compat import DataArray

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import mesh_objects_oracle as mo  # noqa: E402

FIX = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "ref_fixtures", "extremes_unstructured.zarr")
EPS = 2.0 ** -24

# (R_fill, T_fill, quartile, absolute) of the pre-processing runs the contract bound is checked on
PRE_PARAMS = [(3, 2, 0.5, None), (1, 2, None, 5), (1, 2, 0.25, None), (2, 4, 0.5, None)]


def load_mesh_fixture():
    rd = lambda v: zarr_io.read_array(os.path.join(FIX, v))  # noqa: E731
    return {"ev": rd("extreme_events").astype(bool), "mask": rd("mask").astype(bool), "nb": rd("neighbours"),
            "areas": rd("cell_areas"), "lat": rd("lat"), "lon": rd("lon"), "time": rd("time")}


def mesh_tracker(ev, mask, nb, areas, lat, lon, tm=None, **kw):
    T, C = ev.shape
    tm = np.arange(T) if tm is None else tm
    da = DataArray(ev, dims=("time", "ncells"), coords={"time": ("time", tm), "lat": ("ncells", lat), "lon": ("ncells", lon)})
    args = dict(R_fill=1, T_fill=2, area_filter_quartile=0.5, unstructured_grid=True, dimensions={"x": "ncells"},
                coordinates={"x": "lon", "y": "lat"}, coordinate_units="degrees",
                neighbours=DataArray(nb, dims=("nv", "ncells")), cell_areas=DataArray(areas, dims=("ncells",)))
    args.update(kw)
    return marex_amd.tracker(da, DataArray(mask, dims=("ncells",)), **args)


def _small():
    rng = np.random.default_rng(1)
    C = 12
    nb = np.stack([(np.arange(C) + 1) % C + 1, (np.arange(C) - 1) % C + 1, np.zeros(C, np.int64)]).astype(np.int32)
    return dict(ev=rng.random((4, C)) < 0.5, mask=np.ones(C, bool), nb=nb, areas=np.linspace(1.0, 2.0, C).astype(np.float32),
                lat=np.linspace(-60, 60, C), lon=np.linspace(0, 359, C))


def _no_gpu(monkeypatch):
    import marex_amd.detect as det

    def no_gpu(*a, **k):
        raise AssertionError("the constructor touched the GPU engine")

    monkeypatch.setattr(det, "get_engine", no_gpu)


def _grid_da():
    ev = np.zeros((4, 6, 8), dtype=bool)
    return DataArray(ev, dims=("time", "lat", "lon"),
                     coords={"time": np.arange(4), "lat": np.linspace(-80, 80, 6), "lon": np.linspace(0, 360, 8, endpoint=False)})


CASES = [
    ("no neighbours", dict(neighbours=None), ConfigurationError, "unstructured_grid=True is not supported without neighbours and cell_areas"),
    ("no cell_areas", dict(cell_areas=None), ConfigurationError, "unstructured_grid=True is not supported without neighbours and cell_areas"),
    ("missing before dims", dict(neighbours=None, data_bin=_grid_da()), ConfigurationError, "unstructured_grid=True is not supported"),
    ("3-D data", dict(data_bin=_grid_da()), DataValidationError, "Invalid dimensions for unstructured data"),
    ("neighbour rows", dict(neighbours=DataArray(np.ones((2, 12), np.int32), dims=("nv", "ncells"))), DataValidationError,
     "Invalid neighbour array for triangular grid"),
    ("neighbour dims", dict(neighbours=DataArray(np.ones((3, 12), np.int32), dims=("vertex", "ncells"))), DataValidationError,
     "Invalid neighbour array dimensions"),
    ("neighbour beyond the mesh", dict(neighbours=DataArray(np.full((3, 12), 13, np.int32), dims=("nv", "ncells"))),
     DataValidationError, "Invalid neighbour array for triangular grid"),
    ("grid_resolution", dict(grid_resolution=1.0), DataValidationError,
     "grid_resolution parameter is not supported for unstructured grids"),
    ("regional", dict(regional_mode=True), NotImplementedError, "regional_mode is not yet implemented for unstructured grids"),
    ("cell_areas dims", dict(cell_areas=DataArray(np.ones(12, np.float32), dims=("cells",))), DataValidationError,
     "Invalid cell_areas dimensions for unstructured grid"),
    ("negative area", dict(cell_areas=DataArray(-np.ones(12, np.float32), dims=("ncells",))), DataValidationError,
     "cell_areas must be finite and non-negative"),
    ("T_fill", dict(T_fill=3), ConfigurationError, "T_fill must be even for temporal symmetry"),
    ("checkpoint", dict(checkpoint="save"), ConfigurationError, "checkpoint='save' is not supported"),
]


@pytest.mark.parametrize("name,kwargs,exc,prefix", CASES, ids=[c[0] for c in CASES])
def test_constructor_errors_before_any_gpu_call(name, kwargs, exc, prefix, monkeypatch):
    _no_gpu(monkeypatch)
    m = _small()
    kw = dict(kwargs)
    data = kw.pop("data_bin", None)
    with pytest.raises(exc) as ei:
        if data is not None:
            args = dict(R_fill=1, unstructured_grid=True, dimensions={"x": "ncells"}, coordinates={"x": "lon", "y": "lat"},
                        coordinate_units="degrees", neighbours=DataArray(m["nb"], dims=("nv", "ncells")),
                        cell_areas=DataArray(m["areas"], dims=("ncells",)))
            args.update(kw)
            marex_amd.tracker(data, DataArray(m["mask"], dims=("ncells",)), **args)
        else:
            mesh_tracker(**m, **kw)
    assert str(ei.value).startswith(prefix), str(ei.value)


def test_valid_mesh_configurations_construct_without_a_gpu(monkeypatch):
    _no_gpu(monkeypatch)
    m = _small()
    t = mesh_tracker(**m)  # allow_merging=True (the default) needs no time chunking, temp_dir is not required
    assert t.unstructured_grid and t.ydim is None and t.xdim == "ncells" and t.allow_merging
    e, q = mo.weight_tables(m["areas"], m["lat"], m["lon"])
    assert t._mesh_e == e and np.array_equal(t._mesh_q, q)
    t = mesh_tracker(**m, allow_merging=False, area_filter_quartile=None, area_filter_absolute=5, temp_dir="/nonexistent",
                     max_iteration=3, label_block_steps=2)
    assert t.area_filter_absolute == 5 and t.label_block_steps == 2
    ev_t = DataArray(np.ascontiguousarray(m["ev"].T), dims=("ncells", "time"),
                     coords={"time": ("time", np.arange(4)), "lat": ("ncells", m["lat"]), "lon": ("ncells", m["lon"])})
    t = marex_amd.tracker(ev_t, DataArray(m["mask"], dims=("ncells",)), R_fill=0, unstructured_grid=True,
                          dimensions={"x": "ncells"}, coordinates={"x": "lon", "y": "lat"}, coordinate_units="degrees",
                          neighbours=DataArray(m["nb"], dims=("nv", "ncells")), cell_areas=DataArray(m["areas"], dims=("ncells",)))
    assert t._perm == (1, 0)
    rad = mesh_tracker(m["ev"], m["mask"], m["nb"], m["areas"], np.radians(m["lat"]), np.radians(m["lon"]),
                       coordinate_units="radians")   # radians go through _unify_coordinates first
    assert np.abs(rad._mesh_q - q).max() <= 2 ** (e - 40)  # the same tables up to the rounding of the unit conversion


def test_methods_that_need_split_and_merge_raise_before_any_device_work(monkeypatch):
    _no_gpu(monkeypatch)
    t = mesh_tracker(**_small())
    x = np.zeros((4, 12), np.int32)
    for call in (lambda: t.run(), lambda: t.run(return_merges=True), lambda: t.run_tracking(x), lambda: t.track_objects(x),
                 lambda: t.split_and_merge_objects(x, None), lambda: t.consolidate_object_ids(x[0], x[1], None, 1),
                 lambda: t.cluster_rename_objects_and_props(x, None, None, None)):
        with pytest.raises(ConfigurationError, match="is not built for unstructured grids: the split-and-merge stage"):
            call()
    with pytest.raises(ConfigurationError, match="Time connectivity not supported for unstructured grids"):
        t.identify_objects(x, time_connectivity=True)


def _check_tables(areas, lat, lon):
    e, q = mesh_weight_tables(areas, lat, lon)
    oe, oq = mo.weight_tables(areas, lat, lon)
    assert e == oe and q.dtype == np.int64 and q.shape == (4, len(areas)) and q.flags["C_CONTIGUOUS"] and np.array_equal(q, oq)
    sums = [sum(int(v) for v in row) for row in q]             # exact Python integers
    mags = [sum(abs(int(v)) for v in row) for row in q]
    assert all(abs(s) < 2 ** 62 for s in sums) and all(m < 2 ** 62 for m in mags)
    assert sums[0] > 2 ** 59                                    # the scale uses the range: at most two bits are spare
    return e, q


def test_weight_tables_match_the_oracle_and_cannot_overflow():
    f = load_mesh_fixture()
    _check_tables(f["areas"], f["lat"], f["lon"])
    rng = np.random.default_rng(3)
    C = 30000
    lat, lon = np.degrees(np.arcsin(rng.uniform(-1, 1, C))), rng.uniform(-180, 180, C)
    _check_tables(10.0 ** rng.uniform(-3, 12, C), lat, lon)
    _check_tables(np.full(C, 1e-3), lat, lon)
    _check_tables(np.full(C, 1e12), lat, lon)
    _check_tables(np.r_[np.zeros(C - 1), 4.0], lat, lon)       # zero areas are allowed; a power of two as the sum
    for bad in (np.r_[1.0, np.nan], np.r_[1.0, -1e-9], np.r_[1.0, np.inf], np.zeros(2)):
        with pytest.raises(DataValidationError):
            mesh_weight_tables(bad, np.zeros(2), np.zeros(2))
    with pytest.raises(DataValidationError):
        mesh_weight_tables(np.ones(2), np.r_[0.0, np.nan], np.zeros(2))
    with pytest.raises(DataValidationError):
        mesh_weight_tables(np.ones(3), np.zeros(2), np.zeros(2))


def _contract_distance(ids, areas, lat, lon, argument_rounding=False):
    """Largest ratio (distance of the contract from the reference's float32 sums) / (rounding bound of those sums), for the
    area and for the weighted coordinate sums, over every (timestep, object) of ``ids``; and the largest object.  The bound of
    the coordinate sums is (n + 4) 2^-24 sum |a x|; with ``argument_rounding`` it is the wider one of
    test_small_objects_anywhere_on_the_sphere."""
    e, q = mo.weight_tables(areas, lat, lon)
    a64 = np.asarray(areas, np.float64)
    lat_r, lon_r = np.radians(np.asarray(lat, np.float64)), np.radians(np.asarray(lon, np.float64))
    cl, sl, co, so = np.cos(lat_r), np.sin(lat_r), np.cos(lon_r), np.sin(lon_r)
    xyz = [cl * co, cl * so, sl]
    # |d/dlat| |lat| + |d/dlon| |lon| of x, y, z: what a relative error of the angles in radians does to the unit vector
    sens = [np.abs(sl * co * lat_r) + np.abs(cl * so * lon_r), np.abs(sl * so * lat_r) + np.abs(cl * co * lon_r), np.abs(cl * lat_r)]
    worst_a = worst_c = 0.0
    biggest = 0
    for t in range(ids.shape[0]):
        u, ra, *rw = mo.reference_f32_sums(ids[t], areas, lat, lon)
        if u.size == 0:
            continue
        m = ids[t] > 0
        inv = np.searchsorted(u, ids[t][m])
        n = np.bincount(inv, minlength=u.size)
        S = np.zeros((4, u.size), np.int64)
        for k in range(4):
            np.add.at(S[k], inv, q[k][m])
        contract = S.astype(np.float64) / 2.0 ** e
        area32 = contract[0].astype(np.float32).astype(np.float64)     # what the tracker returns
        worst_a = max(worst_a, float(np.max(np.abs(area32 - ra.astype(np.float64)) / (n * EPS * ra.astype(np.float64)))))
        for k in range(3):
            mag = np.zeros(u.size)
            np.add.at(mag, inv, np.abs(a64[m] * xyz[k][m]))
            bound = (n + 4) * EPS * mag
            if argument_rounding:
                arg = np.zeros(u.size)
                np.add.at(arg, inv, a64[m] * sens[k][m])
                bound = (n + 10) * EPS * mag + 2 * EPS * arg
            ok = bound > 0
            if ok.any():
                worst_c = max(worst_c, float(np.max(np.abs(contract[k + 1] - rw[k].astype(np.float64))[ok] / bound[ok])))
        biggest = max(biggest, int(n.max()))
    return worst_a, worst_c, biggest


def test_contract_lies_inside_the_rounding_bound_of_the_reference_sums_on_the_fixture():
    """Relative distance of the contract area from a float32 np.add.at sum of n positive terms in cell order: at most
    n 2^-24; distance of the weighted coordinate sums: at most (n + 4) 2^-24 sum |a x| (the 4: the float32 rounding of
    the two trig factors and the two products)."""
    f = load_mesh_fixture()
    nb0 = f["nb"].astype(np.int32) - 1
    e, q = mo.weight_tables(f["areas"], f["lat"], f["lon"])
    for R, Tf, quart, absolute in PRE_PARAMS:
        pre, _ = mo.run_preprocess(f["ev"], f["mask"], nb0, q, e, R, Tf, 0.5 if quart is None else quart, absolute)
        ids = mo.identify_objects(pre, f["mask"], nb0)
        wa, wc, big = _contract_distance(ids, f["areas"], f["lat"], f["lon"])
        print(f"fixture {(R, Tf, quart, absolute)}: area {wa:.3f} of its bound, coordinates {wc:.3f}, largest object {big} cells")
        assert big >= 50 and wa <= 1.0 and wc <= 1.0


def _random_sphere(rng, C):
    lat = np.degrees(np.arcsin(rng.uniform(-1, 1, C))).astype(np.float32)
    return lat, rng.uniform(-180, 180, C).astype(np.float32), (10.0 ** rng.uniform(6, 8, C)).astype(np.float32)


def test_contract_lies_inside_the_rounding_bound_on_a_large_random_mesh():
    """24 000 cells spread over the whole sphere, areas over two decades, four interleaved objects of about 5 700 cells in
    every timestep: the same two bounds as on the fixture."""
    rng = np.random.default_rng(11)
    C, T = 24000, 3
    lat, lon, areas = _random_sphere(rng, C)
    ids = np.zeros((T, C), np.int32)
    for t in range(T):
        ids[t] = rng.integers(1, 5, C)
        ids[t][rng.random(C) < 0.05] = 0
    smallest = min(int(np.bincount(r)[1:].min()) for r in ids)
    wa, wc, big = _contract_distance(ids, areas, lat, lon)
    print(f"random mesh: area {wa:.4f} of its bound, coordinates {wc:.5f}, objects of {smallest} to {big} cells")
    assert smallest >= 5000 and wa <= 1.0 and wc <= 1.0


def test_small_objects_anywhere_on_the_sphere():
    """Objects of one to three cells at every longitude.  The (n + 4) 2^-24 sum |a x| bound of the two tests above counts the
    float32 rounding of the trig VALUES, which is relative to the value.  The reference also rounds the ARGUMENTS: it
    converts float32 degrees to float32 radians (one rounding of the product and one of the constant: 2 * 2^-24 relative
    to the angle, track.py:2139-2140), and near a zero of the cosine that moves the value by far more than 2^-24 of it --
    measured here on single cells: up to 2 355 times the (n + 4) bound, all of it the reference's own error, since the
    contract evaluates in float64.  With the argument term  2 * 2^-24 sum a (|dx/dlat| |lat| + |dx/dlon| |lon|)  added, and
    10 in place of 4 (two trig factors of at most 2 ulp = 4 * 2^-24 each, two products of 2^-24 each), the distance is
    bounded everywhere; the area bound n 2^-24 needs no such term."""
    rng = np.random.default_rng(12)
    C = 24000
    lat, lon, areas = _random_sphere(rng, C)
    ids = np.stack([np.arange(1, C + 1), np.arange(C) // 2 + 1, np.arange(C) // 3 + 1]).astype(np.int32)
    wa, wc, big = _contract_distance(ids, areas, lat, lon, argument_rounding=True)
    print(f"small objects: area {wa:.3f} of its bound, coordinates {wc:.3f} of the bound with the argument term")
    assert big == 3 and wa <= 1.0 and wc <= 1.0
