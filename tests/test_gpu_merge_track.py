"""GPU parity: the merge tracker (marEx.tracker(..., allow_merging=True).run(return_merges=True), gridded data,
track.py:2554-3802) against the host oracle of tests/merge_oracle.py -- every variable, coordinate, dtype and attribute
(in order) equal; bitwise with unit cell areas, rtol 1e-6 on area and centroid with grid_resolution."""
import os
import sys

import numpy as np
import pytest
import torch

import marex_amd
from marex_amd import zarr_io
from marex_amd.xr_compat import DataArray

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import merge_oracle as mo  # noqa: E402
import track_oracle as tor  # noqa: E402
from test_track_host import FIX, load_fixture  # noqa: E402

pytestmark = pytest.mark.gpu

VARS = ["ID_field", "global_ID", "area", "centroid", "presence", "time_start", "time_end", "merge_ledger"]
ATTRS = ["allow_merging", "N_objects_prefiltered", "N_objects_filtered", "N_events_final", "R_fill", "T_fill",
         "area_filter_quartile", "area_threshold (cells)", "accepted_area_fraction", "preprocessed_area_fraction",
         "overlap_threshold", "nn_partitioning", "total_merges", "multi_parent_merges"]


def _fixture_time():
    return zarr_io.read_dataset(FIX)["time"].values


def _oracle(ev, mask, tv, lat, lon, chunks, R, Tf, q=0.5, nn=False, regional=False, grid_resolution=None, units="degrees",
            thr=0.5):
    e, st = tor.preprocess(ev, mask, R, Tf, q, None, regional)
    lat_d = lat * 180.0 / np.pi if units == "radians" else lat
    lon_d = lon * 180.0 / np.pi if units == "radians" else lon
    w = mo.cell_weights(*ev.shape[1:], lat_d, grid_resolution) if grid_resolution else None
    out, mds, _ = mo.track(e, tv, lat_d, lon_d, chunks, thr, nn, regional, w, lon_init=lon, units=units)
    N = int(out["ID_field"].max())
    attrs = {"allow_merging": 1, "N_objects_prefiltered": st[1], "N_objects_filtered": st[2], "N_events_final": N,
             "R_fill": R, "T_fill": Tf, "area_filter_quartile": q, "area_threshold (cells)": st[3],
             "accepted_area_fraction": st[4], "preprocessed_area_fraction": st[5], "overlap_threshold": thr,
             "nn_partitioning": int(nn), "total_merges": len(mds["n_parents"]),
             "multi_parent_merges": int((mds["n_parents"] > 2).sum())}
    return out, attrs, mds


def _check(ds, merges, exp, attrs, mds, tv, lat, lon, rtol=0.0, names=("time", "lat", "lon")):
    tn, yn, xn = names
    assert list(ds.data_vars) == VARS
    for k in VARS:
        got = np.asarray(ds[k].values)
        want = np.asarray(exp[k])
        assert got.dtype == want.dtype, (k, got.dtype, want.dtype)
        assert got.shape == want.shape, (k, got.shape, want.shape)
        if rtol and k in ("area", "centroid"):
            # the reference sums cell areas in float32 (order-dependent): a last-bit change of that total moves a centroid
            # by up to ~1e-7 of the summed x, which the seam shift can leave next to a small longitude (hence the atol)
            np.testing.assert_allclose(got, want, rtol=rtol, atol=1e-4 if k == "centroid" else 0, equal_nan=True, err_msg=k)
        else:
            assert np.array_equal(got, want, equal_nan=want.dtype.kind == "f"), k
    N = attrs["N_events_final"]
    assert np.array_equal(ds["ID"].values, np.arange(1, N + 1, dtype=np.int32)) and ds["ID"].values.dtype == np.int32
    assert np.array_equal(ds[tn].values, tv)
    assert np.array_equal(ds[yn].values, lat) and np.array_equal(ds[xn].values, lon)
    assert list(ds["component"].values) == [0, 1]
    assert tuple(ds["ID_field"].dims) == ("time", "lat", "lon") or tn != "time"
    assert tuple(ds["merge_ledger"].dims)[1:] == ("ID", "sibling_ID")
    assert list(ds.attrs)[:len(ATTRS)] == ATTRS
    for k in ATTRS:
        assert ds.attrs[k] == attrs[k], (k, ds.attrs[k], attrs[k])
    assert list(merges.data_vars) == list(mds)
    for k in mds:
        got = np.asarray(merges[k].values)
        assert got.dtype == mds[k].dtype and np.array_equal(got, mds[k]), k
    assert merges.attrs["fill_value"] == -1


def _da(ev, tv, lat, lon, names=("time", "lat", "lon")):
    tn, yn, xn = names
    return DataArray(ev, dims=names, coords={tn: (tn, tv), yn: (yn, lat), xn: (xn, lon)}, name="extreme_events")


@pytest.mark.parametrize("nn", [False, True])
@pytest.mark.parametrize("tc", [1, 2, 3, 32])
def test_fixture_matches_oracle(nn, tc):
    ev, mask, lat, lon, _ = load_fixture(True)
    tv = _fixture_time()
    exp, attrs, mds = _oracle(ev, mask, tv, lat, lon, mo.chunk_layout(32, tc), 4, 2, nn=nn)
    trk = marex_amd.tracker(_da(ev, tv, lat, lon), DataArray(mask, dims=("lat", "lon")), R_fill=4, T_fill=2,
                            area_filter_quartile=0.5, allow_merging=True, nn_partitioning=nn, timechunks=tc)
    ds, merges = trk.run(return_merges=True)
    _check(ds, merges, exp, attrs, mds, tv, lat, lon)
    if tc == 2:  # the reference's test ranges (test_tracking_data_consistency / test_advanced_tracking_with_merging)
        assert abs(attrs["N_events_final"] - (20 if nn else 21)) <= 1
        assert abs(attrs["total_merges"] - (13 if nn else 15)) <= 2


def test_store_chunks_and_device_input():
    ds0 = zarr_io.read_dataset(FIX)
    ev0 = ds0["extreme_events"]
    assert tuple(ev0.encoding["chunks"])[0] == 2
    ev, mask, lat, lon, _ = load_fixture(True)
    tv = _fixture_time()
    exp, attrs, mds = _oracle(ev, mask, tv, lat, lon, mo.chunk_layout(32, 2), 4, 2)
    da = DataArray(ev0.values.astype(bool), dims=ev0.dims, coords={k: ev0.coords[k] for k in ev0.coords})
    da.encoding["chunks"] = ev0.encoding["chunks"]
    trk = marex_amd.tracker(da, DataArray(mask, dims=("lat", "lon")), R_fill=4, T_fill=2)
    _check(*trk.run(return_merges=True), exp, attrs, mds, tv, lat, lon)
    hot = marex_amd.detect.get_engine(0)
    dev = zarr_io.open_dataarray_device(FIX, "extreme_events", hot, ("time", "lat", "lon"), coords={"lat": lat, "lon": lon})
    assert tuple(dev.encoding["chunks"])[0] == 2
    dev = zarr_io.DeviceDataArray(dev.device_tensor != 0, dev.dims, dev.coords)  # int8 store -> a bool mask in HBM
    dev.encoding["chunks"] = (2, 180, 360)
    trk = marex_amd.tracker(dev, DataArray(mask, dims=("lat", "lon")), R_fill=4, T_fill=2)
    _check(*trk.run(return_merges=True), exp, attrs, mds, tv, lat, lon)


def test_grid_resolution_custom_names_and_radians():
    ev, mask, lat, lon, _ = load_fixture(True)
    tv = _fixture_time()
    exp, attrs, mds = _oracle(ev, mask, tv, lat, lon, mo.chunk_layout(32, 3), 4, 2, grid_resolution=1.0)
    trk = marex_amd.tracker(_da(ev, tv, lat, lon), DataArray(mask, dims=("lat", "lon")), R_fill=4, T_fill=2,
                            grid_resolution=1.0, timechunks=3)
    _check(*trk.run(return_merges=True), exp, attrs, mds, tv, lat, lon, rtol=1e-6)
    names = ("t", "yy", "xx")
    exp, attrs, mds = _oracle(ev, mask, tv, lat, lon, mo.chunk_layout(32, 5), 4, 2, nn=True)
    trk = marex_amd.tracker(_da(ev, tv, lat, lon, names), DataArray(mask, dims=names[1:]), R_fill=4, T_fill=2, timechunks=5,
                            nn_partitioning=True, dimensions={"time": "t", "y": "yy", "x": "xx"})
    _check(*trk.run(return_merges=True), exp, attrs, mds, tv, lat, lon, names=names)
    latr, lonr = np.radians(lat).astype(np.float32), np.radians(lon).astype(np.float32)
    exp, attrs, mds = _oracle(ev, mask, tv, latr, lonr, mo.chunk_layout(32, 2), 4, 2, units="radians")
    trk = marex_amd.tracker(_da(ev, tv, latr, lonr), DataArray(mask, dims=("lat", "lon")), R_fill=4, T_fill=2, timechunks=2)
    _check(*trk.run(return_merges=True), exp, attrs, mds, tv, latr, lonr)


def _blobs(T, ny, nx, n, seed, rmax=9.0):
    """Drifting discs that collide and split, some across the x seam."""
    rng = np.random.default_rng(seed)
    yy, xx = np.mgrid[0:ny, 0:nx]
    y0, x0 = rng.uniform(0, ny, n), rng.uniform(0, nx, n)
    vy, vx = rng.uniform(-1.5, 1.5, n), rng.uniform(-3, 3, n)
    r = rng.uniform(3, rmax, n)
    out = np.zeros((T, ny, nx), bool)
    for t in range(T):
        for k in range(n):
            cy, cx = y0[k] + vy[k] * t, (x0[k] + vx[k] * t) % nx
            dx = np.abs(xx - cx)
            dx = np.minimum(dx, nx - dx)
            out[t] |= (yy - cy) ** 2 + dx ** 2 <= (r[k] * (1 + 0.3 * np.sin(t / 3 + k))) ** 2
    return out


@pytest.mark.parametrize("seed,nn,regional,tc", [(1, False, False, 4), (2, True, False, 3), (3, False, True, 1),
                                                 (4, True, True, 7)])
def test_fuzz_colliding_blobs(seed, nn, regional, tc):
    T, ny, nx = 24, 60, 240
    ev = _blobs(T, ny, nx, 40, seed)
    mask = np.ones((ny, nx), bool)
    lat = np.linspace(-59.5, 59.5, ny).astype(np.float32)
    lon = np.linspace(0.75, 359.25, nx).astype(np.float32)
    tv = np.arange(T).astype("datetime64[D]").astype("datetime64[ns]")
    exp, attrs, mds = _oracle(ev, mask, tv, lat, lon, mo.chunk_layout(T, tc), 1, 2, q=0.2, nn=nn, regional=regional)
    assert attrs["total_merges"] > 0
    trk = marex_amd.tracker(_da(ev, tv, lat, lon), DataArray(mask, dims=("lat", "lon")), R_fill=1, T_fill=2,
                            area_filter_quartile=0.2, nn_partitioning=nn, regional_mode=regional, timechunks=tc,
                            coordinate_units="degrees")
    _check(*trk.run(return_merges=True), exp, attrs, mds, tv, lat, lon)
    if seed == 1:
        assert (mds["n_parents"] > 2).any() or (mds["n_parents"] == 2).any()


def test_large_field():
    T, ny, nx = 60, 360, 720
    ev = _blobs(T, ny, nx, 160, 11, rmax=24.0)
    mask = np.ones((ny, nx), bool)
    lat = np.linspace(-89.75, 89.75, ny).astype(np.float32)
    lon = np.linspace(0.25, 359.75, nx).astype(np.float32)
    tv = np.arange(T).astype("datetime64[D]").astype("datetime64[ns]")
    exp, attrs, mds = _oracle(ev, mask, tv, lat, lon, mo.chunk_layout(T, 8), 2, 2)
    trk = marex_amd.tracker(_da(ev, tv, lat, lon), DataArray(mask, dims=("lat", "lon")), R_fill=2, T_fill=2, timechunks=8)
    _check(*trk.run(return_merges=True), exp, attrs, mds, tv, lat, lon)


def test_partition_and_relabel_kernels_match_oracle():
    hot = marex_amd.detect.get_engine(0)
    rng = np.random.default_rng(7)
    ny, nx = 50, 300
    for wrap in (True, False):
        for trial in range(6):
            child = np.zeros((ny, nx), np.int32)
            prev = np.zeros((ny, nx), np.int32)
            yy, xx = np.mgrid[0:ny, 0:nx]
            kids, offs, pars, labs, pcs, maxds = [], [0], [], [], [], []
            nid = 100
            for c, cy in enumerate((12, 37)):
                cx = rng.uniform(0, nx)
                dx = np.minimum(np.abs(xx - cx), nx - np.abs(xx - cx)) if wrap else np.abs(xx - cx)
                m = ((yy - cy) ** 2 + dx ** 2 <= rng.uniform(5, 11) ** 2) & (child == 0)
                child[m] = 10 + c
                kids.append(10 + c)
                k = int(rng.integers(2, 5))
                ps = []
                for p in range(k):
                    py, px = cy + rng.uniform(-8, 8), (cx + rng.uniform(-20, 20)) % nx
                    pdx = np.minimum(np.abs(xx - px), nx - np.abs(xx - px)) if wrap else np.abs(xx - px)
                    pm = ((yy - py) ** 2 + pdx ** 2 <= rng.uniform(2, 6) ** 2) & (prev == 0)
                    if not pm.any():
                        free = np.argwhere(prev == 0)[0]
                        pm = (yy == free[0]) & (xx == free[1])
                    prev[pm] = 20 + 5 * c + p
                    ps.append(20 + 5 * c + p)
                    pcs.append((float(np.mean(np.nonzero(pm)[0])), float(np.mean(np.nonzero(pm)[1]))))
                pars += ps
                labs += [10 + c] + list(range(nid, nid + k - 1))
                nid += k - 1
                offs.append(len(pars))
                maxds += [int(rng.choice([3, 8, 40]))] * k
            pcs = np.array(pcs)
            exp = child.copy()
            for c, kid in enumerate(kids):
                ys, xs = np.nonzero(child == kid)
                sl = slice(offs[c], offs[c + 1])
                a = mo.partition_centroid(ys, xs, pcs[sl], nx, wrap)
                exp[ys, xs] = np.array(labs[sl])[a]
            cur = torch.from_numpy(child.reshape(-1).copy()).to(hot.device)
            hot.partition_centroid(cur, ny, nx, kids, offs, pcs[:, 0], pcs[:, 1], labs, wrap)
            assert np.array_equal(cur.cpu().numpy().reshape(ny, nx), exp), ("centroid", wrap, trial)
            exp = child.copy()
            for c, kid in enumerate(kids):
                ys, xs = np.nonzero(child == kid)
                sl = slice(offs[c], offs[c + 1])
                cells = [np.nonzero(prev == p) for p in pars[sl]]
                a = mo.partition_nn(ys, xs, cells, pcs[sl], ny, nx, maxds[offs[c]], wrap)
                exp[ys, xs] = np.array(labs[sl])[a]
            cur = torch.from_numpy(child.reshape(-1).copy()).to(hot.device)
            pv = torch.from_numpy(prev.reshape(-1).copy()).to(hot.device)
            hot.partition_nn(cur, pv, ny, nx, kids, offs, pars, pcs[:, 0], pcs[:, 1], labs, maxds, wrap)
            assert np.array_equal(cur.cpu().numpy().reshape(ny, nx), exp), ("nn", wrap, trial)
    # a centroid tie: the first parent wins
    child = np.zeros((5, 11), np.int32)
    child[2, 5] = 7
    cur = torch.from_numpy(child.reshape(-1).copy()).to(hot.device)
    hot.partition_centroid(cur, 5, 11, [7], [0, 2], [2.0, 2.0], [3.0, 7.0], [7, 8], True)
    assert cur.cpu().numpy().reshape(5, 11)[2, 5] == 7
    # square roots are compared, not squares: 4 + 2^-50 and 4 both give 2.0, so the first parent wins
    child = np.zeros((5, 11), np.int32)
    child[0, 0] = 7
    cur = torch.from_numpy(child.reshape(-1).copy()).to(hot.device)
    hot.partition_centroid(cur, 5, 11, [7], [0, 2], [-2.0 ** -25, 0.0], [2.0, 2.0], [7, 8], False)
    assert cur.cpu().numpy().reshape(5, 11)[0, 0] == 7
    # relabel: sorted table and dense table
    x = rng.integers(0, 50, 10000).astype(np.int32)
    keys = np.array([3, 7, 19, 44], np.int32)
    vals = np.array([1, 2, 3, 4], np.int32)
    d = torch.from_numpy(x.copy()).to(hot.device)
    hot.relabel(d, vals, keys)
    exp = x.copy()
    for k, v in zip(keys, vals):
        exp[x == k] = v
    assert np.array_equal(d.cpu().numpy(), exp)
    lut = rng.integers(1, 9, 50).astype(np.int32)
    d = torch.from_numpy(x.copy()).to(hot.device)
    hot.relabel(d, lut)
    assert np.array_equal(d.cpu().numpy(), np.where(x > 0, lut[x], 0))


def test_public_stage_methods_and_the_iteration_cap():
    """split_and_merge_objects / cluster_rename_objects_and_props / consolidate_object_ids against the oracle on a grid
    narrower than the seam bands (every merge repeats until the cap of 10 iterations) and on a split that consolidation
    rejoins."""
    T, ny, nx = 3, 12, 40
    ids = np.zeros((T, ny, nx), np.int32)
    ids[0, 5:8, 10:13] = 1
    ids[0, 5:8, 20:23] = 2
    ids[1, 5:8, 10:23] = 3
    ids[2, 5:8, 10:14] = 4
    ids[2, 5:8, 19:23] = 5
    tv = np.arange(T).astype("datetime64[D]").astype("datetime64[ns]")
    lat = np.linspace(-10, 10, ny).astype(np.float32)
    lon = np.linspace(0, 351, nx).astype(np.float32)
    ev = _da(ids > 0, tv, lat, lon)
    trk = marex_amd.tracker(ev, DataArray(np.ones((ny, nx), bool), dims=("lat", "lon")), R_fill=1, timechunks=3,
                            coordinate_units="degrees")
    fld = DataArray(ids, dims=("time", "lat", "lon"), coords={"time": ("time", tv)})
    props = trk.calculate_object_properties(fld, properties=["area", "centroid"])
    out, p2, ov, merges = trk.split_and_merge_objects(fld, props)
    e_ids, e_props, e_ov, e_m = mo.split_and_merge(ids, [3], tv)
    assert np.array_equal(out.values, e_ids) and np.array_equal(ov, e_ov)
    assert np.array_equal(p2["ID"].values, np.array(sorted(e_props)))
    assert np.array_equal(p2["area"].values, np.array([e_props[k][0] for k in sorted(e_props)]))
    e_mds = mo.merges_dataset(e_m, tv.dtype)
    assert len(e_mds["n_parents"]) == 10
    for k in e_mds:
        assert np.array_equal(np.asarray(merges[k].values), e_mds[k]), k
    ds = trk.cluster_rename_objects_and_props(out, p2, ov, merges)
    exp = mo.cluster_rename(e_ids, e_ov, e_mds, tv, lat, lon, np.ones((ny, nx), np.float32))
    for k in ("ID_field", "global_ID", "area", "presence", "merge_ledger"):
        assert np.array_equal(np.asarray(ds[k].values), exp[k], equal_nan=k == "area"), k
    a = np.zeros((ny, nx), np.int32)
    a[5:8, 10:31] = 1
    b = np.zeros((ny, nx), np.int32)
    b[5:8, 10:16], b[5:8, 25:31] = 2, 3
    pr = {1: [63.0, 6.0, 20.0], 2: [18.0, 6.0, 12.5], 3: [18.0, 6.0, 27.5]}
    from marex_amd.xr_compat import Dataset
    pds = Dataset({"area": DataArray(np.array([v[0] for v in pr.values()]), dims=("ID",), coords={"ID": ("ID", np.array([1, 2, 3]))}),
                   "centroid": DataArray(np.array([[v[1] for v in pr.values()], [v[2] for v in pr.values()]]),
                                         dims=("component", "ID"), coords={"ID": ("ID", np.array([1, 2, 3]))})})
    got, gp = trk.consolidate_object_ids(DataArray(a, dims=("lat", "lon")), DataArray(b, dims=("lat", "lon")), pds, 1)
    exp_b = mo.consolidate(a, b, pr, 0.5, False)
    assert np.array_equal(got.values, exp_b) and list(gp["ID"].values) == sorted(pr)
    assert gp["area"].values.tolist() == [pr[k][0] for k in sorted(pr)]


@pytest.mark.parametrize("nn", [False, True])
def test_merge_resolved_on_the_second_iteration(nn):
    """The hand case of tests/test_merge_track_host.py whose merge needs a second iteration, through the public
    split_and_merge_objects and cluster_rename_objects_and_props, against the oracle."""
    from test_merge_track_host import second_iteration_case

    ids = second_iteration_case()
    T, ny, nx = ids.shape
    tv = np.arange(T).astype("datetime64[D]").astype("datetime64[ns]")
    lat = np.linspace(-19, 19, ny).astype(np.float32)
    lon = (np.arange(nx) * 1.5 + 0.75).astype(np.float32)
    trk = marex_amd.tracker(_da(ids > 0, tv, lat, lon), DataArray(np.ones((ny, nx), bool), dims=("lat", "lon")), R_fill=1,
                            timechunks=2, nn_partitioning=nn, coordinate_units="degrees")
    fld = DataArray(ids, dims=("time", "lat", "lon"), coords={"time": ("time", tv)})
    props = trk.calculate_object_properties(fld, properties=["area", "centroid"])
    out, p2, ov, merges = trk.split_and_merge_objects(fld, props)
    e_ids, e_props, e_ov, e_m = mo.split_and_merge(ids, [2], tv, 0.5, nn)
    e_mds = mo.merges_dataset(e_m, tv.dtype)
    assert len(e_mds["n_parents"]) == 2 and e_mds["child_IDs"][1, 0] == e_mds["child_IDs"][0, 0]  # 2nd pass, same child
    assert np.array_equal(out.values, e_ids) and np.array_equal(ov, e_ov)
    assert np.array_equal(p2["ID"].values, np.array(sorted(e_props)))
    c = np.asarray(p2["centroid"].values)
    assert np.array_equal(c, np.array([[e_props[k][1] for k in sorted(e_props)], [e_props[k][2] for k in sorted(e_props)]]))
    for k in e_mds:
        assert np.array_equal(np.asarray(merges[k].values), e_mds[k]), k
    ds = trk.cluster_rename_objects_and_props(out, p2, ov, merges)
    exp = mo.cluster_rename(e_ids, e_ov, e_mds, tv, lat, lon, np.ones((ny, nx), np.float32))
    for k in ("ID_field", "global_ID", "area", "centroid", "presence", "merge_ledger"):
        assert np.array_equal(np.asarray(ds[k].values), exp[k], equal_nan=k in ("area", "centroid")), k
