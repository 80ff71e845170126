"""GPU parity: cluster renaming and the end-to-end ``run()`` of the tracker on unstructured meshes (marEx/track.py:1162-1232,
2734-3331) -- the rename-and-accumulate kernel through ``HotPath.mesh_event_rename`` against NumPy, the stage on seeded
scenarios and ``run()`` on the reference's two mesh fixtures against the oracle chain (tests/mesh_objects_oracle.py ->
tests/mesh_merge_oracle.py -> tests/mesh_events_oracle.py), every variable bit for bit."""
import os
import sys

import numpy as np
import pytest
import torch

import marex_amd
from marex_amd.exceptions import ProcessingError
from marex_amd.xr_compat import DataArray
from marex_amd.zarr_io import DeviceDataArray

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import mesh_events_oracle as me  # noqa: E402
import mesh_merge_oracle as mm  # noqa: E402
import mesh_objects_oracle as mo  # noqa: E402
from mesh_merge_scenarios import drifting_runs, ring_mesh  # noqa: E402
from test_mesh_events_host import (assert_events_equal, assert_merges_equal, fixture_events, merges_dataset, same,  # noqa: E402
                                   second_fixture, second_fixture_chain)
from test_mesh_merge_host import EVENTS, MERGES, THRESHOLD, fixture_oracle, load_merging_fixture  # noqa: E402
from test_mesh_tracker_host import mesh_tracker  # noqa: E402

pytestmark = pytest.mark.gpu


def _dev(hot, a):
    return torch.from_numpy(np.array(a, order="C")).to(hot.device)  # np.array copies: the input stays as it is


# ------------------------------------------------------------------ the kernel
N_EV = 6
#: IDs 0..40 -> events: several IDs to one event, some to 0, event 5 without an ID, the table shorter than the largest ID
LUT = np.zeros(33, np.int32)
LUT[[1, 2, 9, 17]], LUT[[3, 4]], LUT[[5, 30, 31, 32]], LUT[[6, 8, 10, 12, 14]], LUT[[20, 21]] = 1, 2, 3, 4, 6


def _kernel_case(T, C):
    rng = np.random.default_rng(100 * T + C)
    mesh = ring_mesh(rng, C)
    e, q = mo.weight_tables(mesh["areas"], mesh["lat"], mesh["lon"])
    ids = rng.integers(0, 41, (T, C)).astype(np.int32)
    runs = rng.integers(0, 41, (T, (C + 99) // 100)).astype(np.int32)   # runs of up to 100 cells: the carried event
    long = np.repeat(runs, 100, axis=1)[:, :C]
    ids = np.where(rng.random((T, C)) < 0.6, long, ids)
    ids[rng.random((T, C)) < 0.05] = -3
    ids[0, 0] = 9
    if C > 1:  # every event with an ID has a cell, and so have an ID past the table, one mapped to 0 and a negative value
        ids[0, 1:11] = [3, 5, 6, 20, 40, 7, -3, 2, 4, 21]
    return ids, e, q


@pytest.mark.parametrize("T", [1, 5])
@pytest.mark.parametrize("C", [1, 63, 1025, 4097])
def test_rename_kernel_equals_numpy(hot, T, C):
    ids, e, q = _kernel_case(T, C)
    assert ids.max() >= LUT.size or C == 1
    new, sums, gid = me.rename_and_sums(ids, LUT, N_EV, q)
    if C > 1:
        assert (sums[:, 4, 0] == 0).all() and (sums[..., 0].sum(axis=0)[[0, 1, 2, 3, 5]] > 0).all() and (ids < 0).any()
    qd = _dev(hot, q)
    outs = []
    for _ in range(2):  # a second call on the same input: the same bytes
        d = _dev(hot, ids)
        r = hot.mesh_event_rename(d, LUT, N_EV, qd, e)
        got = d.cpu().numpy()
        assert same(got, new), np.argwhere(got != new)[:8].ravel()
        assert r["mom"].dtype == np.int64 and same(r["mom"], sums), np.argwhere(r["mom"] != sums)[:8].ravel()
        assert r["gid"].dtype == np.int32 and same(r["gid"], gid)
        outs.append((got.tobytes(), r["mom"].tobytes(), r["gid"].tobytes()))
    assert outs[0] == outs[1]
    one = (LUT > 0).astype(np.int32)  # n_ev = 1
    new1, sums1, gid1 = me.rename_and_sums(ids, one, 1, q)
    d = _dev(hot, ids)
    r = hot.mesh_event_rename(d, one, 1, qd, e)
    assert same(d.cpu().numpy(), new1) and same(r["mom"], sums1) and same(r["gid"], gid1)


def test_rename_checks_its_arguments_before_the_launch(hot):
    ids, e, q = _kernel_case(2, 63)
    d, qd = _dev(hot, ids), _dev(hot, q)
    for bad in (lambda: hot.mesh_event_rename(d, LUT, 5, qd, e),                       # the table names event 6
                lambda: hot.mesh_event_rename(d, LUT.astype(np.int64), N_EV, qd, e),
                lambda: hot.mesh_event_rename(d, LUT, N_EV, qd[:3].contiguous(), e),
                lambda: hot.mesh_event_rename(d.to(torch.int64), LUT, N_EV, qd, e),
                lambda: hot.mesh_event_rename(d, LUT[:0], N_EV, qd, e)):
        with pytest.raises(ProcessingError):
            bad()
    assert np.array_equal(d.cpu().numpy(), ids)  # nothing was written
    lut_d, acc, gid = _dev(hot, LUT), torch.zeros((2 * N_EV, 5), dtype=torch.int64, device=hot.device), \
        torch.zeros(2 * N_EV, dtype=torch.int32, device=hot.device)
    for code, args in ((-4, (d, 2, 2 ** 31 - 1, lut_d, LUT.size, N_EV, qd, acc, gid)),
                       (-4, (d, 2 ** 31 - 1, 63, lut_d, LUT.size, N_EV, qd, acc, gid)),
                       (-1, (d, 0, 63, lut_d, LUT.size, N_EV, qd, acc, gid)), (-1, (d, 2, 63, None, LUT.size, N_EV, qd, acc, gid)),
                       (-1, (d, 2, 63, lut_d, LUT.size, 0, qd, acc, gid))):  # refused by the library before any launch
        with pytest.raises(ProcessingError, match=rf"marex_mesh_event_rename_i64 failed \(code {code}\)"):
            hot.call("marex_mesh_event_rename_i64", *args)
    assert np.array_equal(d.cpu().numpy(), ids)


# ------------------------------------------------------------------ the stage
_scen = {}


def _scenario(C, seed, nn):
    key = (C, seed, nn)
    if key not in _scen:
        mesh, ids = drifting_runs(seed, C)
        e, q = mo.weight_tables(mesh["areas"], mesh["lat"], mesh["lon"])
        r = mm.split_and_merge(ids, q, e, mesh["nb0"], mesh["areas"], mesh["lat"], mesh["lon"], 0.3, [3, 3, 2], nn)
        _scen[key] = (mesh, ids, r, me.cluster_rename(r["field"], r["pairs"], r["events"], q, e, np.arange(8)))
    return _scen[key]


@pytest.mark.parametrize("nn", [True, False], ids=["nn", "centroid"])
@pytest.mark.parametrize("C,seed", [(200, 1), (4097, 7)])
def test_stage_on_drifting_runs_equals_the_oracle(hot, C, seed, nn):
    mesh, ids, r, exp = _scenario(C, seed, nn)
    trk = mesh_tracker(ids > 0, mesh["mask"], mesh["nb0"] + 1, mesh["areas"], mesh["lat"], mesh["lon"], overlap_threshold=0.3,
                       nn_partitioning=nn, timechunks=3)
    field = r["field"].copy()
    ds = trk.cluster_rename_objects_and_props(DataArray(field, dims=("time", "ncells")), None, r["pairs"],
                                              merges_dataset(r["events"], np.arange(8)))
    assert np.array_equal(field, r["field"])  # the input is not written
    assert_events_equal(ds, exp, (C, seed, nn))


# ------------------------------------------------------------------ run() on the reference's fixtures
def _remapped(cen, lon):
    """The centroids in the input's longitude range (degrees in, degrees out: _remap_coordinates, track.py:978-1021)."""
    out = np.array(cen, dtype=np.float32)
    if float(np.min(lon)) >= 0 and float(np.max(lon)) > 180:
        out[1] = np.where(out[1] < 0, out[1] + 360, out[1])
    return out


def _check_structure(ds, N):
    """The structural checks of the reference's tests/test_unstructured_tracking.py:197-260."""
    for k in ("ID_field", "global_ID", "area", "centroid", "presence", "time_start", "time_end", "merge_ledger"):
        assert k in ds.data_vars, k
    assert tuple(ds["ID_field"].dims) == ("time", "ncells") and np.issubdtype(np.asarray(ds["ID_field"].values).dtype, np.integer)
    assert ds.sizes["ID"] == ds.attrs["N_events_final"] == N
    pres, gid = np.asarray(ds["presence"].values), np.asarray(ds["global_ID"].values)
    assert np.array_equal(pres, gid != 0)
    assert (np.asarray(ds["area"].values)[pres] > 0).all()
    ts, te = np.asarray(ds["time_start"].values), np.asarray(ds["time_end"].values)
    assert (ts[pres.any(axis=0)] <= te[pres.any(axis=0)]).all()
    c = ds["ID_field"].coords
    assert tuple(c["lat"].dims) == ("ncells",) and tuple(c["lon"].dims) == ("ncells",)


def _run_fixture_tracker(f, data, chunk, **kw):
    args = dict(R_fill=1, area_filter_quartile=None, area_filter_absolute=5, T_fill=2, overlap_threshold=THRESHOLD,
                nn_partitioning=True, unstructured_grid=True, dimensions={"x": "ncells"}, coordinates={"x": "lon", "y": "lat"},
                coordinate_units="degrees", neighbours=DataArray(f["nb"], dims=("nv", "ncells")),
                cell_areas=DataArray(f["areas"], dims=("ncells",)), timechunks=chunk)
    args.update(kw)
    return marex_amd.tracker(data, DataArray(f["mask"], dims=("ncells",)), **args)


def _check_merging_run(f, ds, chunk):
    exp = dict(fixture_events(True, chunk))
    exp["centroid"] = _remapped(exp["centroid"], f["lon"])
    assert_events_equal(ds, exp, ("run", chunk))
    _check_structure(ds, EVENTS)
    assert np.array_equal(np.asarray(ds["ID_field"].coords["lat"].values), f["lat"])
    at = ds.attrs
    assert (at["N_objects_prefiltered"], at["N_objects_filtered"], at["N_events_final"]) == (98, 98, 11)
    assert at["T_fill"] == 2 and at["R_fill"] == 1
    return at


def _host_mask(f):
    return DataArray(f["ev"], dims=("time", "ncells"),
                     coords={"time": ("time", f["time"]), "lat": ("ncells", f["lat"]), "lon": ("ncells", f["lon"])})


@pytest.mark.parametrize("chunk", [100, 5])
def test_run_on_the_merging_fixture_equals_the_oracle_chain(hot, chunk):
    f = load_merging_fixture()
    trk = _run_fixture_tracker(f, _host_mask(f), chunk)
    ds, merges = trk.run(return_merges=True)
    at = _check_merging_run(f, ds, chunk)
    assert_merges_equal(merges, fixture_oracle(True, chunk)["events"], f["time"], ("run", chunk))
    assert at["allow_merging"] == 1 and at["total_merges"] == MERGES == 9 and at["nn_partitioning"] == 1
    assert at["overlap_threshold"] == THRESHOLD and "multi_parent_merges" in at
    assert set(trk._stage_times) == {"objects", "split_and_merge", "cluster_rename"}


def test_run_with_a_device_resident_mask_and_without_merge_attrs(hot):
    f = load_merging_fixture()
    coords = {"time": f["time"], "lat": DataArray(f["lat"], dims=("ncells",)), "lon": DataArray(f["lon"], dims=("ncells",))}
    xd = torch.from_numpy(f["ev"]).to(hot.device)
    ds, merges = _run_fixture_tracker(f, DeviceDataArray(xd, ("time", "ncells"), coords), 5).run(return_merges=True)
    at = _check_merging_run(f, ds, 5)
    assert at["total_merges"] == 9 and torch.equal(xd.cpu(), torch.from_numpy(f["ev"]))  # the input is not written
    assert_merges_equal(merges, fixture_oracle(True, 5)["events"], f["time"], "device resident")
    out = _run_fixture_tracker(f, _host_mask(f), 5, allow_merging=False).run(return_merges=True)
    assert not isinstance(out, tuple)  # a single return value: the events, tracked through track_objects all the same
    at = _check_merging_run(f, out, 5)
    assert at["allow_merging"] == 0 and not {"total_merges", "multi_parent_merges", "overlap_threshold", "nn_partitioning"} & set(at)


def test_run_on_the_second_fixture_gives_three_events_inside_the_mesh(hot):
    f = second_fixture()
    r, exp = second_fixture_chain(False, 5)
    exp = dict(exp, centroid=_remapped(exp["centroid"], f["lon"]))
    trk = mesh_tracker(f["ev"], f["mask"], f["nb"], f["areas"], f["lat"], f["lon"], tm=f["time"], R_fill=3, T_fill=2,
                       area_filter_quartile=0.5, timechunks=5)
    ds = trk.run()
    assert_events_equal(ds, exp, "second fixture")
    _check_structure(ds, 3)
    assert ds.attrs["total_merges"] == 0 and ds.attrs["allow_merging"] == 1
    st = f["stats"]
    assert (ds.attrs["N_objects_prefiltered"], ds.attrs["N_objects_filtered"]) == (st[1], st[2])
    pres, cen = np.asarray(ds["presence"].values), np.asarray(ds["centroid"].values)
    lat_c, lon_c = cen[0][pres], cen[1][pres]
    assert not np.isnan(lat_c).any() and not np.isnan(lon_c).any()
    assert (lat_c >= f["lat"].min()).all() and (lat_c <= f["lat"].max()).all()      # reference test 326-343
    assert (lon_c >= f["lon"].min()).all() and (lon_c <= f["lon"].max()).all()
    led = np.asarray(ds["merge_ledger"].values)
    assert led.shape[2] == 1 and (led == -1).all()
