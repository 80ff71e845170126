"""GPU parity: the split-and-merge stage of the tracker on unstructured meshes (split_and_merge_objects_parallel,
marEx/track.py:3804-4814, 5246-5419) against the NumPy oracle of tests/mesh_merge_oracle.py -- the two partition engine
methods on ring-with-chords meshes and hand-built paths, the whole stage on the reference's merging fixture and on seeded
synthetic scenarios; IDs, properties, pair lists and merge events bit for bit."""
import os
import sys

import numpy as np
import pytest
import torch

from marex_amd.engine import HotPath
from marex_amd.xr_compat import DataArray
from marex_amd.zarr_io import DeviceDataArray

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import mesh_merge_oracle as mm  # noqa: E402
import mesh_objects_oracle as mo  # noqa: E402
from mesh_merge_scenarios import drifting_runs, ring_mesh  # noqa: E402
from test_mesh_merge_host import (CONFIGS, MERGES, THRESHOLD, assert_stage_equals_oracle, fixture_oracle,  # noqa: E402
                                  load_merging_fixture, props_dataset)
from test_mesh_tracker_host import mesh_tracker  # noqa: E402

pytestmark = pytest.mark.gpu

CHILD, OTHER = 7, 8


def _dev(hot, a):
    return torch.from_numpy(np.array(a, order="C")).to(hot.device)  # np.array copies: the input stays as it is


def _partition_case(seed, C, k):
    """A mesh of C cells, k parents as runs of the previous slice, a child run with holes over and beyond them."""
    rng = np.random.default_rng(seed)
    mesh = ring_mesh(rng, C)
    seg = C // (k + 1)
    prev, cur = np.zeros(C, np.int32), np.zeros(C, np.int32)
    parents = [20 + j for j in range(k)]
    for j, p in enumerate(parents):
        prev[j * seg + 1:j * seg + 1 + max(1, seg // 2)] = p
    prev[k * seg + 1:k * seg + 3] = 99  # an object of the previous slice that is no parent
    cur[:k * seg + seg // 2] = CHILD
    holes = rng.random(C) < 0.15
    cur[holes & (cur == CHILD)] = np.where(rng.random(int((holes & (cur == CHILD)).sum())) < 0.5, 0, OTHER)
    mid = [j * seg + 1 + max(1, seg // 2) // 2 for j in range(k)]  # centroids: the middle cell of every parent run
    cen = np.stack([mesh["lat"][mid], mesh["lon"][mid]], axis=1).astype(np.float32)
    return mesh, prev, cur, parents, cen


def _run_nn(hot, mesh, prev, cur, parents, cen, labels, max_hops, hops_per_read=None):
    u, pv = mm.unit_vectors(mesh["lat"], mesh["lon"]), mm.unit_vectors(cen[:, 0], cen[:, 1])
    owner0 = np.full(cur.size, 255, np.uint8)
    for j, p in enumerate(parents):
        owner0[prev == p] = j
    child = cur == CHILD
    owner, info = mm.partition_nn(child, owner0, mesh["nb0"], max_hops, u, pv)
    exp = cur.copy()
    exp[child] = np.asarray(labels, np.int32)[owner[child]]
    d = _dev(hot, cur)
    r = hot.mesh_partition_nn(d, _dev(hot, prev), _dev(hot, mesh["nb0"]), CHILD, parents, pv, labels, max_hops, _dev(hot, u),
                              hops_per_read=hops_per_read)
    got = d.cpu().numpy()
    assert np.array_equal(got, exp), np.argwhere(got != exp)[:8].ravel()
    assert (r["hops"], r["leftover"]) == (info["hops"], info["leftover"]), (r, info)
    return r, info


@pytest.mark.parametrize("k", [2, 3, 10])
@pytest.mark.parametrize("C", [63, 64, 65, 405, 5000])
def test_partition_methods_equal_the_oracle(hot, C, k):
    mesh, prev, cur, parents, cen = _partition_case(1000 * k + C, C, k)
    labels = [CHILD] + list(range(500, 500 + k - 1))
    r, info = _run_nn(hot, mesh, prev, cur, parents, cen, labels, 40)
    assert info["hops"] >= 1
    r1, _ = _run_nn(hot, mesh, prev, cur, parents, cen, labels, 40, hops_per_read=1)  # the control block read after every hop
    assert (r1["hops"], r1["leftover"], r1["reason"]) == (r["hops"], r["leftover"], r["reason"]) and r1["reads"] >= r["reads"]

    # centroid partition: two children in one launch, the second with its own parents
    u = mm.unit_vectors(mesh["lat"], mesh["lon"])
    pv = mm.unit_vectors(cen[:, 0], cen[:, 1])
    keys, off = [CHILD, OTHER], [0, k, k + 2]
    pv_all = np.concatenate([pv, pv[:, ::-1][:, :2]], axis=1)
    lab_all = labels + [OTHER, 900]
    exp = cur.copy()
    for j, key in enumerate(keys):
        m = cur == key
        exp[m] = np.asarray(lab_all[off[j]:off[j + 1]], np.int32)[mm.nearest_centroid(u[:, m], pv_all[:, off[j]:off[j + 1]])]
    d = _dev(hot, cur)
    hot.mesh_partition_centroid(d, keys, off, pv_all, lab_all, _dev(hot, u))
    assert np.array_equal(d.cpu().numpy(), exp)
    assert len(np.unique(exp[cur == CHILD])) >= 2  # the child was split


def _line_mesh(C, both_ways):
    rng = np.random.default_rng(5)
    mesh = ring_mesh(rng, C, chords=False)
    if not both_ways:
        mesh["nb0"][0] = -1  # every cell lists the cell before it only
    return mesh


def test_a_cell_reachable_only_against_its_listing_falls_back_to_the_centroid(hot):
    mesh = _line_mesh(16, both_ways=False)
    mesh["nb0"][1][6] = -1  # cell 6 lists nobody: the frontier that comes down from cell 8 ends there
    prev, cur = np.zeros(16, np.int32), np.zeros(16, np.int32)
    prev[0:2], prev[8:10] = 20, 21
    cur[2:8] = CHILD
    cen = np.array([[mesh["lat"][1], mesh["lon"][1]], [mesh["lat"][9], mesh["lon"][9]]], np.float32)
    r, info = _run_nn(hot, mesh, prev, cur, [20, 21], cen, [CHILD, 500], 40)
    assert info["leftover"] == 4 and info["early_stop"] and info["hops"] == 3 and not info["capped"]
    assert r["reason"] == 2


def test_max_hops_cuts_a_long_child(hot):
    mesh = _line_mesh(64, both_ways=True)
    prev, cur = np.zeros(64, np.int32), np.zeros(64, np.int32)
    prev[0:2], prev[40:42] = 20, 21
    cur[2:40] = CHILD
    cen = np.array([[mesh["lat"][0], mesh["lon"][0]], [mesh["lat"][41], mesh["lon"][41]]], np.float32)
    r, info = _run_nn(hot, mesh, prev, cur, [20, 21], cen, [CHILD, 500], 2)
    assert info["capped"] and info["hops"] == 2 and info["leftover"] == 38 - 4
    assert r["reason"] == 3
    r, info = _run_nn(hot, mesh, prev, cur, [20, 21], cen, [CHILD, 500], 40)  # uncut: the frontiers meet
    assert info["leftover"] == 0 and info["hops"] == 19 and r["reason"] == 1


def test_a_hop_that_claims_only_other_cells_stops_the_search(hot):
    mesh = _line_mesh(64, both_ways=True)
    prev, cur = np.zeros(64, np.int32), np.zeros(64, np.int32)
    prev[0:2], prev[30:32] = 20, 21
    cur[10:13] = CHILD
    cen = np.array([[mesh["lat"][0], mesh["lon"][0]], [mesh["lat"][31], mesh["lon"][31]]], np.float32)
    r, info = _run_nn(hot, mesh, prev, cur, [20, 21], cen, [CHILD, 500], 40)
    assert info["nonchild_only_hop"] and info["hops"] == 1 and info["leftover"] == 3
    assert r["reason"] == 2


# ------------------------------------------------------------------ the whole stage
def _fixture_tracker(nn, chunk):
    f = load_merging_fixture()
    return mesh_tracker(f["pre"], f["mask"], f["nb"], f["areas"], f["lat"], f["lon"], tm=f["time"], R_fill=1, T_fill=2,
                        area_filter_quartile=None, area_filter_absolute=5, overlap_threshold=THRESHOLD, nn_partitioning=nn,
                        timechunks=chunk)


@pytest.mark.parametrize("nn,chunk", list(CONFIGS), ids=[f"{'nn' if n else 'centroid'}-{c}" for n, c in CONFIGS])
def test_stage_on_the_reference_fixture_equals_the_oracle(hot, nn, chunk):
    f = load_merging_fixture()
    trk = _fixture_tracker(nn, chunk)
    got = trk.split_and_merge_objects_parallel(DataArray(f["ids"], dims=("time", "ncells")), props_dataset(f["ids"], f["q"], f["e"]))
    exp = fixture_oracle(nn, chunk)
    assert_stage_equals_oracle(got, exp, f["time"], (nn, chunk))
    st = trk._merge_stats
    assert st["iterations"] == CONFIGS[(nn, chunk)] and st["partitions"] == MERGES
    if nn:
        assert st["hops"] == sum(i["hops"] for i in exp["nn"])


_scen = {}


def _scenario(C, seed, nn):
    key = (C, seed, nn)
    if key not in _scen:
        mesh, ids = drifting_runs(seed, C)
        e, q = mo.weight_tables(mesh["areas"], mesh["lat"], mesh["lon"])
        _scen[key] = (mesh, ids, e, q, mm.split_and_merge(ids, q, e, mesh["nb0"], mesh["areas"], mesh["lat"], mesh["lon"], 0.3,
                                                          [3, 3, 2], nn))
    return _scen[key]


def _scenario_tracker(mesh, ids, nn):
    return mesh_tracker(ids > 0, mesh["mask"], mesh["nb0"] + 1, mesh["areas"], mesh["lat"], mesh["lon"], overlap_threshold=0.3,
                        nn_partitioning=nn, timechunks=3)


@pytest.mark.parametrize("nn", [True, False])
@pytest.mark.parametrize("C,seed", [(200, 1), (4097, 7)])
def test_stage_on_drifting_runs_equals_the_oracle(hot, C, seed, nn):
    mesh, ids, e, q, exp = _scenario(C, seed, nn)
    if nn:  # what the scenario is there for
        assert max(len(m[3]) for m in exp["merges"]) >= 3 and exp["iterations"] >= 2
        assert len({min(m[1] // 3, 2) for m in exp["merges"]}) >= 2
    trk = _scenario_tracker(mesh, ids, nn)
    got = trk.split_and_merge_objects_parallel(DataArray(ids, dims=("time", "ncells")), props_dataset(ids, q, e))
    assert_stage_equals_oracle(got, exp, np.arange(8), (C, seed, nn))


def test_device_resident_field_repeat_and_control_block_reads(hot, monkeypatch):
    mesh, ids, e, q, exp = _scenario(200, 1, True)
    trk = _scenario_tracker(mesh, ids, True)
    props = props_dataset(ids, q, e)
    dev_field = DeviceDataArray(_dev(hot, ids), ("time", "ncells"), {"time": np.arange(8)}, name="ID_field")
    a = trk.split_and_merge_objects_parallel(dev_field, props)
    assert np.array_equal(dev_field.device_tensor.cpu().numpy(), ids)  # the input is not written
    assert_stage_equals_oracle(a, exp, np.arange(8), "device-resident field")
    reads = trk._merge_stats["reads"]
    b = trk.split_and_merge_objects_parallel(DataArray(ids, dims=("time", "ncells")), props)
    assert_stage_equals_oracle(b, exp, np.arange(8), "second run")
    monkeypatch.setattr(HotPath, "MESH_NN_HOPS_PER_READ", 1)
    c = trk.split_and_merge_objects_parallel(DataArray(ids, dims=("time", "ncells")), props)
    assert_stage_equals_oracle(c, exp, np.arange(8), "control block read after every hop")
    assert trk._merge_stats["reads"] > reads and trk._merge_stats["hops"] == sum(i["hops"] for i in exp["nn"])
