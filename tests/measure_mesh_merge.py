"""One-off measurement (not a pytest file): ``tracker.split_and_merge_objects_parallel`` on the device against the NumPy
oracle of tests/mesh_merge_oracle.py on the same input, on the host cores of the same box -- the parent commit has no such
stage to compare with.  Inputs: the reference's merging fixture (405 cells x 100 steps) and drifting runs on ring meshes
(tests/mesh_merge_scenarios.py) of ``MERGE_CELLS`` cells (default 200 000) x 8 steps, chunks of 3, nearest-neighbour and
centroid partition.

Per input and partition: the stage's wall time (host clock, ends in a synchronise; median of REPS after one warm-up), the
oracle's time (one run), the equality of the two ID fields, and from the stage's own counters: iterations, steps with
pending children, partitions, hops and launches per child, reads of the control block, and the share of the wall time
spent in the partition calls against the reused overlap / moment calls."""
import json
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import numpy as np
import torch

import mesh_merge_oracle as mm
import mesh_objects_oracle as mo
from mesh_merge_scenarios import drifting_runs
from test_mesh_merge_host import THRESHOLD, load_merging_fixture, props_dataset
from test_mesh_tracker_host import mesh_tracker

from marex_amd.xr_compat import DataArray

REPS = 5
CELLS = int(os.environ.get("MERGE_CELLS", 200_000))


def measure(name, trk, ids, q, e, oracle):
    props = props_dataset(ids, q, e)
    field = DataArray(ids, dims=("time", "ncells"))
    eng = trk._engine()
    trk.split_and_merge_objects_parallel(field, props)  # warm-up: tables uploaded, allocator warm
    ms = []
    for _ in range(REPS):
        eng.sync()
        t0 = time.perf_counter()
        got = trk.split_and_merge_objects_parallel(field, props)
        eng.sync()
        ms.append((time.perf_counter() - t0) * 1e3)
    st = dict(trk._merge_stats)
    t0 = time.perf_counter()
    exp = oracle()
    oracle_ms = (time.perf_counter() - t0) * 1e3
    med = statistics.median(ms)
    n = max(st["partitions"], 1)
    print(json.dumps({
        "input": name, "T": int(ids.shape[0]), "C": int(ids.shape[1]), "nn_partitioning": bool(trk.nn_partitioning),
        "stage_ms_median": round(med, 2), "stage_ms_min": round(min(ms), 2), "stage_ms_max": round(max(ms), 2),
        "oracle_ms": round(oracle_ms, 1), "oracle_over_stage": round(oracle_ms / med, 2),
        "equal_to_oracle": bool(np.array_equal(np.asarray(got[0].values), exp["field"])),
        "merges": len(exp["merges"]), "iterations": st["iterations"], "steps_with_children": st["steps"],
        "partitions": st["partitions"], "hops_per_child": round(st["hops"] / n, 2), "launches_per_child": round(st["launches"] / n, 1),
        "control_reads_per_child": round(st["reads"] / n, 2),
        "partition_share": round(st["partition_s"] * 1e3 / med, 3), "tables_share": round(st["tables_s"] * 1e3 / med, 3)}), flush=True)


print(json.dumps({"device": torch.cuda.get_device_name(0), "reps": REPS, "host_threads": torch.get_num_threads()}), flush=True)
f = load_merging_fixture()
for nn in (True, False):
    for chunk in (100, 5):
        trk = mesh_tracker(f["pre"], f["mask"], f["nb"], f["areas"], f["lat"], f["lon"], tm=f["time"], R_fill=1, T_fill=2,
                           area_filter_quartile=None, area_filter_absolute=5, overlap_threshold=THRESHOLD, nn_partitioning=nn,
                           timechunks=chunk)
        measure(f"fixture, chunks of {chunk}", trk, f["ids"], f["q"], f["e"],
                lambda: mm.split_and_merge(f["ids"], f["q"], f["e"], f["nb0"], f["areas"], f["lat"], f["lon"], THRESHOLD,
                                           [chunk] * (100 // chunk), nn))
for C, seed in ((4097, 7), (CELLS, 7)):
    mesh, ids = drifting_runs(seed, C)
    e, q = mo.weight_tables(mesh["areas"], mesh["lat"], mesh["lon"])
    for nn in (True, False):
        trk = mesh_tracker(ids > 0, mesh["mask"], mesh["nb0"] + 1, mesh["areas"], mesh["lat"], mesh["lon"], overlap_threshold=0.3,
                           nn_partitioning=nn, timechunks=3)
        measure("drifting runs", trk, ids, q, e,
                lambda: mm.split_and_merge(ids, q, e, mesh["nb0"], mesh["areas"], mesh["lat"], mesh["lon"], 0.3, [3, 3, 2], nn))
