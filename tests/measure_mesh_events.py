"""One-off measurement (not a pytest file): the rename-and-accumulate pass of cluster renaming on a mesh.  Input: drifting
runs (tests/mesh_merge_scenarios.py) on a ring mesh of ``EVENT_CELLS`` cells (default 2^20) x ``EVENT_STEPS`` timesteps
(default 64), the events taken from the time overlaps of the runs.

(a) ``HotPath.mesh_event_rename``: one kernel, in place.
(b) the composition it replaces, from calls the library had before it: ``clone`` of the field, ``relabel``, and
    ``mesh_object_moments`` on the relabelled field (its sizing passes included; it does not even deliver global_ID, which
    would take one more pass over both copies).
(c) the three entries of ``tracker._stage_times`` of a whole ``run()`` on the same cells, tracked over the ring edges only
    (centroid partition).

Wall times are host clocks that end in a synchronise (median of REPS after one warm-up); for (a) also the device time of
the bare library call between two events.  Bytes are counted from the shapes: 4 per cell for every read or write of the
field, 32 per cell that holds an event for the weights; the share is of the 8 TB/s HBM peak used in DESIGN.md."""
import json
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import numpy as np
import torch

import mesh_events_oracle as me
import mesh_objects_oracle as mo
from mesh_merge_scenarios import drifting_runs
from test_mesh_tracker_host import mesh_tracker

from marex_amd.detect import get_engine

REPS = 7
CELLS = int(os.environ.get("EVENT_CELLS", 2 ** 20))
STEPS = int(os.environ.get("EVENT_STEPS", 64))
PEAK = 8e12


def timed(fn, prepare, sync):
    ms = []
    for k in range(REPS + 1):  # the first one warms up
        arg = prepare()
        sync()
        t0 = time.perf_counter()
        out = fn(arg)
        sync()
        ms.append((time.perf_counter() - t0) * 1e3)
    return statistics.median(ms[1:]), min(ms[1:]), max(ms[1:]), out


def report(name, med, lo, hi, nbytes, **extra):
    print(json.dumps(dict({"variant": name, "ms_median": round(med, 3), "ms_min": round(lo, 3), "ms_max": round(hi, 3),
                           "bytes": int(nbytes), "GB_per_s": round(nbytes / med / 1e6, 1),
                           "share_of_8TBs": round(nbytes / (med * 1e-3) / PEAK, 4)}, **extra)), flush=True)


eng = get_engine(0)
print(json.dumps({"device": torch.cuda.get_device_name(0), "reps": REPS, "T": STEPS, "C": CELLS}), flush=True)
mesh, ids_h = drifting_runs(7, CELLS, T=STEPS)
e, q_h = mo.weight_tables(mesh["areas"], mesh["lat"], mesh["lon"])
ids, q = torch.from_numpy(ids_h).to(eng.device), torch.from_numpy(q_h).to(eng.device)
pairs = eng.mesh_overlap_pairs(ids, q, e)[:, :2].astype(np.int64)
lut, N = me.event_table(ids_h, pairs)
n, held = STEPS * CELLS, int((ids_h > 0).sum())
print(json.dumps({"objects": int(ids_h.max()), "events": N, "cells_with_an_event": held, "share": round(held / n, 3)}), flush=True)

# (a) the fused pass
med, lo, hi, ra = timed(lambda w: (eng.mesh_event_rename(w, lut, N, q, e), w), ids.clone, eng.sync)
bytes_a = 8 * n + 32 * held
report("a: mesh_event_rename", med, lo, hi, bytes_a, full_size_buffers=1)
lut_d = torch.from_numpy(lut).to(eng.device)
acc = torch.empty((STEPS * N, 5), dtype=torch.int64, device=eng.device)
gid = torch.empty(STEPS * N, dtype=torch.int32, device=eng.device)
ev = []
for k in range(REPS + 1):
    w = ids.clone()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    eng.sync()
    a.record()
    eng.call("marex_mesh_event_rename_i64", w, STEPS, CELLS, lut_d, lut.size, N, q, acc, gid)
    b.record()
    eng.sync()
    ev.append(a.elapsed_time(b))
report("a: the library call alone (device events)", statistics.median(ev[1:]), min(ev[1:]), max(ev[1:]), bytes_a)


# (b) clone + relabel + moments of the relabelled field
def composition(w):
    orig = w.clone()
    eng.relabel(w, lut)
    return eng.mesh_object_moments(w, q, e), w, orig


med_b, lo, hi, rb = timed(composition, ids.clone, eng.sync)
# clone: read + write; relabel: read + write; moments: the minimum / maximum pass, the span pass and the sums read the field
bytes_b = (8 + 8 + 12) * n + 32 * held
report("b: clone + relabel + mesh_object_moments", med_b, lo, hi, bytes_b, full_size_buffers=2)
same_field = bool(torch.equal(ra[1], rb[1]))
mom = ra[0]["mom"]
pres = mom[..., 0] > 0
same_sums = bool(np.array_equal(mom[pres][:, 0], rb[0]["cells"]))
print(json.dumps({"a_over_b": round(med / med_b, 3), "same_event_field": same_field, "same_cell_counts": same_sums}), flush=True)
del ra, rb, acc, gid, ids
torch.cuda.empty_cache()

# (c) the whole run, over the ring edges only: the chords would fuse the seven runs into objects of more than ten parents
ring = np.zeros((3, CELLS), np.int32)
ring[0], ring[1] = (np.arange(CELLS) + 1) % CELLS + 1, (np.arange(CELLS) - 1) % CELLS + 1
trk = mesh_tracker(ids_h > 0, mesh["mask"], ring, mesh["areas"], mesh["lat"], mesh["lon"], R_fill=1, T_fill=2,
                   area_filter_quartile=None, area_filter_absolute=5, overlap_threshold=0.3, nn_partitioning=False, timechunks=8)
runs = []
for k in range(3):
    eng.sync()
    t0 = time.perf_counter()
    ds = trk.run()
    eng.sync()
    runs.append(dict({k2: round(v * 1e3, 2) for k2, v in trk._stage_times.items()}, run_ms=round((time.perf_counter() - t0) * 1e3, 2)))
med_run = {k2: statistics.median(r[k2] for r in runs[1:]) for k2 in runs[0]}
print(json.dumps({"variant": "c: run(), centroid partition, chunks of 8", "first_run": runs[0], "median_of_2_after_warm_up": med_run,
                  "events": int(ds.attrs["N_events_final"]), "merges": int(ds.attrs["total_merges"]),
                  "iterations": trk._merge_stats["iterations"]}), flush=True)
