"""One-off measurement (not a pytest file): the mesh tracker's device stages -- label + rank (``HotPath.label_objects_mesh``),
object moments, overlaps and area -- on a synthetic triangular mesh of 1448 x 1448 = 2.1 M cells x 365 steps at 10 %
coverage, and, as the yardstick, the gridded ``marex_object_moments_i32`` / ``marex_overlap_pairs_i32`` on the same ID field
read as a 1448 x 1448 grid (the same number of cells, the same coverage, the same objects).

Per stage: the median of REPS timings after WARM warm-up calls.  "kernel_ms" brackets the library call alone with device
events (tables and scratch made before); "call_ms" is the engine method on the host clock, ending in a synchronise, with
its sizing passes, device-to-host copies, sort and float64 division.  Bytes per cell the kernels must read: 4 (the ID) plus
32 (moments) or 8 (overlaps) of ``q`` per active cell on the mesh, 4 on the grid -- the expected time ratio at coverage p is
(4 + 32 p) / 4 for the moments and (8 + 8 p2) / 8 for the overlaps (two slices per cell pair; p2 = the share of cells active
in both)."""
import json
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch

from marex_amd.detect import get_engine
from marex_amd.track import mesh_weight_tables

NY = NX = 1448
T = int(os.environ.get("MESH_T", 365))
COVER = 0.10
WARM, REPS = 2, 7
hot = get_engine(0)
dev = hot.device
C = NY * NX


def triangular_mesh():
    """Cells in rows of NX: left and right in the row, and up (even columns) or down (odd columns): 0-based, -1 = none."""
    c = np.arange(C, dtype=np.int64)
    y, x = c // NX, c % NX
    left = np.where(x > 0, c - 1, -1)
    right = np.where(x < NX - 1, c + 1, -1)
    vert = np.where(x % 2 == 0, np.where(y > 0, c - NX, -1), np.where(y < NY - 1, c + NX, -1))
    return np.stack([left, right, vert]).astype(np.int32)


def blobby(frac, seed=1):
    g = torch.Generator(device=dev).manual_seed(seed)
    out = torch.empty((T, C), dtype=torch.uint8, device=dev)
    thr = None
    for t0 in range(0, T, 73):  # in pieces: the smoothing holds a few float32 copies
        n = min(73, T - t0)
        f = torch.randn((1, 1, n, NY, NX), generator=g, device=dev)
        for _ in range(2):
            f = torch.nn.functional.avg_pool3d(f, (3, 13, 17), stride=1, padding=(1, 6, 8), count_include_pad=False)
        f = f.reshape(n, C)
        if thr is None:
            thr = torch.quantile(f.reshape(-1)[::37][:16_000_000], 1.0 - frac)
        out[t0:t0 + n] = (f > thr).to(torch.uint8)
        del f
    torch.cuda.empty_cache()
    return out


def kernel_ms(fn):
    for _ in range(WARM):
        fn()
    ms = []
    for _ in range(REPS):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        ms.append(a.elapsed_time(b))
    return statistics.median(ms), min(ms), max(ms)


def call_ms(fn):
    for _ in range(WARM):
        fn()
    ms = []
    for _ in range(REPS):
        hot.sync()
        t0 = time.perf_counter()
        fn()
        hot.sync()
        ms.append((time.perf_counter() - t0) * 1e3)
    return statistics.median(ms), min(ms), max(ms)


def row(stage, what, t, cells, nbytes):
    med, lo, hi = t
    print(json.dumps({"stage": stage, "timing": what, "median_ms": round(med, 3), "min_ms": round(lo, 3), "max_ms": round(hi, 3),
                      "Gcells_per_s": round(cells / med / 1e6, 2), "GB_per_s_of_bytes_needed": round(nbytes / med / 1e6, 1)}), flush=True)


rng = np.random.default_rng(0)
lat = np.degrees(np.arcsin(rng.uniform(-1, 1, C)))
lon = rng.uniform(-180, 180, C)
e, q_host = mesh_weight_tables(10.0 ** rng.uniform(6, 8, C), lat, lon)
q = torch.from_numpy(q_host).to(dev)
nbr = torch.from_numpy(triangular_mesh()).to(dev)
mask = torch.ones(C, dtype=torch.uint8, device=dev)
x = blobby(COVER)
cover = float(x.sum(dtype=torch.int64).item()) / x.numel()
cells = T * C
print(json.dumps({"device": torch.cuda.get_device_name(0), "T": T, "C": C, "coverage": round(cover, 4), "reps": REPS, "warm": WARM}), flush=True)

# label + rank (per-timestep IDs), then IDs unique in time: the field every later stage reads
row("label + rank", "call_ms", call_ms(lambda: hot.label_objects_mesh(x, mask, nbr)), cells, cells * (1 + 4))
ids = hot.unique_ids_in_time(hot.label_objects_mesh(x, mask, nbr)["ids"])
hi = hot.ids_minmax(ids)[1]
active = int((ids > 0).sum().item())
both = int(((ids[:-1] > 0) & (ids[1:] > 0)).sum().item())
print(json.dumps({"objects": hi, "active_cells": active, "cells_active_in_both_slices": both}), flush=True)

area_out = torch.empty(T, dtype=torch.int64, device=dev)
row("area", "kernel_ms", kernel_ms(lambda: hot.call("marex_mesh_area_i64", x, T, C, q[0], area_out)), cells, cells + 8 * active)
row("area", "call_ms", call_ms(lambda: hot.mesh_area(x, q, e)), cells, cells + 8 * active)

# moments: mesh against the gridded kernel on the same field, same slots
tmin, _, off, total = hot._object_spans(ids, T, C, hi, "measure", "spans")
n_slots = int(total.item())
acc = torch.empty((n_slots, 5), dtype=torch.int64, device=dev)
t_mesh = kernel_ms(lambda: hot.call("marex_mesh_object_moments_i64", ids, T, C, q, tmin, off, n_slots, acc))
t_grid = kernel_ms(lambda: hot.call("marex_object_moments_i32", ids, T, NY, NX, tmin, off, n_slots, acc))
row("moments (mesh)", "kernel_ms", t_mesh, cells, 4 * cells + 32 * active)
row("moments (grid, yardstick)", "kernel_ms", t_grid, cells, 4 * cells)
row("moments (mesh)", "call_ms", call_ms(lambda: hot.mesh_object_moments(ids, q, e)), cells, 4 * cells + 32 * active)
row("moments (grid, yardstick)", "call_ms", call_ms(lambda: hot.object_moments(ids, NY, NX, wrap=True)), cells, 4 * cells)
print(json.dumps({"moments_ratio_measured": round(t_mesh[0] / t_grid[0], 3),
                  "moments_ratio_expected_from_bytes": round((4 * cells + 32 * active) / (4 * cells), 3)}), flush=True)
del acc

# overlaps: the insert + compact call, tables sized as the engine sizes them
stats = torch.zeros(4, dtype=torch.int64, device=dev)
hot.call("marex_overlap_count_i32", ids, T, C, stats)
runs = int(stats[1].item())
cap = max(64, 1 << (2 * runs - 1).bit_length())
keys, sums = (torch.empty(cap, dtype=torch.int64, device=dev) for _ in range(2))
out_k, out_s = (torch.empty(runs, dtype=torch.int64, device=dev) for _ in range(2))
sums2, out_s2 = torch.empty((cap, 2), dtype=torch.int64, device=dev), torch.empty((runs, 2), dtype=torch.int64, device=dev)
pair_cells = (T - 1) * C
t_mesh = kernel_ms(lambda: hot.call("marex_mesh_overlap_pairs_i64", ids, T, C, q[0], cap, keys, sums2, stats, runs, out_k, out_s2))
t_grid = kernel_ms(lambda: hot.call("marex_overlap_pairs_i32", ids, T, C, cap, keys, sums, stats, runs, out_k, out_s))
row("overlaps (mesh)", "kernel_ms", t_mesh, pair_cells, 8 * pair_cells + 8 * both)
row("overlaps (grid, yardstick)", "kernel_ms", t_grid, pair_cells, 8 * pair_cells)
row("overlaps (mesh)", "call_ms", call_ms(lambda: hot.mesh_overlap_pairs(ids, q, e)), pair_cells, 8 * pair_cells + 8 * both)
row("overlaps (grid, yardstick)", "call_ms", call_ms(lambda: hot.overlap_pairs(ids)), pair_cells, 8 * pair_cells)
print(json.dumps({"overlaps_ratio_measured": round(t_mesh[0] / t_grid[0], 3), "hash_table_entries": cap, "runs": runs,
                  "overlaps_ratio_expected_from_bytes": round((8 * pair_cells + 8 * both) / (8 * pair_cells), 3)}), flush=True)
