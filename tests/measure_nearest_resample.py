"""One-off measurement (not a pytest file): nearest-cell resampling (``marex_nearest.hip``) between a synthetic quasi-uniform
mesh of ``NR_CELLS`` cells (default 1448 x 1448 = 2.1 M, a Fibonacci lattice: cell k at ``z = 1 - (2 k + 1) / C`` and the
golden angle times k in longitude) and a regular ``NR_NY`` x ``NR_NX`` grid (default 720 x 1440), in both directions.

Index, per direction, without a mask and with an ocean-like ``src_mask`` that removes a third of the source cells in blocks
of 15 x 20 degrees; the voxel search at the default ``voxels`` and at half and double of it:
(c) ``marex_voxel_count_f64``;  (p) the prefix sum (torch);  (s) ``marex_voxel_scatter_f64``;  (v) ``marex_nearest_voxel_f64``
    with the default ``max_rings``, and the targets it left open;  (f) the compaction and the brute kernel over those;
(b) ``marex_nearest_brute_f64`` over every target (fewer repetitions: it is the slow one);
(k) baseline: ``scipy.spatial.cKDTree`` build plus query on the host, ``NR_WORKERS`` workers (default 16);
(w) the whole ``marex_amd.nearest_cell_index`` call from host coordinates, unit vectors and distances included.
(x) the crossover of ``method="auto"``: ``HotPath.nearest_index`` from resident vectors with either method, a host clock
    that ends with the result on the host, for random sources and targets of 1 k .. 1 M cells (``NR_ONLY_SWEEP=1``: alone).
Gather, ``NR_STEPS`` steps (default 365) of the mesh to the grid, for uint8, int32 and float32:
(g) the kernel;  (d) baseline: a device-to-device copy of as many bytes as the gather writes;
(t) baseline: ``torch.index_select`` with ``torch.where`` for the fill, from the resident field;
(r) the whole ``marex_amd.resample_nearest`` call from a resident field;  (h) from a host array.

Device times lie between two device events, wall times are host clocks that end in a synchronise; medians of REPS after one
warm-up, with the range."""
import json
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import numpy as np
import torch

import marex_amd
from marex_amd import resample as rs
from marex_amd.detect import get_engine

REPS = int(os.environ.get("NR_REPS", 5))
BRUTE_REPS = int(os.environ.get("NR_BRUTE_REPS", 2))
C = int(os.environ.get("NR_CELLS", 1448 * 1448))
ny, nx = int(os.environ.get("NR_NY", 720)), int(os.environ.get("NR_NX", 1440))
T = int(os.environ.get("NR_STEPS", 365))
WORKERS = int(os.environ.get("NR_WORKERS", 16))
eng = get_engine(0)
print(json.dumps({"device": torch.cuda.get_device_name(0), "reps": REPS, "mesh_cells": C, "grid": [ny, nx], "steps": T}), flush=True)


def med(v):
    return {"ms_median": round(statistics.median(v), 3), "ms_min": round(min(v), 3), "ms_max": round(max(v), 3)}


def device_ms(fn, reps=REPS, prepare=lambda: None):
    out = []
    for _ in range(reps + 1):
        prepare()
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        eng.sync()
        a.record()
        fn()
        b.record()
        eng.sync()
        out.append(a.elapsed_time(b))
    return out[1:]


def wall(fn, reps=REPS):
    out = []
    for _ in range(reps + 1):
        eng.sync()
        t0 = time.perf_counter()
        fn()
        eng.sync()
        out.append((time.perf_counter() - t0) * 1e3)
    return out[1:]


def say(variant, **kw):
    print(json.dumps(dict({"variant": variant}, **kw)), flush=True)


k = np.arange(C, dtype=np.float64)
mesh_lat = np.degrees(np.arcsin(1.0 - (2.0 * k + 1.0) / C))
mesh_lon = np.mod(k * (180.0 * (3.0 - np.sqrt(5.0))), 360.0) - 180.0
gl, go = -90.0 + (np.arange(ny) + 0.5) * (180.0 / ny), -180.0 + (np.arange(nx) + 0.5) * (360.0 / nx)
grid_lat, grid_lon = (a.reshape(-1) for a in np.meshgrid(gl, go, indexing="ij"))


def ocean(lat, lon):
    return (np.floor((lat + 90.0) / 15.0) + np.floor((lon + 180.0) / 20.0)) % 3 != 0


def index_direction(name, s_lat, s_lon, d_lat, d_lon):
    for masked in (False, True):
        ok = ocean(s_lat, s_lon) if masked else np.ones(s_lat.size, bool)
        src_h = np.ascontiguousarray(rs.unit_vectors(s_lat, s_lon)[:, ok])
        ids_h = np.flatnonzero(ok).astype(np.int32)
        dst_h = rs.unit_vectors(d_lat, d_lon)
        src, ids, dst = eng._dev(src_h), eng._dev(ids_h), eng._dev(dst_h)
        N, M = src_h.shape[1], dst_h.shape[1]
        tag = f"{name}, {'ocean mask' if masked else 'no mask'}: {N} sources, {M} targets"
        n0 = rs.default_voxels(N)
        results = {}
        for n in (n0, max(1, n0 // 2), min(1024, 2 * n0)):
            rings = rs.default_max_rings(n)
            count = torch.zeros(n ** 3, dtype=torch.int32, device=eng.device)
            off = torch.zeros(n ** 3 + 1, dtype=torch.int32, device=eng.device)
            srt, sid = torch.empty_like(src), torch.empty_like(ids)
            index, q = torch.empty(M, dtype=torch.int32, device=eng.device), torch.empty(M, dtype=torch.float64, device=eng.device)
            flag = torch.empty(M, dtype=torch.uint8, device=eng.device)
            tc = device_ms(lambda: eng.call("marex_voxel_count_f64", src, N, n, count), prepare=lambda: count.zero_())
            tp = device_ms(lambda: off[1:].copy_(torch.cumsum(count, 0)))
            ts = device_ms(lambda: eng.call("marex_voxel_scatter_f64", src, ids, N, n, off, count, srt, sid), prepare=lambda: count.zero_())
            tv = device_ms(lambda: eng.call("marex_nearest_voxel_f64", srt, sid, N, off, n, dst, M, rings, float("inf"), index, q, flag))
            sel = torch.nonzero(flag).reshape(-1).to(torch.int32)
            K = int(sel.numel())
            occupied = int((off[1:] != off[:-1]).sum())

            def fallback():
                s = torch.nonzero(flag).reshape(-1).to(torch.int32)
                if s.numel():
                    eng.call("marex_nearest_brute_f64", srt, sid, N, dst, M, s, int(s.numel()), index, q)

            tf = device_ms(fallback, reps=min(REPS, 2))
            results[n] = index.cpu().numpy()
            total = statistics.median(tc) + statistics.median(tp) + statistics.median(ts) + statistics.median(tv) + statistics.median(tf)
            say(f"voxel search, {tag}", voxels=n, max_rings=rings, table_MB=round(4 * (n ** 3 + 1) / 1e6, 1), occupied_voxels=occupied,
                cells_per_occupied_voxel=round(N / occupied, 2), count=med(tc), prefix_sum=med(tp), scatter=med(ts), search=med(tv),
                fallback_targets=K, fallback=med(tf), ms_sum_of_medians=round(total, 3))
            del count, off, srt, sid, flag
        bi, bq = torch.empty(M, dtype=torch.int32, device=eng.device), torch.empty(M, dtype=torch.float64, device=eng.device)
        tb = device_ms(lambda: eng.call("marex_nearest_brute_f64", src, ids, N, dst, M, None, M, bi, bq), reps=BRUTE_REPS)
        brute = bi.cpu().numpy()
        say(f"brute kernel, {tag}", **med(tb), pairs_per_s=round(N * M / statistics.median(tb) * 1e3, 0),
            voxel_results_equal_brute={n: bool(np.array_equal(v, brute)) for n, v in results.items()})
        from scipy.spatial import cKDTree

        tk = []
        for _ in range(2):
            t0 = time.perf_counter()
            near = cKDTree(src_h.T).query(dst_h.T, k=1, workers=WORKERS)[1]
            tk.append((time.perf_counter() - t0) * 1e3)
        say(f"cKDTree build and query on the host, {WORKERS} workers, {tag}", ms=[round(v, 1) for v in tk],
            targets_that_differ_from_brute=int((ids_h[near] != brute).sum()))
        tw = wall(lambda: marex_amd.nearest_cell_index(s_lat, s_lon, d_lat, d_lon, src_mask=ok if masked else None), reps=2)
        say(f"nearest_cell_index, whole call from host coordinates, {tag}", **med(tw))
        del src, ids, dst, bi, bq
        torch.cuda.empty_cache()
    return brute  # of the masked run


def sweep():
    rng = np.random.default_rng(3)

    def points(n):
        return eng._dev(rs.unit_vectors(np.degrees(np.arcsin(rng.uniform(-1, 1, n))), rng.uniform(-180, 180, n)))

    for N in (1 << 10, 1 << 12, 1 << 14, 1 << 16, 1 << 18, 1 << 20):
        src = points(N)
        for M in (1 << 10, 1 << 14, 1 << 17, 1 << 20):
            if N * M > 1 << 36:
                continue
            dst = points(M)
            n = rs.default_voxels(N)
            res = {}
            tb = wall(lambda: res.__setitem__("b", eng.nearest_index(src, None, dst, method="brute")), reps=3)
            tv = wall(lambda: res.__setitem__("v", eng.nearest_index(src, None, dst, method="voxel", voxels=n, max_rings=rs.default_max_rings(n))), reps=3)
            say("crossover", sources=N, targets=M, log2_pairs=round(float(np.log2(N * M)), 1), voxels=n, brute=med(tb), voxel=med(tv),
                fallback_targets=res["v"]["fallback"], same=bool(np.array_equal(res["b"]["index"], res["v"]["index"])),
                brute_over_voxel=round(statistics.median(tb) / statistics.median(tv), 2))


if int(os.environ.get("NR_ONLY_SWEEP", "0")):
    sweep()
    sys.exit(0)
if not int(os.environ.get("NR_SKIP_INDEX", "0")):
    sweep()
    index_direction("mesh -> grid", mesh_lat, mesh_lon, grid_lat, grid_lon)
    index_direction("grid -> mesh", grid_lat, grid_lon, mesh_lat, mesh_lon)

# ------------------------------------------------------------------ the gather: T steps of the mesh to the grid
ds = marex_amd.nearest_cell_index(mesh_lat, mesh_lon, gl, go, dst_rectilinear=True, src_mask=ocean(mesh_lat, mesh_lon), max_distance_km=300.0)
idx_h = ds["index"].values.reshape(-1)
M = idx_h.size
idx = eng._dev(idx_h)
say("the gather's index: mesh -> grid, ocean mask, max_distance_km=300", targets=M, without_a_source=int((idx_h < 0).sum()))
g = torch.Generator(device=eng.device).manual_seed(1)
for name, dt, item, fill in (("uint8", torch.uint8, 1, 0), ("int32", torch.int32, 4, 0), ("float32", torch.float32, 4, float("nan"))):
    if dt == torch.float32:
        x = torch.randn((T, C), generator=g, device=eng.device)
    else:
        x = torch.randint(0, 200, (T, C), generator=g, device=eng.device, dtype=dt)
    out = torch.empty((T, M), dtype=dt, device=eng.device)
    tg = device_ms(lambda: eng.resample_nearest(x, idx, out, fill))
    other = torch.empty_like(out)
    td = device_ms(lambda: other.copy_(out))
    del other
    safe, none = idx.clamp(min=0).long(), (idx < 0)[None, :]
    res = {}
    tt = device_ms(lambda: res.__setitem__("t", torch.where(none, torch.full((), fill, dtype=dt, device=eng.device), torch.index_select(x, 1, safe))), reps=3)
    same = bool(torch.equal(res["t"].view(torch.uint8), out.view(torch.uint8)))
    del res
    wrote = T * M * item
    say(f"gather, {name}", kernel=med(tg), GB_per_s_written=round(wrote / statistics.median(tg) / 1e6, 1), copy_of_the_output=med(td),
        copy_GB_per_s_written=round(wrote / statistics.median(td) / 1e6, 1), kernel_over_copy=round(statistics.median(tg) / statistics.median(td), 2),
        torch_index_select_where=med(tt), torch_equals_the_kernel=same)
    tr = wall(lambda: marex_amd.resample_nearest(x, ds, fill=fill), reps=3)
    x_h = x.cpu().numpy()
    del x, out
    torch.cuda.empty_cache()
    th = wall(lambda: marex_amd.resample_nearest(x_h, ds, fill=fill), reps=2)
    say(f"resample_nearest, whole call, {name}", resident=med(tr), host_array=med(th))
    del x_h
