"""One-off measurement (not a pytest file) of the tracker's pre-processing in time blocks (``HotPath.preprocess_blocked``,
``tracker(..., preprocess_block_steps=)``).  ``python tests/measure_preprocess_blocks.py [cost] [big]``:

* ``cost``: on 2 072 steps of 720 x 1440 (the 7-step pattern of tests/test_gpu_label_blocks.py repeated 296 times, built on
  the device) the whole-field ``run_preprocess`` and the blocked one at B = 16, 64, 256 and "auto", percentile and absolute
  filter, with the library calls of one blocked run timed one by one;
* ``big``: one ``tracker(allow_merging=False, preprocess_block_steps="auto").run()`` on a resident field whose number of
  steps is taken from the free device memory: ``tracking_memory_need`` exceeds it, the blocked need and
  ``labelling_memory_need`` fit.  Not started when that or the host memory for the ID field is not there."""
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import numpy as np
import torch

import marex_amd
import marex_amd.track as trk_mod
from marex_amd.detect import get_engine
from marex_amd.engine import HotPath
from marex_amd.zarr_io import DeviceDataArray

ny, nx = 720, 1440
C = ny * nx
hot = get_engine(0)
modes = sys.argv[1:] or ["cost", "big"]
KW = dict(R_fill=2, T_fill=2, allow_merging=False)


def pattern():
    import label_blocks_oracle as lbo

    rng = np.random.default_rng(2072)
    F = np.zeros((7, ny, nx), bool)
    F[1:] = lbo.blobby(rng, (6, ny // 4, nx // 4), 0.05).repeat(4, axis=1).repeat(4, axis=2)
    return torch.from_numpy(F.reshape(7, C).astype(np.uint8)).to(hot.device)


def field(T):
    return pattern().repeat(-(-T // 7), 1)[:T].contiguous()


def tracker_of(x, **kw):
    T = x.shape[0]
    da = DeviceDataArray(x.view(T, ny, nx), ("time", "lat", "lon"),
                         {"time": np.arange(T), "lat": np.linspace(-89.875, 89.875, ny), "lon": np.linspace(0.125, 359.875, nx)})
    return marex_amd.tracker(da, np.ones((ny, nx), bool), **KW, **kw)


def timed(fn, K=2):
    fn()
    hot.sync()
    torch.cuda.reset_peak_memory_stats()
    t0 = time.perf_counter()
    for _ in range(K):
        out = fn()
    hot.sync()
    return out, (time.perf_counter() - t0) / K * 1e3, torch.cuda.max_memory_allocated() / 1e9


def per_call(fn):
    per = {}
    real = HotPath.call

    def call(self, name, *args):
        self.sync()
        t0 = time.perf_counter()
        real(self, name, *args)
        self.sync()
        per.setdefault(name, []).append((time.perf_counter() - t0) * 1e3)

    HotPath.call = call
    try:
        fn()
    finally:
        HotPath.call = real
    return {k.replace("marex_", ""): {"calls": len(v), "ms": round(sum(v), 1)} for k, v in per.items()}


if "cost" in modes:
    x = field(2072)
    T = x.shape[0]
    for filt in (dict(area_filter_quartile=0.5), dict(area_filter_absolute=40)):
        (pre0, st0), ms0, pk0 = timed(lambda: tracker_of(x, **filt).run_preprocess())
        ref = pre0.device_tensor.clone()
        del pre0
        torch.cuda.empty_cache()
        print({"case": "whole field", "filter": filt, "T": T, "ms": round(ms0, 1), "peak_allocated_GB": round(pk0, 2),
               "stats": st0}, flush=True)
        for B in (16, 64, 256, "auto"):
            trk = tracker_of(x, preprocess_block_steps=B, **filt)
            (pre, st), ms, pk = timed(trk.run_preprocess)
            same = torch.equal(pre.device_tensor, ref) and tuple(st) == tuple(st0)
            planned = trk._preprocess_plan(hot, T, ny, C, True)[0]
            del pre
            torch.cuda.empty_cache()
            row = {"case": f"blocked, B = {B}", "filter": filt, "B": planned, "ms": round(ms, 1), "over_whole": round(ms / ms0, 2),
                   "equals_whole": same, "peak_allocated_GB": round(pk, 2)}
            if B == 64:
                row["calls"] = per_call(trk.run_preprocess)
            print(row, flush=True)
        del ref
        torch.cuda.empty_cache()
    del x
    torch.cuda.empty_cache()

if "big" in modes:
    free = trk_mod.tracker._free_bytes(hot)
    avail = 0
    for line in open("/proc/meminfo"):
        if line.startswith("MemAvailable"):
            avail = int(line.split()[1]) * 1024
    # the largest T whose resident input (n), blocked pre-processing (n + window) and labelling (n + 4 n + 8 per cell of a
    # block) fit three quarters of the free memory, the whole-field path (12 n and more) not
    T = int(0.75 * free / (6 * C + 1)) - 2048
    ok = T > 0
    if ok:
        whole = sum(trk_mod.tracking_memory_need(T, ny, nx, KW["R_fill"], KW["T_fill"], resident=True).values())
        lab = sum(trk_mod.labelling_memory_need(T, C).values())
        ok = whole > free - T * C and lab + T * C < free and 4 * T * C * 2 + (8 << 30) < avail
    if not ok:
        print({"case": "capability run", "skipped": "the pre-check failed", "free_GB": round(free / 1e9, 1),
               "host_available_GB": round(avail / 1e9, 1), "T": T}, flush=True)
    else:
        x = field(T)
        trk = tracker_of(x, preprocess_block_steps="auto", area_filter_quartile=0.5)
        torch.cuda.reset_peak_memory_stats()
        trk._check_memory(trk.data_bin.shape)
        B = trk._preprocess_plan(hot, T, ny, C, True)[0]
        hot.sync()
        t0 = time.perf_counter()
        pre, stats = trk.run_preprocess()
        hot.sync()
        t1 = time.perf_counter()
        events, merges, n = trk.run_tracking(pre)
        t2 = time.perf_counter()
        print({"case": f"tracker(preprocess_block_steps='auto') on {T} x {ny} x {nx} = {T * C} cells, resident input", "B": B,
               "free_GB_before": round(free / 1e9, 1), "whole_field_need_GB": round(whole / 1e9, 1),
               "preprocess_s": round(t1 - t0, 2), "labelling_and_host_copy_s": round(t2 - t1, 2), "N_events_final": n,
               "stats": stats, "peak_allocated_GB": round(torch.cuda.max_memory_allocated() / 1e9, 2)}, flush=True)
