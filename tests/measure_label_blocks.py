"""One-off measurement (not a pytest file) of the labelling in time blocks (``HotPath.label_objects_3d(...,
max_block_cells=)``).  ``python tests/measure_label_blocks.py [cfg2] [big] [tracker]``:

* ``cfg2``: on the blobby 5 % field of tests/measure_track.py (1826 x 720 x 1440 after trimming) the single call, the
  blocked path forced to 2 and to 4 blocks, and a device copy of the ID field as the yardstick of one streaming pass;
* ``big``: 2 072 steps of 720 x 1440 (2^31 cells and more; the 7-step pattern of tests/test_gpu_label_blocks.py repeated
  296 times), the passes one by one;
* ``tracker``: ``tracker(allow_merging=False).run()`` on that field end to end, the host copy of the ID field included,
  when the host has the memory for it."""
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import numpy as np
import torch

import marex_amd
from marex_amd.detect import get_engine
from marex_amd.engine import HotPath
from marex_amd.zarr_io import DeviceDataArray

ny, nx = 720, 1440
C = ny * nx
hot = get_engine(0)
modes = sys.argv[1:] or ["cfg2", "big", "tracker"]


def timed_calls(fn):
    """Run ``fn`` with every library call synchronised and timed: ``(result, {entry point: [ms, ...]}, wall ms)``."""
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
        hot.sync()
        t0 = time.perf_counter()
        out = fn()
        hot.sync()
        wall = (time.perf_counter() - t0) * 1e3
    finally:
        HotPath.call = real
    return out, per, wall


def wall_ms(fn, K=3):
    for _ in range(2):
        fn()
    hot.sync()
    t0 = time.perf_counter()
    for _ in range(K):
        fn()
    hot.sync()
    return (time.perf_counter() - t0) / K * 1e3


def summary(per):
    return {k.replace("marex_", ""): {"calls": len(v), "ms": round(sum(v), 2)} for k, v in per.items()}


def cfg2_field(frac=0.05, seed=1):
    """The blobby field of tests/measure_track.py: smoothed device noise above its 95 % quantile, ocean cells only."""
    from marex_amd import binning, calendar, synth

    T, W = 3652, 5
    tm = calendar.daily_time_axis("2015-01-01", T)
    cal = calendar.build_calendar(tm, window_year_baseline=W)
    x = hot.synth_field(synth.make_tables(tm, ny, nx))
    r = hot.shifting_hobday(x, hot.upload_calendar(cal), W=W, S=21, bins=binning.hobday_bins(), q=0.95, wd=11, ws=5, ny=ny, nx=nx)
    T_out, mask = r["extreme_events"].shape[0], r["mask"].clone()
    del x, r
    torch.cuda.empty_cache()
    g = torch.Generator(device=hot.device).manual_seed(seed)
    f = torch.randn((1, 1, T_out, ny, nx), generator=g, device=hot.device)
    for _ in range(2):
        f = torch.nn.functional.avg_pool3d(f, (3, 13, 17), stride=1, padding=(1, 6, 8), count_include_pad=False)
    f = f.reshape(T_out, C)
    thr = torch.quantile(f.reshape(-1)[:: 113][: 16_000_000], 1.0 - frac)
    out = (f > thr).to(torch.uint8) * mask.reshape(1, -1)
    del f
    torch.cuda.empty_cache()
    return out


def big_field(reps=296):
    import label_blocks_oracle as lbo

    rng = np.random.default_rng(2072)
    F = np.zeros((7, ny, nx), bool)
    F[1:] = lbo.blobby(rng, (6, ny // 4, nx // 4), 0.05).repeat(4, axis=1).repeat(4, axis=2)
    return torch.from_numpy(F.reshape(7, C).astype(np.uint8)).to(hot.device).repeat(reps, 1)


if "cfg2" in modes:
    xb = cfg2_field()
    T = xb.shape[0]
    ws = {}
    single = wall_ms(lambda: hot.label_objects_3d(xb, ny, nx, True, wsp=ws))
    ref = hot.label_objects_3d(xb, ny, nx, True, wsp=ws)
    n_ref, ids_ref = int(ref["n"].item()), ref["ids"].clone()
    print({"case": "cfg2 blobby 5 %, single call", "T": T, "ms": round(single, 2), "events": n_ref,
           "Gcells_per_s": round(T * C / single / 1e6, 1)}, flush=True)
    dst = torch.empty_like(ids_ref)
    copy = wall_ms(lambda: dst.copy_(ids_ref))
    print({"case": "device copy of the ID field (4 B read + 4 B written per cell)", "ms": round(copy, 2),
           "TB_per_s": round(8 * T * C / copy / 1e9, 2)}, flush=True)
    del dst, ws, ref
    torch.cuda.empty_cache()
    for nb in (2, 4):
        steps = -(-T // nb)
        wsb = {}
        fn = lambda: hot.label_objects_3d(xb, ny, nx, True, wsp=wsb, max_block_cells=steps * C)  # noqa: E731
        ms = wall_ms(fn)
        r, per, wall = timed_calls(fn)
        same = int(r["n"].item()) == n_ref and torch.equal(r["ids"], ids_ref)
        print({"case": f"cfg2 blobby 5 %, {nb} blocks of {steps} steps", "ms": round(ms, 2), "over_single_ms": round(ms - single, 2),
               "equals_single_call": same, "synchronised_ms": round(wall, 2), "passes": summary(per)}, flush=True)
        del wsb, r
        torch.cuda.empty_cache()
    del xb, ids_ref
    torch.cuda.empty_cache()

if "big" in modes:
    big = big_field()
    T = big.shape[0]
    wsb = {}
    fn = lambda: hot.label_objects_3d(big, ny, nx, True, wsp=wsb)  # noqa: E731
    ms = wall_ms(fn, K=2)
    r, per, wall = timed_calls(fn)
    print({"case": f"{T} x {ny} x {nx} = {T * C} cells, default plan", "ms": round(ms, 2), "events": int(r["n"].item()),
           "Gcells_per_s": round(T * C / ms / 1e6, 1), "synchronised_ms": round(wall, 2), "passes": summary(per),
           "label3d_ms_per_block": [round(v, 2) for v in per["marex_label3d_i32"]],
           "apply_ms_per_block": [round(v, 2) for v in per["marex_label_apply_table_i32"]],
           "peak_allocated_GB": round(torch.cuda.max_memory_allocated() / 1e9, 2)}, flush=True)
    del big, wsb, r
    torch.cuda.empty_cache()

if "tracker" in modes:
    avail = 0
    for line in open("/proc/meminfo"):
        if line.startswith("MemAvailable"):
            avail = int(line.split()[1]) * 1024
    T = 7 * 296
    need_host = 4 * T * C * 2 + (4 << 30)  # the ID field, the Dataset's copy of it, pinned staging and slack
    if avail < need_host:
        print({"case": "tracker end to end", "skipped": f"host has {avail / 1e9:.1f} GB available, {need_host / 1e9:.1f} GB wanted"})
    else:
        big = big_field()
        da = DeviceDataArray(big.view(T, ny, nx), ("time", "lat", "lon"),
                             {"time": np.arange(T), "lat": np.linspace(-89.875, 89.875, ny), "lon": np.linspace(0.125, 359.875, nx)})
        trk = marex_amd.tracker(da, np.ones((ny, nx), bool), R_fill=2, T_fill=2, area_filter_quartile=0.5, allow_merging=False)
        trk._check_memory(da.shape)  # what run() does first
        hot.sync()
        t0 = time.perf_counter()
        pre, stats = trk.run_preprocess()
        hot.sync()
        t1 = time.perf_counter()
        events, merges, n = trk.run_tracking(pre)
        t2 = time.perf_counter()
        ds = trk.run_stats_attributes(events, merges, stats, n)
        t3 = time.perf_counter()
        print({"case": f"tracker(allow_merging=False) on {T * C} cells, device-resident input", "preprocess_s": round(t1 - t0, 2),
               "labelling_and_host_copy_s": round(t2 - t1, 2), "stats_s": round(t3 - t2, 2), "total_s": round(t3 - t0, 2),
               "N_events_final": n, "ID_field_GB": round(4 * T * C / 1e9, 2), "host_available_GB": round(avail / 1e9, 1),
               "peak_allocated_GB": round(torch.cuda.max_memory_allocated() / 1e9, 2)}, flush=True)
