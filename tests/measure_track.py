"""One-off measurement (not a pytest file): the 3-D labelling (``HotPath.label_objects_3d``) and the basic tracker
(``marex_amd.tracker(..., allow_merging=False).run()``) stage by stage at the size of cfg2 (1826 x 720 x 1440 after
trimming).

* worst case: the extreme mask the hot path produces on the device from the synthetic cfg2 field; its white-noise
  extremes close (R_fill = 8, T_fill = 2) into one giant component that spans every timestep;
* blobby: a 5 % mask of smoothed device noise of the same shape, whose objects look like real extreme events."""
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch

import marex_amd
from marex_amd import binning, calendar, synth
from marex_amd.detect import get_engine
from marex_amd.zarr_io import DeviceDataArray

ny, nx, T, W = 720, 1440, 3652, 5
hot = get_engine(0)
tm = calendar.daily_time_axis("2015-01-01", T)
cal = calendar.build_calendar(tm, window_year_baseline=W)
dcal = hot.upload_calendar(cal)
bt = binning.hobday_bins()
x = hot.synth_field(synth.make_tables(tm, ny, nx))
r = hot.shifting_hobday(x, dcal, W=W, S=21, bins=bt, q=0.95, wd=11, ws=5, ny=ny, nx=nx)
ext, mask = r["extreme_events"], r["mask"]
del x, r
torch.cuda.empty_cache()
T_out = ext.shape[0]
mask_h = mask.cpu().numpy().astype(bool).reshape(ny, nx)


def blobby(frac=0.05, seed=1):
    g = torch.Generator(device=hot.device).manual_seed(seed)
    f = torch.randn((1, 1, T_out, ny, nx), generator=g, device=hot.device)
    for _ in range(2):  # two box passes ~ a Gaussian of (1, 6, 8) cells
        f = torch.nn.functional.avg_pool3d(f, (3, 13, 17), stride=1, padding=(1, 6, 8), count_include_pad=False)
    f = f.reshape(T_out, ny * nx)
    thr = torch.quantile(f.reshape(-1)[:: 113][: 16_000_000], 1.0 - frac)
    out = (f > thr).to(torch.uint8) * mask.reshape(1, -1)
    del f
    torch.cuda.empty_cache()
    return out


def time_label(xb, K=3):
    ws = {}
    for _ in range(2):
        lab = hot.label_objects_3d(xb, ny, nx, True, wsp=ws)
    hot.sync()
    t0 = time.perf_counter()
    for _ in range(K):
        lab = hot.label_objects_3d(xb, ny, nx, True, wsp=ws)
    hot.sync()
    dt = (time.perf_counter() - t0) / K
    n = int(lab["n"].item())
    areas = lab["areas"][:n]
    big = int(torch.argmax(areas).item()) + 1 if n else 0
    ids = lab["ids"]
    span = int(((ids == big).any(dim=1)).sum().item()) if n else 0
    return {"label3d_ms": round(dt * 1e3, 2), "Gcells_per_s": round(xb.numel() / dt / 1e9, 1), "events": n,
            "largest_frac_of_true": round(float(areas.max().item()) / max(1, float(xb.sum(dtype=torch.int64).item())), 4) if n else 0,
            "largest_spans_steps": span, "true_frac": round(float(xb.float().mean().item()), 4)}


def time_tracker(xb, name):
    """tracker.run() by stage; the second of two runs is reported (the first warms the allocator up)."""
    da = DeviceDataArray(xb.view(T_out, ny, nx), ("time", "lat", "lon"),
                         {"time": np.arange(T_out), "lat": np.linspace(-89.875, 89.875, ny), "lon": np.linspace(0.125, 359.875, nx)})
    for _ in range(2):
        trk = marex_amd.tracker(da, mask_h, R_fill=8, T_fill=2, area_filter_quartile=0.5, allow_merging=False)
        hot.sync()
        t0 = time.perf_counter()
        pre, stats = trk.run_preprocess()
        hot.sync()
        t1 = time.perf_counter()
        events, merges, n = trk.run_tracking(pre)  # labelling + the one D2H copy of ID_field
        t2 = time.perf_counter()
        ds = trk.run_stats_attributes(events, merges, stats, n)
        t3 = time.perf_counter()
        del pre, events, ds
    return {"case": name, "preprocess_ms": round((t1 - t0) * 1e3, 1), "tracking_ms": round((t2 - t1) * 1e3, 1),
            "stats_ms": round((t3 - t2) * 1e3, 1), "total_ms": round((t3 - t0) * 1e3, 1), "N_objects_prefiltered": stats[1],
            "N_objects_filtered": stats[2], "N_events_final": n, "ID_field_GB": round(T_out * ny * nx * 4 / 1e9, 2)}


print({"case": "worst: filled cfg2 extreme mask", **time_label(hot.fill_time_gaps(hot.fill_holes(ext, mask, ny, nx, 8), mask, ny, nx, 8, 2))},
      flush=True)
torch.cuda.empty_cache()
print(time_tracker(ext, "worst: cfg2 extreme mask"), flush=True)
torch.cuda.empty_cache()
b = blobby()
print({"case": "blobby 5 %", **time_label(b)}, flush=True)
print(time_tracker(b, "blobby 5 %"), flush=True)
