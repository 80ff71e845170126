"""One-off measurement (not a pytest file): per-cell intensity (``marex_local_intensity_i32`` / ``marex_local_intensity_u8``)
on a field of the size of cfg2 (``LI_STEPS`` x ``LI_NY`` x ``LI_NX``, default 1826 x 720 x 1440, daily from 2000-01-01): the
int32 event field of the basic tracker on a 5 % mask of smoothed device noise (the field of tests/measure_event_occurrence.py)
and the uint8 mask ``ID_field > 0`` of it, joined with the smoothed noise itself as the anomaly field (scaled so that the
mask is ``anomaly > 1``) and day-of-year thresholds around 1.  Per presence field:

(k1) the kernel without categories (one group);
(k2) the kernel with categories;
(k3) the kernel with categories, ``by="year"`` and monthly zonal sections;
(c)  baseline: a ``torch`` device-to-device copy of the presence field plus the anomaly field -- the bytes a dense read
     would move, read and written;
(r)  ``marex_amd.local_intensity(thresholds, by="year", zonal=True)`` on resident inputs (uint8 mask);
(h)  the same from host arrays (block_steps=None: uploaded whole);
(n)  baseline: the NumPy row loop on the host (days, invalid, float64 sum, maximum and its step, the category compares),
     timed on the first ``LI_HOST_STEPS`` steps (default 32) and scaled.

Kernel times are the engine's launch timer (HIP events around the launch inside the library), the copy is timed between
two device events, wall times are host clocks that end in a synchronise; medians of REPS after one warm-up."""
import json
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch

import marex_amd
import marex_amd.occurrence as mo
from marex_amd.detect import get_engine
from marex_amd.xr_compat import DataArray
from marex_amd.zarr_io import DeviceDataArray

REPS = 5
T = int(os.environ.get("LI_STEPS", 1826))
ny = int(os.environ.get("LI_NY", 720))
nx = int(os.environ.get("LI_NX", 1440))
HOST_STEPS = min(T, int(os.environ.get("LI_HOST_STEPS", 32)))
C = ny * nx
n = T * C
eng = get_engine(0)
print(json.dumps({"device": torch.cuda.get_device_name(0), "reps": REPS, "T": T, "ny": ny, "nx": nx}), flush=True)


def blobby(frac=0.05, seed=1):
    """Smoothed noise scaled so that its upper ``frac`` lies above 1, and that mask."""
    g = torch.Generator(device=eng.device).manual_seed(seed)
    f = torch.randn((1, 1, T, ny, nx), generator=g, device=eng.device)
    for _ in range(2):  # two box passes ~ a Gaussian of (1, 6, 8) cells
        f = torch.nn.functional.avg_pool3d(f, (3, 13, 17), stride=1, padding=(1, 6, 8), count_include_pad=False)
    f = f.reshape(T, C)
    thr = torch.quantile(f.reshape(-1)[:: 113][: 16_000_000], 1.0 - frac)
    f /= thr
    return f, f > 1.0


def med(v):
    return {"ms_median": round(statistics.median(v), 3), "ms_min": round(min(v), 3), "ms_max": round(max(v), 3)}


def wall(fn, reps=REPS):
    out = []
    for _ in range(reps + 1):
        eng.sync()
        t0 = time.perf_counter()
        fn()
        eng.sync()
        out.append((time.perf_counter() - t0) * 1e3)
    return out[1:]


def kernel_ms(fn):
    """Milliseconds the library's launch timer saw per call of ``fn``."""
    out = []
    for _ in range(REPS + 1):
        eng.sync()
        eng.ctx.timing_reset()
        fn()
        eng.sync()
        out.append(eng.ctx.timing_get("morph")[0])
    return out[1:]


anom, mask = blobby()
da = DeviceDataArray(mask.view(T, ny, nx), ("time", "lat", "lon"),
                     {"time": np.arange(T), "lat": np.linspace(-89.875, 89.875, ny), "lon": np.linspace(0.125, 359.875, nx)})
t0 = time.perf_counter()
events = marex_amd.tracker(da, np.ones((ny, nx), bool), R_fill=2, T_fill=2, area_filter_quartile=0.5, allow_merging=False).run()
print(json.dumps({"tracker_run_s": round(time.perf_counter() - t0, 2)}), flush=True)
del mask, da
ids_h = np.ascontiguousarray(np.asarray(events["ID_field"].values).reshape(T, C), dtype=np.int32)
del events
ids = torch.from_numpy(ids_h).to(eng.device)
m8 = (ids > 0).to(torch.uint8)
held = int(m8.sum(dtype=torch.int64).item())
print(json.dumps({"events": int(ids.max().item()), "cells_present": held, "coverage": round(held / n, 4)}), flush=True)

tv = (np.datetime64("2000-01-01") + np.arange(T)).astype("datetime64[ns]")
year, G_y, _, _ = mo.group_labels("year", tv, T)
month, G_m, _, _ = mo.zonal_labels("month", tv, T)
doy = (mo._calendar(tv, "measure")[2] - 1).astype(np.int32)
rows = np.repeat(np.arange(ny, dtype=np.int32), nx)
g = torch.Generator(device=eng.device).manual_seed(2)
thr = 1.0 + 0.1 * torch.rand((366, C), generator=g, device=eng.device)  # day-of-year-major float32
eng.ctx.timing_enable(True)
CONFIGS = [("k1: no categories", {}),
           ("k2: categories", dict(thr=thr, doy=doy)),
           ("k3: categories, by='year', zonal_by='month'", dict(thr=thr, doy=doy, grp=year, G=G_y, sgrp=month, G2=G_m, cls=rows, R=ny))]
for fname, x, item in (("int32 ID field", ids, 4), ("uint8 mask", m8, 1)):
    for name, kw in CONFIGS:
        res = {}
        k = kernel_ms(lambda: res.__setitem__("r", eng.local_intensity(x, anom, finish=False, **kw)))
        acc = res["r"]["acc"]
        assert acc["status"].cpu().tolist() == [0, 0]
        seen = int(acc["days"].sum(dtype=torch.int64).item()) + int(acc["invalid"].sum(dtype=torch.int64).item())
        assert seen == held and (acc["cat_days"] is None or int(acc["cat_days"].sum(dtype=torch.int64).item()) == held)
        assert acc["sec_cnt"] is None or int(acc["sec_cnt"].sum().item()) == held
        cats = None if acc["cat_days"] is None else acc["cat_days"].sum(dim=(0, 2), dtype=torch.int64).cpu().tolist()
        print(json.dumps(dict({"field": fname, "variant": name}, **med(k), category_days=cats,
                              GB_per_s_on_presence_plus_anomalies=round((item + 4) * n / statistics.median(k) / 1e6, 1))), flush=True)
        del res, acc
        torch.cuda.empty_cache()
    dx, da_ = torch.empty_like(x), torch.empty_like(anom)
    cp = []
    for _ in range(REPS + 1):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        eng.sync()
        a.record()
        dx.copy_(x)
        da_.copy_(anom)
        b.record()
        eng.sync()
        cp.append(a.elapsed_time(b))
    cp = cp[1:]
    print(json.dumps(dict({"field": fname, "variant": "c: device-to-device copy of the presence field and the anomalies"}, **med(cp),
                          GB_per_s_read_plus_written=round(2 * (item + 4) * n / statistics.median(cp) / 1e6, 1))), flush=True)
    del dx, da_
    torch.cuda.empty_cache()
eng.ctx.timing_enable(False)
del ids

# (r), (h) the whole call: thresholds, annual maps, monthly zonal category counts
coords = {"time": ("time", tv)}
dims = ("time", "lat", "lon")
thr_da = DataArray(thr.view(366, ny, nx), dims=("dayofyear", "lat", "lon"))
res = {}
kw = dict(by="year", zonal=True)
r = wall(lambda: res.__setitem__("r", marex_amd.local_intensity(DataArray(m8.view(T, ny, nx), dims=dims, coords=coords),
                                                                 DataArray(anom.view(T, ny, nx), dims=dims, coords=coords), thr_da, **kw)))
print(json.dumps(dict({"field": "uint8 mask", "variant": "r: local_intensity(by='year', zonal=True), resident inputs"}, **med(r))), flush=True)
m8_h, anom_h, thr_h = m8.cpu().numpy().reshape(T, ny, nx), anom.cpu().numpy().reshape(T, ny, nx), thr.cpu().numpy().reshape(366, ny, nx)
del m8, anom, thr, thr_da
torch.cuda.empty_cache()
h = wall(lambda: res.__setitem__("h", marex_amd.local_intensity(DataArray(m8_h, dims=dims, coords=coords), DataArray(anom_h, dims=dims, coords=coords),
                                                                 DataArray(thr_h, dims=("dayofyear", "lat", "lon")), **kw)), reps=3)
print(json.dumps(dict({"field": "uint8 mask", "variant": "h: the same from host arrays (uploaded whole)"}, **med(h))), flush=True)
same = all(np.asarray(res["r"][v].values).tobytes() == np.asarray(res["h"][v].values).tobytes() for v in res["r"].data_vars)
print(json.dumps({"resident_and_host_results_same_bytes": same}), flush=True)


# (n) NumPy on the host: the row loop, vectorised over the cells
def numpy_steps(steps):
    days, inv = np.zeros(C, np.uint32), np.zeros(C, np.uint32)
    s, vmax, tmax = np.zeros(C), np.full(C, -np.inf, np.float32), np.full(C, -1, np.int32)
    cat = np.zeros((6, C), np.uint32)
    a3, m3, h3 = anom_h.reshape(T, C), m8_h.reshape(T, C), thr_h.reshape(366, C)
    for t in range(steps):
        a, hh = a3[t], h3[doy[t]]
        ok = (m3[t] > 0) & np.isfinite(a)
        days += ok
        inv += (m3[t] > 0) & ~ok
        s += np.where(ok, a.astype(np.float64), 0.0)
        better = ok & (a > vmax)
        vmax = np.where(better, a, vmax)
        tmax = np.where(better, np.int32(t), tmax)
        k = (a >= hh).astype(np.int8) + (a >= np.float32(2) * hh) + (a >= np.float32(3) * hh) + (a >= np.float32(4) * hh)
        k = np.where(np.isfinite(hh) & (hh > 0), k, 5)
        for q in range(6):
            cat[q] += ok & (k == q)
    return days, inv, s, vmax, tmax, cat


nt = []
for _ in range(3):
    t0 = time.perf_counter()
    got = numpy_steps(HOST_STEPS)
    nt.append((time.perf_counter() - t0) * 1e3)
per = statistics.median(nt[1:]) / HOST_STEPS
print(json.dumps({"variant": "n: NumPy row loop on the host (sums, maximum, categories per step), uint8 mask", "steps_timed": HOST_STEPS,
                  "ms_per_step": round(per, 3), "ms_scaled_to_all_steps": round(per * T, 1)}), flush=True)
