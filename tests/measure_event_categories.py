"""One-off measurement (not a pytest file): severity categories of tracked events (``marex_event_categories_f32``) on the
tracked field of tests/measure_event_intensity.py (``CAT_STEPS`` x ``CAT_NY`` x ``CAT_NX``, default 1826 x 720 x 1440: the
basic tracker's events on a 5 % mask of smoothed device noise), its anomalies, and day-of-year thresholds of 366 rows.

(k) the library call alone, resident inputs, between two device events, without the field;
(f) the same with the one-byte-per-cell field;
(i) the yardstick: ``marex_event_intensity_f32`` on the same IDs and anomalies, in the same run;
(c) baseline: a device-to-device copy of the ID and anomaly fields;
(r) ``marex_amd.event_categories`` on resident inputs: the span passes, the kernel, the host finish;
(h) the same from host arrays (block_steps=None: both fields are uploaded whole);
(n) baseline: the NumPy oracle of tests/event_categories_oracle.py on the host, timed on the first ``CAT_HOST_STEPS`` steps
    (default 16) and scaled.

Wall times are host clocks that end in a synchronise, device times are HIP events; medians of REPS after one warm-up."""
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
from marex_amd.detect import get_engine
from marex_amd.engine import HotPath
from marex_amd.zarr_io import DeviceDataArray

import event_categories_oracle as co

REPS = 5
T = int(os.environ.get("CAT_STEPS", 1826))
ny = int(os.environ.get("CAT_NY", 720))
nx = int(os.environ.get("CAT_NX", 1440))
HOST_STEPS = min(T, int(os.environ.get("CAT_HOST_STEPS", 16)))
C = ny * nx
eng = get_engine(0)
print(json.dumps({"device": torch.cuda.get_device_name(0), "reps": REPS, "T": T, "ny": ny, "nx": nx}), flush=True)


def blobby(frac=0.05, seed=1):
    g = torch.Generator(device=eng.device).manual_seed(seed)
    f = torch.randn((1, 1, T, ny, nx), generator=g, device=eng.device)
    for _ in range(2):  # two box passes ~ a Gaussian of (1, 6, 8) cells
        f = torch.nn.functional.avg_pool3d(f, (3, 13, 17), stride=1, padding=(1, 6, 8), count_include_pad=False)
    f = f.reshape(T, C)
    thr = torch.quantile(f.reshape(-1)[:: 113][: 16_000_000], 1.0 - frac)
    return f > thr


def med(v):
    return {"ms_median": round(statistics.median(v), 3), "ms_min": round(min(v), 3), "ms_max": round(max(v), 3)}


def wall(fn):
    out = []
    for _ in range(REPS + 1):
        eng.sync()
        t0 = time.perf_counter()
        fn()
        eng.sync()
        out.append((time.perf_counter() - t0) * 1e3)
    return out[1:]


def device_ms(fn, zero):
    out = []
    for _ in range(REPS + 1):
        for b in zero:
            b.zero_()
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        eng.sync()
        a.record()
        fn()
        b.record()
        eng.sync()
        out.append(a.elapsed_time(b))
    return out[1:]


mask = blobby()
tv = (np.datetime64("2001-01-01", "D") + np.arange(T)).astype("datetime64[ns]")
da = DeviceDataArray(mask.view(T, ny, nx), ("time", "lat", "lon"),
                     {"time": tv, "lat": np.linspace(-89.875, 89.875, ny), "lon": np.linspace(0.125, 359.875, nx)})
t0 = time.perf_counter()
events = marex_amd.tracker(da, np.ones((ny, nx), bool), R_fill=2, T_fill=2, area_filter_quartile=0.5, allow_merging=False).run()
print(json.dumps({"tracker_run_s": round(time.perf_counter() - t0, 2)}), flush=True)
del mask, da
ids_h = np.ascontiguousarray(np.asarray(events["ID_field"].values).reshape(T, C), dtype=np.int32)
ids = torch.from_numpy(ids_h).to(eng.device)
g = torch.Generator(device=eng.device).manual_seed(2)
anom = torch.randn((T, C), generator=g, device=eng.device) + 1.5
anom_h = anom.cpu().numpy()
thr = 0.5 + torch.rand((366, C), generator=g, device=eng.device)  # 0.5 .. 1.5: every class from below to extreme occurs
thr_h = thr.cpu().numpy()
doy = (marex_amd.calendar._to_year_doy(tv)[1].astype(np.int32) - 1)
n = T * C
held = int((ids > 0).sum().item())
N = int(ids.max().item())
print(json.dumps({"events": N, "cells_with_an_event": held, "coverage": round(held / n, 4)}), flush=True)

sp = eng.id_spans(ids)
tmin, tmax = sp[0].astype(np.int64), sp[1].astype(np.int64)
off = HotPath.event_slot_plan(tmin, tmax)
slots = max(int(off[-1]), 1)
tm_d, off_d, doy_d = eng._dev(np.clip(tmin, 0, 2**31 - 1).astype(np.int32)), eng._dev(off), eng._dev(doy)
cat = torch.zeros((slots, 7), dtype=torch.int64, device=eng.device)
status = torch.zeros(2, dtype=torch.int64, device=eng.device)
field = torch.empty((T, C), dtype=torch.uint8, device=eng.device)


def categories(f):
    eng.call("marex_event_categories_f32", ids, anom, 0, T, C, N, tm_d, off_d, slots, thr, doy_d, 366, None, cat, None, f, status)


k = device_ms(lambda: categories(None), (cat, status))
assert status.cpu().tolist() == [0, 0]
totals = cat.sum(dim=0).cpu().tolist()
print(json.dumps(dict({"variant": "k: library call alone, no field (device events)", "slots": slots, "cells_per_class": totals},
                      **med(k))), flush=True)
f = device_ms(lambda: categories(field), (cat, status))
assert cat.sum(dim=0).cpu().tolist() == totals
assert [int((field == v).sum().item()) for v in range(1, 8)] == totals  # the histogram of the field is the counts
print(json.dumps(dict({"variant": "f: library call alone, with the field"}, **med(f))), flush=True)
del field
cnt = torch.zeros((slots, 2), dtype=torch.int64, device=eng.device)
sums = torch.zeros((slots, 2), dtype=torch.float64, device=eng.device)
vmax = torch.zeros(slots, dtype=torch.int32, device=eng.device)
st1 = torch.zeros(1, dtype=torch.int64, device=eng.device)
i = device_ms(lambda: eng.call("marex_event_intensity_f32", ids, anom, 0, T, C, N, tm_d, off_d, slots, None, cnt, sums, vmax, st1),
              (cnt, sums, vmax, st1))
mi = statistics.median(i)
print(json.dumps(dict({"variant": "i: marex_event_intensity_f32 on the same field (the yardstick)"}, **med(i),
                      k_over_i=round(statistics.median(k) / mi, 3), f_over_i=round(statistics.median(f) / mi, 3))), flush=True)
assert int(cnt.sum().item()) == sum(totals)
del cnt, sums, vmax

dst_i, dst_a = torch.empty_like(ids), torch.empty_like(anom)


def copy():
    dst_i.copy_(ids)
    dst_a.copy_(anom)


cp = device_ms(copy, ())
print(json.dumps(dict({"variant": "c: device-to-device copy of both fields (reads 8, writes 8 bytes per cell)"}, **med(cp),
                      GB_per_s_read_plus_written=round(16 * n / statistics.median(cp) / 1e6, 1))), flush=True)
del dst_i, dst_a
torch.cuda.empty_cache()

res = {}
dims = ("time", "lat", "lon")
tc = {"time": ("time", tv)}
r_i = marex_amd.DataArray(ids.view(T, ny, nx), dims=dims, coords=tc)
r_a = marex_amd.DataArray(anom.view(T, ny, nx), dims=dims)
r_t = thr.view(366, ny, nx)
r = wall(lambda: res.__setitem__("r", marex_amd.event_categories(r_i, r_a, r_t)))
print(json.dumps(dict({"variant": "r: event_categories, resident inputs"}, **med(r))), flush=True)
h_i = marex_amd.DataArray(ids_h.reshape(T, ny, nx), dims=dims, coords=tc)
h_a = marex_amd.DataArray(anom_h.reshape(T, ny, nx), dims=dims)
h = wall(lambda: res.__setitem__("h", marex_amd.event_categories(h_i, h_a, thr_h.reshape(366, ny, nx))))
print(json.dumps(dict({"variant": "h: event_categories, host inputs (uploads 8 bytes per cell and the thresholds)"}, **med(h))),
      flush=True)
same = all(np.asarray(res["r"][v].values).tobytes() == np.asarray(res["h"][v].values).tobytes() for v in res["r"].data_vars)
print(json.dumps({"resident_and_host_results_same_bytes": same,
                  "events_per_category": np.bincount(np.asarray(res["r"]["event_category"].values), minlength=5).tolist()}), flush=True)

nt = []
for _ in range(2):
    t0 = time.perf_counter()
    co.categories(ids_h[:HOST_STEPS], anom_h[:HOST_STEPS], thr_h, doy[:HOST_STEPS], None, N)
    nt.append((time.perf_counter() - t0) * 1e3)
per = nt[1] / HOST_STEPS
print(json.dumps({"variant": "n: the NumPy oracle on the host", "steps_timed": HOST_STEPS, "ms_per_step": round(per, 3),
                  "ms_scaled_to_all_steps": round(per * T, 1), "k_over_n": round(statistics.median(k) / (per * T), 6),
                  "h_over_n": round(statistics.median(h) / (per * T), 6)}), flush=True)
