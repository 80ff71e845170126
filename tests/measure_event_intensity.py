"""One-off measurement (not a pytest file): per-event intensity (``marex_event_intensity_f32``) on a tracked field of the
size of cfg2 (``INT_STEPS`` x ``INT_NY`` x ``INT_NX``, default 1826 x 720 x 1440).  The event field comes from the basic
tracker itself on a 5 % mask of smoothed device noise (the blobby mask of tests/measure_track.py), so the coverage and the
shape of the events are those of a tracked field; the coverage is reported.

(k) the library call alone, resident inputs, between two device events;
(r) ``marex_amd.event_intensity`` on resident inputs: the span passes, the kernel, the host finish;
(h) the same from host arrays (block_steps=None: both fields are uploaded whole);
(z) control for the predicated anomaly loads: the library call on an all-background ID field (4 bytes per cell are read);
(c) baseline: a device-to-device copy of the two fields;
(n) baseline: the vectorised NumPy equivalent on the host, ``np.bincount`` per step for the counts and the sums and a
    sorted ``np.maximum.reduceat`` for the maximum, timed on the first ``INT_HOST_STEPS`` steps (default 64) and scaled.

Wall times are host clocks that end in a synchronise, device times are HIP events; medians of REPS after one warm-up.
Rates: on 8 bytes per cell (both fields), and on 4 bytes per cell plus the 128-byte anomaly lines that hold an event cell."""
import json
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch

import marex_amd
from marex_amd.detect import get_engine
from marex_amd.engine import HotPath
from marex_amd.zarr_io import DeviceDataArray

REPS = 5
T = int(os.environ.get("INT_STEPS", 1826))
ny = int(os.environ.get("INT_NY", 720))
nx = int(os.environ.get("INT_NX", 1440))
HOST_STEPS = min(T, int(os.environ.get("INT_HOST_STEPS", 64)))
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


mask = blobby()
da = DeviceDataArray(mask.view(T, ny, nx), ("time", "lat", "lon"),
                     {"time": np.arange(T), "lat": np.linspace(-89.875, 89.875, ny), "lon": np.linspace(0.125, 359.875, nx)})
t0 = time.perf_counter()
events = marex_amd.tracker(da, np.ones((ny, nx), bool), R_fill=2, T_fill=2, area_filter_quartile=0.5, allow_merging=False).run()
print(json.dumps({"tracker_run_s": round(time.perf_counter() - t0, 2)}), flush=True)
del mask, da
ids_h = np.ascontiguousarray(np.asarray(events["ID_field"].values).reshape(T, C), dtype=np.int32)
ids = torch.from_numpy(ids_h).to(eng.device)
g = torch.Generator(device=eng.device).manual_seed(2)
anom = torch.randn((T, C), generator=g, device=eng.device) + 1.5
anom_h = anom.cpu().numpy()
n = T * C
held = int((ids > 0).sum().item())
lines = int((ids > 0).view(T, C // 32, 32).any(dim=2).sum().item()) if C % 32 == 0 else None
N = int(ids.max().item())
print(json.dumps({"events": N, "cells_with_an_event": held, "coverage": round(held / n, 4),
                  "anomaly_lines_with_an_event": lines, "share_of_lines": None if lines is None else round(lines / (n / 32), 4)}),
      flush=True)
bytes8 = 8 * n
bytes_min = None if lines is None else 4 * n + 128 * lines

# (k) the library call alone
sp = eng.id_spans(ids)
tmin, tmax = sp[0].astype(np.int64), sp[1].astype(np.int64)
off = HotPath.event_slot_plan(tmin, tmax)
slots = max(int(off[-1]), 1)
tm_d, off_d = eng._dev(np.clip(tmin, 0, 2**31 - 1).astype(np.int32)), eng._dev(off)
cnt = torch.zeros((slots, 2), dtype=torch.int64, device=eng.device)
sums = torch.zeros((slots, 2), dtype=torch.float64, device=eng.device)
vmax = torch.zeros(slots, dtype=torch.int32, device=eng.device)
status = torch.zeros(1, dtype=torch.int64, device=eng.device)


def device_ms(field):
    out = []
    for _ in range(REPS + 1):
        for b in (cnt, sums, vmax, status):
            b.zero_()
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        eng.sync()
        a.record()
        eng.call("marex_event_intensity_f32", field, anom, 0, T, C, N, tm_d, off_d, slots, None, cnt, sums, vmax, status)
        b.record()
        eng.sync()
        out.append(a.elapsed_time(b))
    return out[1:]


def rates(ms):
    r = {"GB_per_s_on_8_bytes_per_cell": round(bytes8 / ms / 1e6, 1)}
    if bytes_min is not None:
        r["GB_per_s_on_4_bytes_per_cell_plus_event_lines"] = round(bytes_min / ms / 1e6, 1)
    return r


k = device_ms(ids)
assert int(status.item()) == 0
print(json.dumps(dict({"variant": "k: library call alone (device events)", "slots": slots}, **med(k), **rates(statistics.median(k)))),
      flush=True)
zero = torch.zeros_like(ids)
z = device_ms(zero)
print(json.dumps(dict({"variant": "z: library call, all-background IDs (reads 4 bytes per cell)"}, **med(z),
                      GB_per_s_on_4_bytes_per_cell=round(4 * n / statistics.median(z) / 1e6, 1))), flush=True)
del zero

# (c) device-to-device copy of the two fields
dst_i, dst_a = torch.empty_like(ids), torch.empty_like(anom)
cp = []
for _ in range(REPS + 1):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    eng.sync()
    a.record()
    dst_i.copy_(ids)
    dst_a.copy_(anom)
    b.record()
    eng.sync()
    cp.append(a.elapsed_time(b))
cp = cp[1:]
print(json.dumps(dict({"variant": "c: device-to-device copy of both fields (reads 8, writes 8 bytes per cell)"}, **med(cp),
                      GB_per_s_read_plus_written=round(2 * bytes8 / statistics.median(cp) / 1e6, 1))), flush=True)
del dst_i, dst_a
torch.cuda.empty_cache()

# (r), (h) the whole call
res = {}
r = wall(lambda: res.__setitem__("r", marex_amd.event_intensity(ids, anom)))
print(json.dumps(dict({"variant": "r: event_intensity, resident inputs"}, **med(r), **rates(statistics.median(r)))), flush=True)
h = wall(lambda: res.__setitem__("h", marex_amd.event_intensity(ids_h, anom_h)))
print(json.dumps(dict({"variant": "h: event_intensity, host inputs (uploads 8 bytes per cell)"}, **med(h),
                      **rates(statistics.median(h)))), flush=True)
same = all(np.asarray(res["r"][v].values).tobytes() == np.asarray(res["h"][v].values).tobytes() for v in res["r"].data_vars)
print(json.dumps({"resident_and_host_results_same_bytes": same}), flush=True)


# (n) NumPy on the host
def numpy_steps(steps):
    out = []
    for t in range(steps):
        i, a = ids_h[t], anom_h[t]
        sel = np.nonzero(i)[0]
        e, v = i[sel], a[sel]
        ok = np.isfinite(v)
        c = np.bincount(e[ok], minlength=N + 1)
        s = np.bincount(e[ok], weights=v[ok].astype(np.float64), minlength=N + 1)
        o = np.argsort(e[ok], kind="stable")
        es, vs = e[ok][o], v[ok][o]
        first = np.nonzero(np.diff(es, prepend=-1))[0]
        m = np.maximum.reduceat(vs, first) if first.size else vs[:0]
        out.append((c, s, es[first], m))
    return out


nt = []
for _ in range(3):
    t0 = time.perf_counter()
    numpy_steps(HOST_STEPS)
    nt.append((time.perf_counter() - t0) * 1e3)
per = statistics.median(nt[1:]) / HOST_STEPS
print(json.dumps({"variant": "n: NumPy on the host (bincount per step)", "steps_timed": HOST_STEPS, "ms_per_step": round(per, 3),
                  "ms_scaled_to_all_steps": round(per * T, 1), "k_over_n": round(statistics.median(k) / (per * T), 5),
                  "h_over_n": round(statistics.median(h) / (per * T), 5)}), flush=True)
