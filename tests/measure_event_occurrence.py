"""One-off measurement (not a pytest file): occurrence statistics (``marex_occurrence_i32`` / ``marex_occurrence_u8``) on a
field of the size of cfg2 (``OCC_STEPS`` x ``OCC_NY`` x ``OCC_NX``, default 1826 x 720 x 1440, daily from 2000-01-01): the
int32 event field of the basic tracker on a 5 % mask of smoothed device noise (the blobby mask of tests/measure_track.py),
and the uint8 mask ``ID_field > 0`` of the same field.  Per field:

(k1) the kernel, default outputs (one group, run statistics);
(k2) the kernel with ``by="season"`` and ``zonal=True, zonal_by="month"`` added;
(k3) the kernel with ``by="dayofyear"``: the grouping that flushes the per-cell counter at every row;
(c)  baseline: a ``torch`` device-to-device copy of the same field (reads and writes it: twice the bytes (k1) reads);
(r)  ``marex_amd.event_occurrence`` on the resident field, defaults;
(h)  the same from the host array (block_steps=None: the field is uploaded whole);
(n)  baseline: the NumPy equivalent on the host (``> 0``, a running count, run length, runs begun and longest run per
     step), timed on the first ``OCC_HOST_STEPS`` steps (default 64) and scaled.

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
from marex_amd.zarr_io import DeviceDataArray

REPS = 5
T = int(os.environ.get("OCC_STEPS", 1826))
ny = int(os.environ.get("OCC_NY", 720))
nx = int(os.environ.get("OCC_NX", 1440))
HOST_STEPS = min(T, int(os.environ.get("OCC_HOST_STEPS", 64)))
C = ny * nx
n = T * C
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


mask = blobby()
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
season, G_s, _, _ = mo.group_labels("season", tv, T)
doy, G_d, _, _ = mo.group_labels("dayofyear", tv, T)
month, G_m, _, _ = mo.zonal_labels("month", tv, T)
rows = np.repeat(np.arange(ny, dtype=np.int32), nx)
eng.ctx.timing_enable(True)
CONFIGS = [("k1: default outputs", {}),
           ("k2: by='season', zonal_by='month'", dict(grp=season, G=G_s, sgrp=month, G2=G_m, cls=rows, R=ny)),
           ("k3: by='dayofyear'", dict(grp=doy, G=G_d))]
checks = {}
for fname, x, item in (("int32 ID field", ids, 4), ("uint8 mask", m8, 1)):
    for name, kw in CONFIGS:
        res = {}
        k = kernel_ms(lambda: res.__setitem__("r", eng.occurrence(x, finish=False, **kw)))
        acc = res["r"]["acc"]
        assert acc["status"].cpu().tolist() == [0, 0]
        checks[(fname, name)] = (int(acc["cell_cnt"].sum(dtype=torch.int64).item()),
                                 None if acc["sec_cnt"] is None else int(acc["sec_cnt"].sum().item()))
        assert checks[(fname, name)][0] == held and checks[(fname, name)][1] in (None, held)
        print(json.dumps(dict({"field": fname, "variant": name}, **med(k),
                              GB_per_s_on_the_field=round(item * n / statistics.median(k) / 1e6, 1))), flush=True)
        del res, acc
    dst = torch.empty_like(x)
    cp = []
    for _ in range(REPS + 1):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        eng.sync()
        a.record()
        dst.copy_(x)
        b.record()
        eng.sync()
        cp.append(a.elapsed_time(b))
    cp = cp[1:]
    print(json.dumps(dict({"field": fname, "variant": "c: device-to-device copy (reads and writes the field)"}, **med(cp),
                          GB_per_s_read_plus_written=round(2 * item * n / statistics.median(cp) / 1e6, 1))), flush=True)
    del dst
    torch.cuda.empty_cache()
eng.ctx.timing_enable(False)

# (r), (h) the whole call, defaults
res = {}
for fname, dev, host in (("int32 ID field", ids, ids_h), ("uint8 mask", m8, None)):
    r = wall(lambda: res.__setitem__("r", marex_amd.event_occurrence(dev.view(T, ny, nx))))
    print(json.dumps(dict({"field": fname, "variant": "r: event_occurrence, resident field"}, **med(r))), flush=True)
    if host is None:
        host = dev.cpu().numpy()
    h = wall(lambda: res.__setitem__("h", marex_amd.event_occurrence(host.reshape(T, ny, nx))))
    print(json.dumps(dict({"field": fname, "variant": "h: event_occurrence, host field (uploaded whole)"}, **med(h))), flush=True)
    same = all(np.asarray(res["r"][v].values).tobytes() == np.asarray(res["h"][v].values).tobytes() for v in res["r"].data_vars)
    print(json.dumps({"field": fname, "resident_and_host_results_same_bytes": same}), flush=True)
del m8, ids
torch.cuda.empty_cache()


# (n) NumPy on the host
def numpy_steps(steps):
    occ = np.zeros(C, np.uint32)
    run, nrun, longest = np.zeros(C, np.uint32), np.zeros(C, np.uint32), np.zeros(C, np.uint32)
    for t in range(steps):
        p = ids_h[t] > 0
        occ += p
        nrun += p & (run == 0)
        run = np.where(p, run + 1, 0).astype(np.uint32)
        np.maximum(longest, run, out=longest)
    return occ, nrun, longest


nt = []
for _ in range(3):
    t0 = time.perf_counter()
    got = numpy_steps(HOST_STEPS)
    nt.append((time.perf_counter() - t0) * 1e3)
per = statistics.median(nt[1:]) / HOST_STEPS
print(json.dumps({"variant": "n: NumPy on the host (count and run statistics per step), int32 ID field", "steps_timed": HOST_STEPS,
                  "ms_per_step": round(per, 3), "ms_scaled_to_all_steps": round(per * T, 1)}), flush=True)
