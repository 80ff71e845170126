"""One-off measurement (not a pytest file): accumulated heat stress (``marex_heat_stress_f32``, ``marex_group_mean_f32``) on a
synthetic SST of the size of cfg2 (``HS_STEPS`` x ``HS_NY`` x ``HS_NX``, default 1826 x 720 x 1440, daily from 2000-01-01,
degrees Celsius: a per-cell mean, an annual cycle and device noise; every third column of cells is land, NaN).
``window=84, steps_per_week=7, hotspot_min=1, levels=(4, 8)``:

(k0) the kernel, summary only;  (k1) with ``dhw`` written;  (k2) with ``dhw`` and ``alert_level`` written;
(k3) summary only under ``by="year"`` labels;  (k4) fields only, the build without accumulators;
(w)  (k0) at windows of 1, 7, 84, 183 and 366 steps: the lagging second read is the row just read at 1 and reaches back
     over 0.03, 0.35, 0.76 and 1.5 GB of field at the others, below and above the 256 MiB of the Infinity Cache;
(g)  the climatology kernel, all steps labelled by their month;
(c1) baseline: a ``torch`` device-to-device copy of the field -- what (k0) reads once, read and written;
(c2) the same plus a copy of a second float32 field, the ``dhw`` output (k1) writes;
(t)  the torch composition the kernel replaces, from the resident field: the thresholded HotSpots in float64, their
     ``cumsum`` along time, the difference of the sums ``window`` steps apart, divided and rounded -- and its peak memory;
(r)  ``marex_amd.heat_stress`` with a given ``mmm`` (``by="year"``; with both fields returned) and with the climatology
     of the first four years, and ``marex_amd.monthly_maximum_climatology``, on the resident field;
(h)  the first and the third of those from a host array (block_steps=None: uploaded whole);
(n)  baseline: the NumPy row loop of tests/heat_stress_oracle.py on the host over the first ``HS_HOST_CELLS`` cells (default
     4096), all steps, scaled to all cells.

Kernel times are the engine's launch timer (HIP events around the launch inside the library), the copies are timed between
two device events, wall times are host clocks that end in a synchronise; medians of REPS after one warm-up.
``HS_ONLY_KERNEL=1`` runs (k0) alone, for a counters run of its own."""
import json
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import numpy as np
import torch

import heat_stress_oracle as ho
import marex_amd
from marex_amd.detect import get_engine
from marex_amd.xr_compat import DataArray

REPS = 5
T = int(os.environ.get("HS_STEPS", 1826))
ny = int(os.environ.get("HS_NY", 720))
nx = int(os.environ.get("HS_NX", 1440))
HOST_CELLS = int(os.environ.get("HS_HOST_CELLS", 4096))
ONLY_KERNEL = bool(int(os.environ.get("HS_ONLY_KERNEL", "0")))
C = ny * nx
n = T * C
W = 84
eng = get_engine(0)
print(json.dumps({"device": torch.cuda.get_device_name(0), "reps": REPS, "T": T, "ny": ny, "nx": nx}), flush=True)


def synthetic():
    """``(x float32 [T, C], m float32 [C])``: SST in degrees Celsius and a threshold 1.3 K above the cell's mean."""
    g = torch.Generator(device=eng.device).manual_seed(1)
    mean = 18.0 + 11.0 * torch.rand(C, generator=g, device=eng.device)
    day = torch.arange(T, device=eng.device, dtype=torch.float32)
    x = torch.randn((T, C), generator=g, device=eng.device) * 0.9
    x += (2.0 * torch.sin(day * (2.0 * np.pi / 365.25)))[:, None]
    x += mean[None, :]
    x[:, 2::3] = float("nan")
    m = (mean + 1.3).to(torch.float32)
    m[2::3] = float("nan")
    return x, m


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


def copy_ms(pairs):
    out = []
    for _ in range(REPS + 1):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        eng.sync()
        a.record()
        for dst, src in pairs:
            dst.copy_(src)
        b.record()
        eng.sync()
        out.append(a.elapsed_time(b))
    return out[1:]


x, m = synthetic()
tv = (np.datetime64("2000-01-01") + np.arange(T)).astype("datetime64[ns]")
year = (tv.astype("datetime64[Y]").astype(int) - 30).astype(np.int32)
G = int(year.max()) + 1
month = (tv.astype("datetime64[M]").astype(int) % 12).astype(np.int32)
eng.ctx.timing_enable(True)
if ONLY_KERNEL:
    k = kernel_ms(lambda: eng.heat_stress(x, m, window=W, finish=False))
    print(json.dumps(dict({"variant": "k0: summary only"}, **med(k))), flush=True)
    sys.exit(0)

dhw = torch.empty((T, C), dtype=torch.float32, device=eng.device)
alert = torch.empty((T, C), dtype=torch.uint8, device=eng.device)
res = {}
for name, kw, item in (("k0: summary only", {}, 4), ("k1: summary and dhw", dict(dhw=dhw), 8),
                       ("k2: summary, dhw and alert_level", dict(dhw=dhw, alert=alert), 9),
                       ("k3: summary only, by='year'", dict(grp=year, G=G), 4),
                       ("k4: dhw and alert_level, no accumulators", dict(dhw=dhw, alert=alert, summary=False), 9)):
    k = kernel_ms(lambda: res.__setitem__("r", eng.heat_stress(x, m, window=W, finish=False, **kw)))
    print(json.dumps(dict({"variant": name}, **med(k), GB_per_s_on_field_once_plus_outputs=round(item * n / statistics.median(k) / 1e6, 1))),
          flush=True)
r = eng.heat_stress(x, m, window=W, dhw=dhw, alert=alert)
print(json.dumps({"steps_per_alert_class": r["alert_steps"].sum(axis=(0, 2), dtype=np.int64).tolist(),
                  "invalid_steps": int(r["invalid"].sum(dtype=np.int64)), "dhw_max": float(np.nanmax(r["dhw_max"]))}), flush=True)
for w in (1, 7, 84, 183, 366):
    k = kernel_ms(lambda: eng.heat_stress(x, m, window=w, finish=False))
    print(json.dumps(dict({"variant": f"w: summary only, window={w}", "history_GB": round(w * C * 4 / 1e9, 3)}, **med(k))), flush=True)
k = kernel_ms(lambda: eng.group_mean(x, month, 12, finish=False))
print(json.dumps(dict({"variant": "g: the climatology kernel, 12 months"}, **med(k), GB_per_s_on_field=round(4 * n / statistics.median(k) / 1e6, 1))),
      flush=True)
eng.ctx.timing_enable(False)
x2 = torch.empty_like(x)
cp = copy_ms([(x2, x)])
print(json.dumps(dict({"variant": "c1: device-to-device copy of the field"}, **med(cp),
                      GB_per_s_read_plus_written=round(2 * 4 * n / statistics.median(cp) / 1e6, 1))), flush=True)
cp = copy_ms([(x2, x), (dhw, x)])
print(json.dumps(dict({"variant": "c2: the same and a second float32 field"}, **med(cp),
                      GB_per_s_read_plus_written=round(2 * 8 * n / statistics.median(cp) / 1e6, 1))), flush=True)
del x2
torch.cuda.empty_cache()


# (t) the torch composition from the resident field
def torch_dhw():
    d = x - m[None, :]
    h = torch.where(torch.isfinite(d) & (d.abs() < 1024) & (d >= 1.0), d, torch.zeros((), device=x.device)).to(torch.float64)
    del d
    cs = torch.cumsum(h, dim=0)
    del h
    cs[W:] -= cs[:-W].clone()
    return torch.where(torch.isfinite(m)[None, :], (cs / 7.0).to(torch.float32), torch.full((), float("nan"), device=x.device))


torch.cuda.reset_peak_memory_stats()
base = torch.cuda.memory_allocated()
tt = wall(lambda: res.__setitem__("t", torch_dhw()), reps=3)
peak = torch.cuda.max_memory_allocated() - base
same = bool(torch.equal(torch.nan_to_num(res["t"], nan=-1.0), torch.nan_to_num(dhw, nan=-1.0)))
print(json.dumps(dict({"variant": "t: torch composition of dhw (float64 cumsum difference), resident field"}, **med(tt),
                      peak_GB_beyond_the_field=round(peak / 1e9, 2), equals_the_kernel=same)), flush=True)
del res, dhw, alert
torch.cuda.empty_cache()

# (r), (h) the whole call
coords = {"time": ("time", tv)}
dims = ("time", "lat", "lon")
out = {}
m2 = m.view(ny, nx)
CALLS = (("mmm given, by='year'", lambda f: marex_amd.heat_stress(f, m2, by="year")),
         ("mmm given, by='year', return_dhw and return_alert", lambda f: marex_amd.heat_stress(f, m2, by="year", return_dhw=True, return_alert=True)),
         ("mmm of 2000..2003, by='year'", lambda f: marex_amd.heat_stress(f, baseline=(2000, 2003), by="year")),
         ("monthly_maximum_climatology, all years", lambda f: marex_amd.monthly_maximum_climatology(f)))
for name, fn in CALLS:
    rr = wall(lambda: out.__setitem__(("r", name), fn(DataArray(x.view(T, ny, nx), dims=dims, coords=coords))), reps=3)
    print(json.dumps(dict({"variant": f"r: {name}, resident field"}, **med(rr))), flush=True)
x_h = x.cpu().numpy().reshape(T, ny, nx)
m_h = m.cpu().numpy()
del x
torch.cuda.empty_cache()
for name, fn in (CALLS[0], CALLS[2]):
    hh = wall(lambda: out.__setitem__(("h", name), fn(DataArray(x_h, dims=dims, coords=coords))), reps=2)
    print(json.dumps(dict({"variant": f"h: {name}, host array (uploaded whole)"}, **med(hh))), flush=True)
    a, b = out[("r", name)], out[("h", name)]
    same = all(np.asarray(v.values).tobytes() == np.asarray(b[k].values).tobytes() for k, v in a.data_vars.items())
    print(json.dumps({"variant": name, "resident_and_host_results_same_bytes": same}), flush=True)
del out

# (n) NumPy on the host: the row loop, vectorised over the cells
xs, ms_ = np.ascontiguousarray(x_h.reshape(T, C)[:, :HOST_CELLS]), m_h[:HOST_CELLS]
nt = []
for _ in range(2):
    t0 = time.perf_counter()
    ho.walk(xs, ms_, window=W, grp=year, G=G)
    nt.append((time.perf_counter() - t0) * 1e3)
print(json.dumps({"variant": "n: NumPy row loop on the host, by='year', no fields", "cells_timed": HOST_CELLS,
                  "ms": round(min(nt), 1), "ms_scaled_to_all_cells": round(min(nt) * C / HOST_CELLS, 1)}), flush=True)
