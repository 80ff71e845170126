"""One-off measurement (not a pytest file): per-cell Hobday events (``marex_cell_events_u8``) on a field of the size of cfg2
(``CE_STEPS`` x ``CE_NY`` x ``CE_NX``, default 1826 x 720 x 1440, daily from 2000-01-01): the uint8 mask ``ID_field > 0`` of
the basic tracker's result on a 5 % mask of smoothed device noise (the field of tests/measure_local_intensity.py), joined
with the smoothed noise itself as the anomaly field.  ``min_duration=5, max_gap=2``:

(k0) the kernel without anomalies, summary only;
(k1) the kernel with anomalies, summary only;
(k2) the same with the filtered mask written;
(k3) the second pass, which writes the records;
(c1) baseline: a ``torch`` device-to-device copy of the mask and the anomalies -- the bytes (k1) and (k3) would move if they
     read densely, read and written;  (c2) the same plus a copy of one more uint8 field, the mask (k2) writes;
(li) ``marex_local_intensity_u8`` without categories on the same field in the same run;
(r)  ``marex_amd.cell_events(by="year")`` and ``(return_mask=True, records=True)`` on resident inputs;
(h)  the same from host arrays (block_steps=None: uploaded whole, twice with records);
(n)  baseline: the NumPy row loop of tests/cell_events_oracle.py on the host, timed on the first ``CE_HOST_STEPS`` steps
     (default 32) and scaled.

Kernel times are the engine's launch timer (HIP events around the launch inside the library), the copies are timed between
two device events, wall times are host clocks that end in a synchronise; medians of REPS after one warm-up."""
import json
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import numpy as np
import torch

import cell_events_oracle as co
import marex_amd
from marex_amd.detect import get_engine
from marex_amd.xr_compat import DataArray
from marex_amd.zarr_io import DeviceDataArray

REPS = 5
T = int(os.environ.get("CE_STEPS", 1826))
ny = int(os.environ.get("CE_NY", 720))
nx = int(os.environ.get("CE_NX", 1440))
HOST_STEPS = min(T, int(os.environ.get("CE_HOST_STEPS", 32)))
C = ny * nx
n = T * C
D, GAP = 5, 2
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


anom, mask = blobby()
da = DeviceDataArray(mask.view(T, ny, nx), ("time", "lat", "lon"),
                     {"time": np.arange(T), "lat": np.linspace(-89.875, 89.875, ny), "lon": np.linspace(0.125, 359.875, nx)})
t0 = time.perf_counter()
events = marex_amd.tracker(da, np.ones((ny, nx), bool), R_fill=2, T_fill=2, area_filter_quartile=0.5, allow_merging=False).run()
print(json.dumps({"tracker_run_s": round(time.perf_counter() - t0, 2)}), flush=True)
del mask, da
m8 = torch.from_numpy(np.ascontiguousarray(np.asarray(events["ID_field"].values).reshape(T, C) > 0).view(np.uint8)).to(eng.device)
del events
held = int(m8.sum(dtype=torch.int64).item())
print(json.dumps({"cells_present": held, "coverage": round(held / n, 4)}), flush=True)

eng.ctx.timing_enable(True)
hob = torch.empty((T, C), dtype=torch.uint8, device=eng.device)
res = {}
for name, kw in (("k0: summary, no anomalies", dict(anom=None)), ("k1: summary", dict(anom=anom)),
                 ("k2: summary and the filtered mask", dict(anom=anom, mask=hob))):
    k = kernel_ms(lambda: res.__setitem__("r", eng.cell_events(m8, min_duration=D, max_gap=GAP, finish=True, **kw)))
    r = res["r"]
    item = 1 + (4 if kw["anom"] is not None else 0)
    print(json.dumps(dict({"variant": name}, **med(k), events=int(r["events"].sum(dtype=np.int64)),
                          event_days=int(r["event_days"].sum(dtype=np.int64)),
                          GB_per_s_on_mask_plus_anomalies=round(item * n / statistics.median(k) / 1e6, 1))), flush=True)
assert int(hob.sum(dtype=torch.int64).item()) == int(res["r"]["event_days"].sum(dtype=np.int64))
rec = eng.cell_event_records(res["r"]["acc"])
k = kernel_ms(lambda: res.__setitem__("r2", eng.cell_events(m8, anom, min_duration=D, max_gap=GAP, records=rec, finish=True)))
assert res["r2"]["rec"]["start"].size == rec["n"]
print(json.dumps(dict({"variant": "k3: the second pass, records written", "records": rec["n"]}, **med(k))), flush=True)
k = kernel_ms(lambda: eng.local_intensity(m8, anom, finish=False))
print(json.dumps(dict({"variant": "li: marex_local_intensity_u8 without categories, the same field"}, **med(k))), flush=True)
eng.ctx.timing_enable(False)
dx, da_ = torch.empty_like(m8), torch.empty_like(anom)
cp = copy_ms([(dx, m8), (da_, anom)])
print(json.dumps(dict({"variant": "c1: device-to-device copy of the mask and the anomalies"}, **med(cp),
                      GB_per_s_read_plus_written=round(2 * 5 * n / statistics.median(cp) / 1e6, 1))), flush=True)
cp = copy_ms([(dx, m8), (da_, anom), (hob, m8)])
print(json.dumps(dict({"variant": "c2: the same and one more uint8 field"}, **med(cp),
                      GB_per_s_read_plus_written=round(2 * 6 * n / statistics.median(cp) / 1e6, 1))), flush=True)
del dx, da_, hob, res, rec
torch.cuda.empty_cache()

# (r), (h) the whole call
tv = (np.datetime64("2000-01-01") + np.arange(T)).astype("datetime64[ns]")
coords = {"time": ("time", tv)}
dims = ("time", "lat", "lon")
out = {}
CALLS = (("by='year'", dict(by="year")), ("return_mask=True, records=True", dict(return_mask=True, records=True)))
for name, kw in CALLS:
    r = wall(lambda: out.__setitem__(("r", name), marex_amd.cell_events(
        DataArray(m8.view(T, ny, nx), dims=dims, coords=coords), DataArray(anom.view(T, ny, nx), dims=dims, coords=coords), **kw)))
    print(json.dumps(dict({"variant": f"r: cell_events({name}), resident inputs"}, **med(r))), flush=True)
m8_h, anom_h = m8.cpu().numpy().reshape(T, ny, nx), anom.cpu().numpy().reshape(T, ny, nx)
del m8, anom
torch.cuda.empty_cache()
for name, kw in CALLS:
    h = wall(lambda: out.__setitem__(("h", name), marex_amd.cell_events(
        DataArray(m8_h, dims=dims, coords=coords), DataArray(anom_h, dims=dims, coords=coords), **kw)), reps=3)
    print(json.dumps(dict({"variant": f"h: cell_events({name}), host arrays (uploaded whole)"}, **med(h))), flush=True)
    a, b = out[("r", name)], out[("h", name)]
    same = all((v.data.cpu().numpy() if isinstance(v.data, torch.Tensor) else np.asarray(v.data)).astype(np.asarray(b[k].data).dtype).tobytes()
               == np.asarray(b[k].data).tobytes() for k, v in a.data_vars.items())
    print(json.dumps({"variant": name, "resident_and_host_results_same_bytes": same}), flush=True)
del out

# (n) NumPy on the host: the row loop of the state machine, vectorised over the cells
nt = []
for _ in range(2):
    t0 = time.perf_counter()
    co.walk(m8_h.reshape(T, C)[:HOST_STEPS], anom_h.reshape(T, C)[:HOST_STEPS], 0, D, GAP, None, 1, np.zeros((HOST_STEPS, C), np.uint8))
    nt.append((time.perf_counter() - t0) * 1e3)
per = min(nt) / HOST_STEPS
print(json.dumps({"variant": "n: NumPy row loop of the state machine on the host, with the mask", "steps_timed": HOST_STEPS,
                  "ms_per_step": round(per, 3), "ms_scaled_to_all_steps": round(per * T, 1)}), flush=True)
