"""One-off measurement (not a pytest file): compound events (``marex_compound_u8``) on a pair of uint8 masks of the size of
cfg2 (``CMP_STEPS`` x ``CMP_NY`` x ``CMP_NX``, default 1826 x 720 x 1440, daily from 2000-01-01).  Field A is a 5 % mask of
smoothed device noise (the blobby mask of tests/measure_event_occurrence.py); field B is A shifted by three steps over the
northern half of the rows and an independent 5 % mask over the southern half.

(k00) the kernel, ``max_lag=0, tolerance=0``;     (k72) ``max_lag=7, tolerance=2``;     (k3030) ``max_lag=30, tolerance=30``;
(kg)  (k00) with ``by="season"`` and ``zonal=True, zonal_by="month"`` added;
(km)  (k00) with the joint mask written;
(c)   baseline: ``torch`` device-to-device copies of both fields (reads and writes them: twice the bytes (k00) reads);
(t)   the composition the call replaces: ``torch`` ``a & b``, then ``marex_occurrence_u8`` on a, on b and on the joint mask
      (device events around all four; the three launches alone from the launch timer);
(r)   ``marex_amd.compound_events`` on the resident fields, ``max_lag=7, tolerance=2``;
(h)   the same from the host arrays (block_steps=None: both fields are uploaded whole);
(n)   baseline: NumPy on the host, the vectorised oracle functions of tests/compound_oracle.py (counts, lags -7 .. 7, run
      coincidence at tolerance 2) plus a per-step loop for the joint run statistics, on the first ``CMP_HOST_STEPS`` steps
      (default 64), scaled.

Kernel times are the engine's launch timer (HIP events around the launch inside the library), the copy and the composition
are timed between two device events, wall times are host clocks that end in a synchronise; medians of REPS after one
warm-up."""
import json
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import numpy as np
import torch

import compound_oracle as co
import marex_amd
import marex_amd.occurrence as mo
from marex_amd.detect import get_engine

REPS = 5
T = int(os.environ.get("CMP_STEPS", 1826))
ny = int(os.environ.get("CMP_NY", 720))
nx = int(os.environ.get("CMP_NX", 1440))
HOST_STEPS = min(T, int(os.environ.get("CMP_HOST_STEPS", 64)))
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
    return (f > thr).to(torch.uint8)


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


def events_ms(fn):
    out = []
    for _ in range(REPS + 1):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        eng.sync()
        a.record()
        fn()
        b.record()
        eng.sync()
        out.append(a.elapsed_time(b))
    return out[1:]


A = blobby(seed=1)
B = blobby(seed=2)
half = (ny // 2) * nx  # the northern rows: B follows A by three steps
B[3:, :half] = A[:T - 3, :half]
B[:3, :half] = 0
both = int((A & B).sum(dtype=torch.int64).item())
print(json.dumps({"coverage_a": round(int(A.sum(dtype=torch.int64).item()) / n, 4), "coverage_b": round(int(B.sum(dtype=torch.int64).item()) / n, 4),
                  "coverage_both": round(both / n, 5)}), flush=True)

tv = (np.datetime64("2000-01-01") + np.arange(T)).astype("datetime64[ns]")
season, G_s, _, _ = mo.group_labels("season", tv, T)
month, G_m, _, _ = mo.zonal_labels("month", tv, T)
rows = np.repeat(np.arange(ny, dtype=np.int32), nx)
joint = torch.empty((T, C), dtype=torch.uint8, device=eng.device)
eng.ctx.timing_enable(True)
CONFIGS = [("k00: max_lag=0, tolerance=0", {}), ("k72: max_lag=7, tolerance=2", dict(max_lag=7, tolerance=2)),
           ("k3030: max_lag=30, tolerance=30", dict(max_lag=30, tolerance=30)),
           ("kg: k00 + by='season', zonal_by='month'", dict(grp=season, G=G_s, sgrp=month, G2=G_m, cls=rows, R=ny)),
           ("km: k00 + the joint mask written", dict(mask=joint))]
for name, kw in CONFIGS:
    res = {}
    k = kernel_ms(lambda: res.__setitem__("r", eng.compound(A, B, finish=False, **kw)))
    acc = res["r"]["acc"]
    assert acc["status"].cpu().tolist() == [0, 0] and int(acc["cell_cnt"][2].sum(dtype=torch.int64).item()) == both
    extra = {}
    if acc["lag"] is not None:
        L = kw["max_lag"]
        assert int(acc["lag"][L].sum(dtype=torch.int64).item()) == both
        extra["pairs_counted"] = int(acc["lag"].sum(dtype=torch.int64).item())
    if "mask" in kw:
        assert int(joint.sum(dtype=torch.int64).item()) == both
    print(json.dumps(dict({"variant": name}, **med(k), GB_per_s_on_both_fields=round(2 * n / statistics.median(k) / 1e6, 1), **extra)),
          flush=True)
    del res, acc
del joint
torch.cuda.empty_cache()

dst = torch.empty((2, T, C), dtype=torch.uint8, device=eng.device)
cp = events_ms(lambda: (dst[0].copy_(A), dst[1].copy_(B)))
print(json.dumps(dict({"variant": "c: device-to-device copies of both fields (read and written)"}, **med(cp),
                      GB_per_s_read_plus_written=round(4 * n / statistics.median(cp) / 1e6, 1))), flush=True)
del dst
torch.cuda.empty_cache()


def composition():
    j = A & B
    for x in (A, B, j):
        eng.occurrence(x, finish=False)


comp = events_ms(composition)
comp_k = kernel_ms(composition)
print(json.dumps(dict({"variant": "t: torch a & b, then three marex_occurrence_u8 launches"}, **med(comp),
                      ms_median_of_the_three_launches_alone=round(statistics.median(comp_k), 3))), flush=True)
eng.ctx.timing_enable(False)
torch.cuda.empty_cache()

# (r), (h) the whole call
res = {}
kw = dict(max_lag=7, tolerance=2)
r = wall(lambda: res.__setitem__("r", marex_amd.compound_events(A.view(T, ny, nx), B.view(T, ny, nx), **kw)))
print(json.dumps(dict({"variant": "r: compound_events(max_lag=7, tolerance=2), resident fields"}, **med(r))), flush=True)
A_h, B_h = A.cpu().numpy().reshape(T, ny, nx), B.cpu().numpy().reshape(T, ny, nx)
h = wall(lambda: res.__setitem__("h", marex_amd.compound_events(A_h, B_h, **kw)))
print(json.dumps(dict({"variant": "h: the same from host arrays (uploaded whole)"}, **med(h))), flush=True)
same = all(np.asarray(res["r"][v].values).tobytes() == np.asarray(res["h"][v].values).tobytes() for v in res["r"].data_vars)
print(json.dumps({"resident_and_host_results_same_bytes": same}), flush=True)
del A, B, res
torch.cuda.empty_cache()


# (n) NumPy on the host
def numpy_steps(steps):
    a, b = A_h[:steps].reshape(steps, C) != 0, B_h[:steps].reshape(steps, C) != 0
    out = [co.day_counts(a, b), co.lag_days(a, b, 7), co.run_coincidence(a, b, 2), co.run_coincidence(b, a, 2)]
    run, nrun, longest = np.zeros(C, np.uint32), np.zeros(C, np.uint32), np.zeros(C, np.uint32)
    for t in range(steps):
        p = a[t] & b[t]
        nrun += p & (run == 0)
        run = np.where(p, run + 1, 0).astype(np.uint32)
        np.maximum(longest, run, out=longest)
    return out, nrun, longest


nt = []
for _ in range(3):
    t0 = time.perf_counter()
    numpy_steps(HOST_STEPS)
    nt.append((time.perf_counter() - t0) * 1e3)
per = statistics.median(nt[1:]) / HOST_STEPS
print(json.dumps({"variant": "n: NumPy on the host (counts, lags -7 .. 7, run coincidence, joint runs)", "steps_timed": HOST_STEPS,
                  "ms_per_step": round(per, 3), "ms_scaled_to_all_steps": round(per * T, 1)}), flush=True)
