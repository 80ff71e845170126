"""One-off measurement (not a pytest file): lagged composites (``marex_event_composites_u8``) on a uint8 mask of the size of
cfg2 (``CPS_STEPS`` x ``CPS_NY`` x ``CPS_NX``, default 1826 x 720 x 1440, daily from 2000-01-01) and its float32 anomalies:
the mask is the upper ``CPS_COVER`` (default 4.5 %) of smoothed device noise (the blobby mask of
tests/measure_event_occurrence.py), the values are that smoothed noise itself.

(k)   the kernel at ``max_lag`` 10 and 30, for onsets and for ends, and at 10 with ``by="season"``;
(c)   baseline: ``torch`` device-to-device copies of the two fields (reads and writes them);
(t)   the composition the call replaces, in ``torch`` from the resident fields: the onset mask ``m[1:] & ~m[:-1]``, then
      for every lag a masked, NaN-aware float64 sum and a count of the shifted values -- ``2 L + 1`` passes, at 10 and at 30;
(r)   ``marex_amd.event_composites(max_lag=10)`` on the resident fields;
(h)   the same from the host arrays (block_steps=None: both fields are uploaded whole);
(n)   baseline: the NumPy oracle of tests/event_composites_oracle.py on the first ``CPS_HOST_CELLS`` cells (default 4096),
      ``max_lag=10``, scaled to all cells.

Kernel times are the engine's launch timer (HIP events around the launch inside the library), the copy and the composition
are timed between two device events, wall times are host clocks that end in a synchronise; medians of REPS after one
warm-up, with the smallest and the largest.  The cost of the kernel scales with anchors x (2 L + 1), not with the field's
size: the anchors per cell of the measured field are printed beside the times."""
import json
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import numpy as np
import torch

import event_composites_oracle as eo
import marex_amd
import marex_amd.occurrence as mo
from marex_amd.detect import get_engine

REPS = 5
T = int(os.environ.get("CPS_STEPS", 1826))
ny = int(os.environ.get("CPS_NY", 720))
nx = int(os.environ.get("CPS_NX", 1440))
COVER = float(os.environ.get("CPS_COVER", 0.045))
HOST_CELLS = int(os.environ.get("CPS_HOST_CELLS", 4096))
C = ny * nx
n = T * C
eng = get_engine(0)
print(json.dumps({"device": torch.cuda.get_device_name(0), "reps": REPS, "T": T, "ny": ny, "nx": nx}), flush=True)


def blobby(frac, seed=1):
    g = torch.Generator(device=eng.device).manual_seed(seed)
    f = torch.randn((1, 1, T, ny, nx), generator=g, device=eng.device)
    for _ in range(2):  # two box passes ~ a Gaussian of (1, 6, 8) cells
        f = torch.nn.functional.avg_pool3d(f, (3, 13, 17), stride=1, padding=(1, 6, 8), count_include_pad=False)
    f = f.reshape(T, C).contiguous()
    thr = torch.quantile(f.reshape(-1)[:: 113][: 16_000_000], 1.0 - frac)
    return (f > thr).to(torch.uint8), f


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


X, V = blobby(COVER)
torch.cuda.empty_cache()
Xb = X.view(torch.bool)
n_on = int((Xb[1:] & ~Xb[:-1]).sum(dtype=torch.int64).item())
n_end = int((Xb[:-1] & ~Xb[1:]).sum(dtype=torch.int64).item())
print(json.dumps({"coverage": round(int(X.sum(dtype=torch.int64).item()) / n, 4), "onsets_per_cell": round(n_on / C, 3),
                  "ends_per_cell": round(n_end / C, 3)}), flush=True)

tv = (np.datetime64("2000-01-01") + np.arange(T)).astype("datetime64[ns]")
season, G_s, _, _ = mo.group_labels("season", tv, T)
eng.ctx.timing_enable(True)
kernel_runs = {}
CONFIGS = [("k: max_lag=10, onset", dict(max_lag=10, anchor="onset")), ("k: max_lag=10, end", dict(max_lag=10, anchor="end")),
           ("k: max_lag=30, onset", dict(max_lag=30, anchor="onset")), ("k: max_lag=30, end", dict(max_lag=30, anchor="end")),
           ("k: max_lag=10, onset, by='season'", dict(max_lag=10, anchor="onset", grp=season, G=G_s))]
for name, kw in CONFIGS:
    res = {}
    k = kernel_ms(lambda: res.__setitem__("r", eng.event_composites(X, V, 0, 0, T, T, finish=False, **kw)))
    acc = res["r"]["acc"]
    used = int(acc["anchors"].sum(dtype=torch.int64).item())
    assert acc["status"].cpu().tolist() == [0] and used == (n_on if kw["anchor"] == "onset" else n_end)
    L = kw["max_lag"]
    kernel_runs[name] = k
    print(json.dumps(dict({"variant": name}, **med(k), anchors=used, anchors_per_cell=round(used / C, 3),
                          ns_per_anchor_and_lag=round(statistics.median(k) * 1e6 / max(used * (2 * L + 1), 1), 4))), flush=True)
    del res, acc
    torch.cuda.empty_cache()

dst_x, dst_v = torch.empty_like(X), torch.empty_like(V)
cp = events_ms(lambda: (dst_x.copy_(X), dst_v.copy_(V)))
print(json.dumps(dict({"variant": "c: device-to-device copies of the two fields (read and written)"}, **med(cp),
                      GB_per_s_read_plus_written=round(10 * n / statistics.median(cp) / 1e6, 1))), flush=True)
del dst_x, dst_v
torch.cuda.empty_cache()


def composition(L):
    on = torch.zeros((T, C), dtype=torch.bool, device=eng.device)
    on[1:] = Xb[1:] & ~Xb[:-1]
    s = torch.zeros((2 * L + 1, C), dtype=torch.float64, device=eng.device)
    cnt = torch.zeros((2 * L + 1, C), dtype=torch.int64, device=eng.device)
    for lag in range(-L, L + 1):
        lo, hi = max(0, -lag), min(T, T - lag)  # the anchor steps whose step t + lag lies in the record
        if lo >= hi:
            continue
        vv = V[lo + lag:hi + lag]
        ok = on[lo:hi] & torch.isfinite(vv)
        s[lag + L] = torch.where(ok, vv, 0.0).sum(dim=0, dtype=torch.float64)
        cnt[lag + L] = ok.sum(dim=0)
    return s, cnt


for L in (10, 30):
    comp = events_ms(lambda: composition(L))
    name = f"k: max_lag={L}, onset"
    k = kernel_runs[name]
    spreads = (max(comp) - min(comp)) + (max(k) - min(k))
    print(json.dumps(dict({"variant": f"t: torch composition, max_lag={L}: onset mask, then {2 * L + 1} masked sums and counts"}, **med(comp),
                          kernel_ms_median=round(statistics.median(k), 3), both_spreads_ms=round(spreads, 3),
                          times_the_kernel=round(statistics.median(comp) / statistics.median(k), 1),
                          kernel_faster_by_more_than_both_spreads=statistics.median(comp) - statistics.median(k) > spreads)), flush=True)
    torch.cuda.empty_cache()
# the two agree (the torch sums are in another order: compared loosely)
r = eng.event_composites(X, V, 0, 0, T, T, max_lag=2, finish=False)["acc"]
s, cnt = composition(2)
assert torch.equal(r["cnt"][0].t().to(torch.int64), cnt)
assert torch.allclose(r["sum"][0].t(), s, rtol=1e-9, atol=1e-9)
del r, s, cnt
eng.ctx.timing_enable(False)
torch.cuda.empty_cache()

# (r), (h) the whole call
res = {}
kw = dict(max_lag=10)
rr = wall(lambda: res.__setitem__("r", marex_amd.event_composites(X.view(T, ny, nx), V.view(T, ny, nx), **kw)))
print(json.dumps(dict({"variant": "r: event_composites(max_lag=10), resident fields"}, **med(rr))), flush=True)
X_h, V_h = X.cpu().numpy().reshape(T, ny, nx), V.cpu().numpy().reshape(T, ny, nx)
h = wall(lambda: res.__setitem__("h", marex_amd.event_composites(X_h, V_h, **kw)))
print(json.dumps(dict({"variant": "h: the same from host arrays (uploaded whole)"}, **med(h))), flush=True)
same = all(np.asarray(res["r"][v].values).tobytes() == np.asarray(res["h"][v].values).tobytes() for v in res["r"].data_vars)
print(json.dumps({"resident_and_host_results_same_bytes": same}), flush=True)
cells = min(C, HOST_CELLS)
sub_x = np.ascontiguousarray(X_h.reshape(T, C)[:, :cells])
sub_v = np.ascontiguousarray(V_h.reshape(T, C)[:, :cells])
got = {k: np.asarray(res["r"][k].values).reshape(-1, C)[:, :cells] for k in ("composite_count", "composite_sum", "composite_sumsq")}
del X, V, Xb, res
torch.cuda.empty_cache()

# (n) NumPy on the host
nt = []
for _ in range(3):
    t0 = time.perf_counter()
    want = eo.composites(sub_x, sub_v, 10)
    nt.append((time.perf_counter() - t0) * 1e3)
equal = all(np.ascontiguousarray(got["composite_" + k]).tobytes() == want[k][0].tobytes() for k in ("count", "sum", "sumsq"))
per = statistics.median(nt[1:]) / cells
print(json.dumps({"variant": "n: the NumPy oracle on the host, max_lag=10", "cells_timed": cells, "ms_per_cell": round(per, 4),
                  "ms_scaled_to_all_cells": round(per * C, 1), "device_result_equals_the_oracle_on_these_cells": equal}), flush=True)
