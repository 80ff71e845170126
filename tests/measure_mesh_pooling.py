"""MI355X: what do thresholds pooled over mesh neighbour rings cost?
    python tests/measure_mesh_pooling.py [cells]
The cfg4 shape per device (15 output years of a 30-yr record x 0.5 M cells, lists of 15 rows: 1 list of 2 chunks per bucket,
11-day window): kernel time of marex_hobday_thresholds_pool_f32 for one and two rings on both of its paths (first chunks in
an LDS ring / read from global memory at every probe) beside the unpooled k_thr_cells on the same lists in the
same run, the whole hobday_approx stage with and without pooling, and a device-to-device copy of the lists as the memory
yardstick.  Kernel times are the library's own event timers around the launches (the host-side check of the pool table is
outside them and shows in the stage times)."""
import json
import sys
import time

import numpy as np
import torch

sys.path.insert(0, ".")
from marex_amd import binning, calendar  # noqa: E402
from marex_amd.engine import HotPath  # noqa: E402

C = int(sys.argv[1]) if len(sys.argv) > 1 else 500_000
REPS = 5
hot = HotPath(0)
bt = binning.hobday_bins()
tm = calendar.daily_time_axis("2005-01-01", 5478)
cal = calendar.build_calendar(tm)
dcal = hot.upload_calendar(cal)
gen = torch.Generator(device=hot.device).manual_seed(1)
anom = torch.randn((len(tm), C), device=hot.device, dtype=torch.float32, generator=gen) * 0.8
tl = hot.tail_extract(anom, dcal, bt, list_rows=hot.LIST_ROWS_SHIFT)
rng = np.random.default_rng(2)
nbr = np.zeros((3, C), dtype=np.int32)  # a ring with one random chord per cell, 1-based
nbr[0] = (np.arange(C) + 1) % C + 1
nbr[1] = (np.arange(C) - 1) % C + 1
nbr[2] = rng.integers(0, C, C) + 1
wsp = {}


def kernel_ms(fn):
    hot.ctx.timing_enable(True)
    for k in range(REPS + 1):
        if k == 1:
            hot.sync()
            hot.ctx.timing_reset()
        fn()
    hot.sync()
    ms, n = hot.ctx.timing_get("thresholds")
    hot.ctx.timing_enable(False)
    return round(ms / max(n, 1), 3)


def wall_ms(fn):
    fn()
    hot.sync()
    t0 = time.perf_counter()
    for _ in range(REPS):
        fn()
    hot.sync()
    return round((time.perf_counter() - t0) / REPS * 1e3, 3)


out = {"cells": C, "rows": len(tm), "max_bucket": int(cal.max_bucket), "list_bytes": int(tl["tails"].numel() * 2)}
out["unpooled k_thr_cells ms"] = kernel_ms(lambda: hot.hobday_thresholds_tails(tl, anom, dcal, bt, 0.95, 11, 1, 0, C, wsp=wsp))
out["hobday_approx unpooled ms"] = wall_ms(lambda: hot.hobday_approx(anom, dcal, bt, 0.95, 11, 1, 0, C, wsp=wsp, tails=tl))
copy = torch.empty_like(tl["tails"])
out["lists device-to-device copy ms"] = wall_ms(lambda: copy.copy_(tl["tails"]))
del copy
for rings in (1, 2):
    t0 = time.perf_counter()
    tab = HotPath.pool_table(nbr, rings)
    out[f"r={rings} pool_table host ms"] = round((time.perf_counter() - t0) * 1e3, 1)
    pool = torch.from_numpy(tab).to(hot.device)
    out[f"r={rings} K"] = int(tab.shape[0])
    for ring in (-1, 1, 0):
        with hot.ctx.options(**({} if ring < 0 else {"THR_POOL_RING": ring})):
            hot.ctx.debug_counters(reset=True)
            ms = kernel_ms(lambda: hot.hobday_thresholds_pool(tl, anom, dcal, bt, 0.95, 11, pool, wsp=wsp))
            c = hot.ctx.debug_counters(reset=True)
        out[f"r={rings} pooled kernel ms ({'auto' if ring < 0 else 'THR_POOL_RING=%d' % ring}: {'LDS ring' if c[0] else 'global memory'})"] = ms
        if ring < 0:
            out[f"r={rings} ratio to unpooled"] = round(ms / out["unpooled k_thr_cells ms"], 2)
    out[f"r={rings} hobday_approx pooled ms"] = wall_ms(lambda: hot.hobday_approx(anom, dcal, bt, 0.95, 11, 1, 0, C, wsp=wsp, tails=tl, pool=pool))
print(json.dumps(out, indent=1))
