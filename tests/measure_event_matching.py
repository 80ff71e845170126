"""One-off measurement (not a pytest file): the event matching (``marex_event_matching_count_i32`` /
``marex_event_matching_i32``) on two tracked fields of the size of cfg2 (``MAT_STEPS`` x ``MAT_NY`` x ``MAT_NX``, default 1826 x
720 x 1440).  Field A is the blobby 5 % mask of the other ``measure_*`` scripts, tracked by the basic tracker.  Field B is A
moved three steps later over the southern half of the rows; with ``MAT_RETRACK=1`` its mask is tracked again, otherwise (the
default: one tracker run per visit) its IDs are permuted at random, so that the labels of B say nothing about those of A.  The
output says which.

(k) resident inputs, between two device events: the count pass; the whole insert call (zeroing the table, the insert pass,
    the compaction) for the cells alone and with areas; the latter on one step at the same table size (zeroing and compaction
    alone, so that the insert pass is the difference); the runs, the distinct keys, the widths and the table's bytes;
(c) baseline: a device-to-device copy of the two ID fields;
(x) ``marex_event_exposure_count_i32`` / ``marex_event_exposure_i32`` on field A with the 720 grid rows as regions, areas, no
    anomalies: the same passes over one field and a map;
(r) ``marex_amd.event_matching`` from resident and (h) from host fields: both passes, the sort, the host finish;
(n) the NumPy oracle of the tests on the first ``MAT_ORACLE_STEPS`` steps (default 2), scaled.

Wall times are host clocks that end in a synchronise, device times are HIP events; medians of REPS after one warm-up."""
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
from marex_amd.regional import area_weight_table
from marex_amd.zarr_io import DeviceDataArray

REPS = 5
T = int(os.environ.get("MAT_STEPS", 1826))
ny = int(os.environ.get("MAT_NY", 720))
nx = int(os.environ.get("MAT_NX", 1440))
ORACLE_STEPS = min(T, int(os.environ.get("MAT_ORACLE_STEPS", 2)))
RETRACK = os.environ.get("MAT_RETRACK", "0") == "1"
SHIFT = 3
C = ny * nx
n = T * C
eng = get_engine(0)
dev = eng.device
print(json.dumps({"device": torch.cuda.get_device_name(0), "reps": REPS, "T": T, "ny": ny, "nx": nx}), flush=True)


def blobby(frac=0.05, seed=1):
    g = torch.Generator(device=dev).manual_seed(seed)
    f = torch.randn((1, 1, T, ny, nx), generator=g, device=dev)
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


def device_ms(launch, prepare=lambda: None):
    out = []
    for _ in range(REPS + 1):
        prepare()
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        eng.sync()
        a.record()
        launch()
        b.record()
        eng.sync()
        out.append(a.elapsed_time(b))
    return out[1:]


lat, lon = np.linspace(-89.875, 89.875, ny), np.linspace(0.125, 359.875, nx)


def track(mask):
    da = DeviceDataArray(mask.view(T, ny, nx), ("time", "lat", "lon"), {"time": np.arange(T), "lat": lat, "lon": lon})
    t0 = time.perf_counter()
    events = marex_amd.tracker(da, np.ones((ny, nx), bool), R_fill=2, T_fill=2, area_filter_quartile=0.5, allow_merging=False).run()
    print(json.dumps({"tracker_run_s": round(time.perf_counter() - t0, 2)}), flush=True)
    return np.ascontiguousarray(np.asarray(events["ID_field"].values).reshape(T, C), dtype=np.int32)


def later_in_the_south(x):
    y = x.clone().view(T, ny, nx)
    y[SHIFT:, : ny // 2] = x.view(T, ny, nx)[: T - SHIFT, : ny // 2]
    y[:SHIFT, : ny // 2] = 0
    return y.view(T, C)


field = blobby()
ids_a_h = track(field)
ids_a = torch.from_numpy(ids_a_h).to(dev)
Na = int(ids_a.max().item())
if RETRACK:
    ids_b_h = track(later_in_the_south(field))
    ids_b = torch.from_numpy(ids_b_h).to(dev)
    second = f"the mask of A moved {SHIFT} steps later over the southern half of the rows, tracked again"
else:
    perm = torch.zeros(Na + 1, dtype=torch.int32, device=dev)
    perm[1:] = (torch.randperm(Na, generator=torch.Generator(device=dev).manual_seed(3), device=dev) + 1).to(torch.int32)
    ids_b = perm[later_in_the_south(ids_a).long()].contiguous()
    ids_b_h = ids_b.cpu().numpy()
    second = f"field A moved {SHIFT} steps later over the southern half of the rows, its IDs permuted at random (not tracked again)"
del field
held = int(((ids_a > 0) | (ids_b > 0)).sum().item())
Nb = int(ids_b.max().item())
print(json.dumps({"second_field": second, "events_a": Na, "events_b": Nb, "present_cells": held, "coverage": round(held / n, 4)}), flush=True)
area_y = np.cos(np.radians(lat)) * (111.195 * 0.25) ** 2
areas = np.repeat(area_y, nx)
e, q_h = area_weight_table(areas)
q = eng._dev(q_h)
status = torch.zeros(8, dtype=torch.int64, device=dev)

# (k) the kernels
cms = device_ms(lambda: eng.call("marex_event_matching_count_i32", ids_a, ids_b, T, C, status))
s = status.cpu().numpy()
runs = int(s[2])
assert int(s[0]) == 0 and int(s[1]) == 0 and int(s[3]) == Na and int(s[4]) == Nb
widths = HotPath.matching_widths(Na, Nb, T)
assert T <= 1 << widths[2]
cap = HotPath.exposure_cap(runs)
per = HotPath.matching_entry_bytes(True)
tab = {k: torch.empty(cap, dtype=torch.int64, device=dev) for k in ("keys", "cnt", "area")}
out = {k: torch.empty(runs, dtype=torch.int64, device=dev) for k in tab}


def insert(xa, xb, steps, areas_on=True):
    return lambda: eng.call("marex_event_matching_i32", xa, xb, steps, C, q if areas_on else None, *widths, cap, tab["keys"], tab["cnt"],
                            tab["area"] if areas_on else None, status, runs, out["keys"], out["cnt"], out["area"] if areas_on else None)


bare = device_ms(insert(ids_a, ids_b, T, False))
whole = device_ms(insert(ids_a, ids_b, T))
s = status.cpu().numpy()
keys = int(s[7])
assert int(s[5]) == 0 and int(s[6]) == 0 and 0 < keys <= runs and int(out["cnt"][:keys].sum().item()) == held
rest = device_ms(insert(ids_a[:1], ids_b[:1], 1))
k_ms = statistics.median(cms) + statistics.median(whole)
ins = statistics.median(whole) - statistics.median(rest)
print(json.dumps({"variant": "k: event matching kernels", "runs": runs, "distinct_keys": keys, "widths": list(widths), "cap": cap,
                  "entry_bytes": per, "table_bytes": per * cap, "compacted_bytes": per * runs, "count_pass": med(cms),
                  "insert_call_cells_only": med(bare), "insert_call_with_areas": med(whole), "zeroing_and_compaction_alone": med(rest),
                  "insert_pass_ms_by_difference": round(ins, 3), "count_GB_per_s_on_both_fields": round(8 * n / statistics.median(cms) / 1e6, 1),
                  "insert_GB_per_s_on_both_fields": round(8 * n / ins / 1e6, 1), "insert_ns_per_run": round(ins * 1e6 / runs, 2)}), flush=True)
del tab, out
torch.cuda.empty_cache()

# (c) a device-to-device copy of the two fields
d1, d2 = torch.empty_like(ids_a), torch.empty_like(ids_b)
cp = device_ms(lambda: (d1.copy_(ids_a), d2.copy_(ids_b)))
print(json.dumps({"variant": "c: device-to-device copy of the two ID fields", "both": med(cp),
                  "GB_per_s_read_plus_written": round(16 * n / statistics.median(cp) / 1e6, 1),
                  "count_pass_over_copy": round(statistics.median(cms) / statistics.median(cp), 3),
                  "insert_pass_over_copy": round(ins / statistics.median(cp), 3)}), flush=True)
del d1, d2
torch.cuda.empty_cache()

# (x) the exposure passes on field A, the grid rows as regions
reg = eng._dev(np.repeat(np.arange(ny, dtype=np.int32), nx))
xc = device_ms(lambda: eng.call("marex_event_exposure_count_i32", ids_a, T, C, reg, ny, status))
xruns = int(status.cpu().numpy()[2])
xcap = HotPath.exposure_cap(xruns)
xt = {k: torch.empty(xcap, dtype=torch.int64, device=dev) for k in ("keys", "cnt", "area")}
xo = {k: torch.empty(xruns, dtype=torch.int64, device=dev) for k in xt}


def xinsert(x, steps):
    return lambda: eng.call("marex_event_exposure_i32", x, steps, C, reg, ny, q, None, None, xcap, xt["keys"], xt["cnt"], xt["area"], None,
                            None, status, xruns, xo["keys"], xo["cnt"], xo["area"], None, None)


xw = device_ms(xinsert(ids_a, T))
xkeys = int(status.cpu().numpy()[3])
xr = device_ms(xinsert(ids_a[:1], 1))
xins = statistics.median(xw) - statistics.median(xr)
print(json.dumps({"variant": "x: marex_event_exposure on field A, R=720 rows, areas, no anomalies", "runs": xruns, "distinct_keys": xkeys,
                  "cap": xcap, "count_pass": med(xc), "insert_call": med(xw), "zeroing_and_compaction_alone": med(xr),
                  "insert_pass_ms_by_difference": round(xins, 3), "insert_ns_per_run": round(xins * 1e6 / xruns, 2),
                  "matching_count_over_exposure_count": round(statistics.median(cms) / statistics.median(xc), 3),
                  "matching_insert_over_exposure_insert": round(ins / xins, 3)}), flush=True)
del xt, xo, reg
torch.cuda.empty_cache()

# (r), (h) the whole call
a3, b3 = ids_a.view(T, ny, nx), ids_b.view(T, ny, nx)
keep = {}
r = wall(lambda: keep.__setitem__("ds", marex_amd.event_matching(a3, b3, cell_areas=area_y)))
ds = keep["ds"]
print(json.dumps(dict({"variant": "r: event_matching, resident fields, areas", "pairs": int(np.asarray(ds["pair_ID_a"].values).size),
                       "pod": float(ds["pod"].values), "far": float(ds["far"].values), "csi": float(ds["csi"].values),
                       "kernels_ms": round(k_ms, 3)}, **med(r))), flush=True)
h = wall(lambda: marex_amd.event_matching(ids_a_h.reshape(T, ny, nx), ids_b_h.reshape(T, ny, nx), cell_areas=area_y, block_steps="auto"))
print(json.dumps(dict({"variant": "h: event_matching, host fields, areas"}, **med(h))), flush=True)

# (n) the NumPy oracle of the tests on a slice
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import event_matching_oracle as mo  # noqa: E402

ot = []
for _ in range(2):
    t0 = time.perf_counter()
    recs = mo.step_records(ids_a_h[:ORACLE_STEPS + SHIFT][SHIFT:], ids_b_h[:ORACLE_STEPS + SHIFT][SHIFT:], q_h)
    ot.append((time.perf_counter() - t0) * 1e3)
per_step = min(ot) / ORACLE_STEPS
print(json.dumps({"variant": "n: the NumPy oracle of the tests (tests/event_matching_oracle.py), areas", "steps_timed": ORACLE_STEPS,
                  "records": len(recs), "ms_per_step": round(per_step, 1), "ms_scaled_to_all_steps": round(per_step * T, 1),
                  "kernels_over_n": round(k_ms / (per_step * T), 7)}), flush=True)
