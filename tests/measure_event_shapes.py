"""One-off measurement (not a pytest file): event shapes (``marex_event_shapes_i32``) on a tracked field of the size of cfg2
(``SHP_STEPS`` x ``SHP_NY`` x ``SHP_NX``, default 1826 x 720 x 1440).  The event field comes from the basic tracker itself on
a 5 % mask of smoothed device noise (the blobby mask of tests/measure_event_intensity.py); the coverage is reported.

(k)  the library call alone, plain, between two device events;
(km) the same with ``mask``;  (kt) with ``cell_areas`` and ``edge_lengths``;  (ka) with all three;
(z)  control: the plain call on an all-background ID field (4 bytes per cell are read, nothing else);
(m)  yardstick: ``marex_object_moments_i32`` on the same field;
(i)  yardstick: ``marex_event_intensity_f32`` on the same field and an anomaly field;
(c)  yardstick: a device-to-device copy of the ID field;
(r)  ``marex_amd.event_shapes`` on the resident field with every table, per_timestep off: the span passes, the kernel, the
     host finish;  (h) the same from a host array (block_steps=None: the field is uploaded whole);
(o)  the brute-force oracle of tests/event_shapes_oracle.py on the first ``SHP_ORACLE_STEPS`` steps (default 2), scaled;
(rp) one run of (r) with the dense (time, ID) variables (``SHP_DENSE=0`` leaves it out).

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
from marex_amd.regional import area_weight_table
from marex_amd.shapes import edge_weight_tables
from marex_amd.zarr_io import DeviceDataArray

REPS = 5
T = int(os.environ.get("SHP_STEPS", 1826))
ny = int(os.environ.get("SHP_NY", 720))
nx = int(os.environ.get("SHP_NX", 1440))
ORACLE_STEPS = min(T, int(os.environ.get("SHP_ORACLE_STEPS", 2)))
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


field = blobby()
lat, lon = np.linspace(-89.875, 89.875, ny), np.linspace(0.125, 359.875, nx)
da = DeviceDataArray(field.view(T, ny, nx), ("time", "lat", "lon"), {"time": np.arange(T), "lat": lat, "lon": lon})
t0 = time.perf_counter()
events = marex_amd.tracker(da, np.ones((ny, nx), bool), R_fill=2, T_fill=2, area_filter_quartile=0.5, allow_merging=False).run()
print(json.dumps({"tracker_run_s": round(time.perf_counter() - t0, 2)}), flush=True)
del field, da
ids_h = np.ascontiguousarray(np.asarray(events["ID_field"].values).reshape(T, C), dtype=np.int32)
ids = torch.from_numpy(ids_h).to(eng.device)
n = T * C
held = int((ids > 0).sum().item())
N = int(ids.max().item())
print(json.dumps({"events": N, "cells_with_an_event": held, "coverage": round(held / n, 4)}), flush=True)

rng = np.random.default_rng(3)
land = rng.random((ny // 8 + 1, nx // 8 + 1)) > 0.3  # blocky land, 30 %
mask_h = np.kron(land, np.ones((8, 8), bool))[:ny, :nx]
areas_h = np.repeat(np.cos(np.radians(lat))[:, None] * 770.0, nx, axis=1)
edges_h = marex_amd.grid_edge_lengths(lat, lon)
e_a, area_q = area_weight_table(areas_h)
e_l, ns_q, ew_q = edge_weight_tables(edges_h, ny, nx)
mask_d, area_d, ns_d, ew_d = eng._dev(mask_h.view(np.uint8).reshape(-1)), eng._dev(area_q.reshape(-1)), eng._dev(ns_q), eng._dev(ew_q)

sp = eng.id_spans(ids)
tmin, tmax = sp[0].astype(np.int64), sp[1].astype(np.int64)
off = HotPath.event_slot_plan(tmin, tmax)
slots = max(int(off[-1]), 1)
tm_d, off_d = eng._dev(np.clip(tmin, 0, 2**31 - 1).astype(np.int32)), eng._dev(off)
mom = torch.zeros((slots, 16), dtype=torch.int64, device=eng.device)
box = torch.zeros((slots, 6), dtype=torch.int32, device=eng.device)
status = torch.zeros(1, dtype=torch.int64, device=eng.device)


def prepare():
    mom.zero_()
    status.zero_()
    box[:, 0::2] = 2**31 - 1
    box[:, 1::2] = -1


def shapes(f, m=None, a=None, s=None, w=None):
    return lambda: eng.call("marex_event_shapes_i32", f, 0, T, ny, nx, 0, N, tm_d, off_d, slots, m, a, s, w, mom, box, status)


res = {}
for key, what, launch in (("k", "plain", shapes(ids)), ("km", "with mask", shapes(ids, mask_d)),
                          ("kt", "with cell_areas and edge_lengths", shapes(ids, None, area_d, ns_d, ew_d)),
                          ("ka", "with mask, cell_areas and edge_lengths", shapes(ids, mask_d, area_d, ns_d, ew_d))):
    res[key] = device_ms(launch, prepare)
    assert int(status.item()) == 0 and int(mom[:, 0].sum().item()) == held
    print(json.dumps(dict({"variant": f"{key}: marex_event_shapes_i32 alone, {what} (device events)", "slots": slots},
                          **med(res[key]), GB_per_s_on_4_bytes_per_cell=round(4 * n / statistics.median(res[key]) / 1e6, 1))), flush=True)
zero = torch.zeros_like(ids)
z = device_ms(shapes(zero), prepare)
print(json.dumps(dict({"variant": "z: plain call, all-background IDs (reads 4 bytes per cell)"}, **med(z),
                      GB_per_s_on_4_bytes_per_cell=round(4 * n / statistics.median(z) / 1e6, 1))), flush=True)
del zero

# (m) the moments kernel on the same field: its own spans and slots
o_tmin, _, o_off, o_total = eng._object_spans(ids, T, C, N, "measure", "spans")
o_slots = int(o_total.item())
o_acc = torch.zeros((o_slots, 5), dtype=torch.int64, device=eng.device)
m = device_ms(lambda: eng.call("marex_object_moments_i32", ids, T, ny, nx, o_tmin, o_off, o_slots, o_acc), o_acc.zero_)
print(json.dumps(dict({"variant": "m: marex_object_moments_i32 alone (device events)", "slots": o_slots}, **med(m),
                      k_over_m=round(statistics.median(res["k"]) / statistics.median(m), 2),
                      ka_over_m=round(statistics.median(res["ka"]) / statistics.median(m), 2))), flush=True)
del o_acc

# (i) the intensity kernel
g = torch.Generator(device=eng.device).manual_seed(2)
anom = torch.randn((T, C), generator=g, device=eng.device) + 1.5
cnt = torch.zeros((slots, 2), dtype=torch.int64, device=eng.device)
sums = torch.zeros((slots, 2), dtype=torch.float64, device=eng.device)
vmax = torch.zeros(slots, dtype=torch.int32, device=eng.device)
i = device_ms(lambda: eng.call("marex_event_intensity_f32", ids, anom, 0, T, C, N, tm_d, off_d, slots, None, cnt, sums, vmax, status),
              lambda: [b.zero_() for b in (cnt, sums, vmax, status)])
print(json.dumps(dict({"variant": "i: marex_event_intensity_f32 alone (device events)"}, **med(i),
                      k_over_i=round(statistics.median(res["k"]) / statistics.median(i), 2))), flush=True)
del anom, cnt, sums, vmax

# (c) device-to-device copy of the ID field
dst = torch.empty_like(ids)
cp = device_ms(lambda: dst.copy_(ids))
print(json.dumps(dict({"variant": "c: device-to-device copy of the ID field (reads 4, writes 4 bytes per cell)"}, **med(cp),
                      GB_per_s_read_plus_written=round(8 * n / statistics.median(cp) / 1e6, 1),
                      k_over_c=round(statistics.median(res["k"]) / statistics.median(cp), 2))), flush=True)
del dst, mom, box
torch.cuda.empty_cache()

# (r), (rp), (h) the whole call
ids3 = ids.view(T, ny, nx)
out = {}
kw = dict(mask=mask_h, cell_areas=areas_h, edge_lengths=edges_h, lat=lat, lon=lon, per_timestep=False)
r = wall(lambda: out.__setitem__("r", marex_amd.event_shapes(ids3, **kw)))
print(json.dumps(dict({"variant": "r: event_shapes, resident field, every table, per_timestep=False"}, **med(r))), flush=True)
h = wall(lambda: out.__setitem__("h", marex_amd.event_shapes(ids_h.reshape(T, ny, nx), **kw)))
print(json.dumps(dict({"variant": "h: the same from a host field (uploads 4 bytes per cell)"}, **med(h))), flush=True)
same = all(np.asarray(out["r"][v].values).tobytes() == np.asarray(out["h"][v].values).tobytes() for v in out["r"].data_vars)
print(json.dumps({"resident_and_host_results_same_bytes": same, "rows": int(np.asarray(out["r"]["event_duration"].values).sum())}),
      flush=True)

# (o) the brute-force oracle on a few steps
import event_shapes_oracle as so  # noqa: E402

t0 = time.perf_counter()
so.event_shapes(ids_h[:ORACLE_STEPS].reshape(ORACLE_STEPS, ny, nx), mask=mask_h)
per = (time.perf_counter() - t0) * 1e3 / ORACLE_STEPS
print(json.dumps({"variant": "o: brute-force oracle on the host", "steps_timed": ORACLE_STEPS, "ms_per_step": round(per, 1),
                  "s_scaled_to_all_steps": round(per * T / 1e3, 1)}), flush=True)

# (rp) last: the dense (time, ID) variables are 20 arrays of T x N values on the host
if os.environ.get("SHP_DENSE", "1") != "0":
    kw["per_timestep"] = True
    t0 = time.perf_counter()
    dense = marex_amd.event_shapes(ids3, **kw)
    print(json.dumps({"variant": "rp: event_shapes, resident field, per_timestep=True (one run)",
                      "s": round(time.perf_counter() - t0, 2),
                      "dense_GB": round(sum(np.asarray(v.values).nbytes for v in dense.data_vars.values()) / 1e9, 2)}), flush=True)
