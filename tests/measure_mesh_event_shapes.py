"""One-off measurement (not a pytest file): mesh event shapes (``marex_mesh_event_shapes_i64``) on the field and the mesh of
tests/measure_mesh_objects.py -- a row-triangular mesh of ``MSH_NY`` x ``MSH_NX`` cells (default 1448 x 1448 = 2.1 M) x
``MSH_T`` steps (default 365), a 10 % mask of smoothed device noise, labelled per step on the device and tracked by overlap
(objects of consecutive steps that share a cell are one event: the basic tracker's linking, without its area filter).

(k)  the library call alone, plain (no mask, no lengths, with the coordinate keys), between two device events;
(ka) the same with ``mask`` and ``len_q``;
(z)  control: the plain call on an all-background ID field (4 bytes per cell are read, nothing else);
ablations of (k) by its inputs, nothing in the library is switched: (kb) without the coordinate keys (no box reductions);
(kn) with a neighbour table of -1 (the indices are read, no neighbour ID is gathered);  (k1) on the field with every event
cell renamed to event 1 and one slot per step (the same gathers and reductions, one flush per wave and row);
(i)  yardstick: ``marex_event_intensity_f32`` on the same field and an anomaly field;
(m)  yardstick: ``marex_mesh_object_moments_i64`` on the same field;
(c)  yardstick: a device-to-device copy of the ID field;
(r)  ``marex_amd.mesh_event_shapes`` on the resident field with every table, per_timestep off: the span passes, the kernel,
     the host finish;  (h) the same from a host array;  (f) the host finish alone, and inside it the 128-bit numerators.

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
import marex_amd.shapes_mesh as sm
from marex_amd.detect import get_engine
from marex_amd.engine import HotPath

REPS = 5
NY, NX = int(os.environ.get("MSH_NY", 1448)), int(os.environ.get("MSH_NX", 1448))
T = int(os.environ.get("MSH_T", 365))
C = NY * NX
eng = get_engine(0)
dev = eng.device
print(json.dumps({"device": torch.cuda.get_device_name(0), "reps": REPS, "T": T, "C": C}), flush=True)


def triangular_mesh():
    c = np.arange(C, dtype=np.int64)
    y, x = c // NX, c % NX
    left, right = np.where(x > 0, c - 1, -1), np.where(x < NX - 1, c + 1, -1)
    vert = np.where(x % 2 == 0, np.where(y > 0, c - NX, -1), np.where(y < NY - 1, c + NX, -1))
    return np.stack([left, right, vert]).astype(np.int32)


def blobby(frac=0.10, seed=1):
    g = torch.Generator(device=dev).manual_seed(seed)
    out = torch.empty((T, C), dtype=torch.uint8, device=dev)
    thr = None
    for t0 in range(0, T, 73):  # in pieces: the smoothing holds a few float32 copies
        n = min(73, T - t0)
        f = torch.randn((1, 1, n, NY, NX), generator=g, device=dev)
        for _ in range(2):
            f = torch.nn.functional.avg_pool3d(f, (3, 13, 17), stride=1, padding=(1, 6, 8), count_include_pad=False)
        f = f.reshape(n, C)
        if thr is None:
            thr = torch.quantile(f.reshape(-1)[::37][:16_000_000], 1.0 - frac)
        out[t0:t0 + n] = (f > thr).to(torch.uint8)
        del f
    torch.cuda.empty_cache()
    return out


def track_by_overlap(obj):
    """Event numbers 1 .. N for the objects of ``obj`` (IDs unique in time): objects of consecutive steps sharing a cell are
    one event (union-find on the host over the distinct pairs the device finds)."""
    hi = int(obj.max().item())
    parent = np.arange(hi + 1, dtype=np.int64)

    def find(a):
        while parent[a] != a:
            parent[a] = parent[parent[a]]
            a = parent[a]
        return a

    for t in range(T - 1):
        both = (obj[t] > 0) & (obj[t + 1] > 0)
        pairs = torch.unique(torch.stack([obj[t][both], obj[t + 1][both]], 1), dim=0).cpu().numpy()
        for a, b in pairs:
            ra, rb = find(int(a)), find(int(b))
            if ra != rb:
                parent[max(ra, rb)] = min(ra, rb)
    root = np.array([find(a) for a in range(hi + 1)])
    _, lut = np.unique(root, return_inverse=True)  # root 0 (background) is the smallest: event 0
    return torch.from_numpy(lut.astype(np.int32)).to(dev)[obj.long()]


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


rng = np.random.default_rng(0)
lat = np.degrees(np.arcsin(rng.uniform(-1, 1, C)))
lon = rng.uniform(-180, 180, C)
areas = 10.0 ** rng.uniform(6, 8, C)
edges = rng.uniform(1.0, 10.0, (3, C))
land = rng.random((NY // 8 + 1, NX // 8 + 1)) > 0.3  # blocky land, 30 %
mask_h = np.kron(land, np.ones((8, 8), bool))[:NY, :NX].reshape(-1)
nbr_h = triangular_mesh()
e, q_h = sm.mesh_shape_tables(areas, lat, lon)
_, len_h = sm.mesh_edge_weight_table(edges, C)
lat_k, lon_k = sm.coordinate_keys(lat, lon)
nbr, q, len_q, mask_d = eng._dev(nbr_h), eng._dev(q_h), eng._dev(len_h), eng._dev(mask_h.view(np.uint8))
lat_d, lon_d = eng._dev(lat_k), eng._dev(lon_k)

x = blobby()
t0 = time.perf_counter()
obj = eng.unique_ids_in_time(eng.label_objects_mesh(x, torch.ones(C, dtype=torch.uint8, device=dev), nbr)["ids"])
del x
ids = track_by_overlap(obj).contiguous()
del obj
torch.cuda.empty_cache()
n = T * C
held = int((ids > 0).sum().item())
N = int(ids.max().item())
print(json.dumps({"label_and_link_s": round(time.perf_counter() - t0, 2), "events": N, "cells_with_an_event": held,
                  "coverage": round(held / n, 4)}), flush=True)


def slots_of(field):
    sp = eng.id_spans(field)
    tmin, tmax = sp[0].astype(np.int64), sp[1].astype(np.int64)
    off = HotPath.event_slot_plan(tmin, tmax)
    k = max(int(off[-1]), 1)
    return (tmin.size - 1, eng._dev(np.clip(tmin, 0, 2**31 - 1).astype(np.int32)), eng._dev(off), k,
            torch.zeros((k, 16), dtype=torch.int64, device=dev), torch.zeros((k, 6), dtype=torch.int32, device=dev))


n_ev, tm_d, off_d, slots, mom, box = slots_of(ids)
status = torch.zeros(1, dtype=torch.int64, device=dev)


def prepare():
    mom.zero_()
    status.zero_()
    box[:, 0::2] = 2**31 - 1
    box[:, 1::2] = -2**31


def shapes(f, nb=nbr, m=None, ln=None, la=lat_d, lo=lon_d):
    return lambda: eng.call("marex_mesh_event_shapes_i64", f, 0, T, C, n_ev, tm_d, off_d, slots, nb, m, q, ln, la, lo, mom, box, status)


res = {}
none_nbr = torch.full_like(nbr, -1)
for key, what, launch in (("k", "plain", shapes(ids)), ("ka", "with mask and len_q", shapes(ids, m=mask_d, ln=len_q)),
                          ("kb", "ablation: no coordinate keys", shapes(ids, la=None, lo=None)),
                          ("kn", "ablation: a neighbour table of -1", shapes(ids, nb=none_nbr))):
    res[key] = device_ms(launch, prepare)
    assert int(status.item()) == 0 and int(mom[:, 0].sum().item()) == held
    print(json.dumps(dict({"variant": f"{key}: marex_mesh_event_shapes_i64 alone, {what} (device events)", "slots": slots},
                          **med(res[key]), GB_per_s_on_4_bytes_per_cell=round(4 * n / statistics.median(res[key]) / 1e6, 1))), flush=True)
zero = torch.zeros_like(ids)
z = device_ms(shapes(zero), prepare)
print(json.dumps(dict({"variant": "z: plain call, all-background IDs (reads 4 bytes per cell)"}, **med(z),
                      GB_per_s_on_4_bytes_per_cell=round(4 * n / statistics.median(z) / 1e6, 1))), flush=True)
del zero, none_nbr

# (k1) every event cell renamed to event 1: one slot per step, one flush per wave and row
keep = (n_ev, tm_d, off_d, slots, mom, box)
one = (ids > 0).to(torch.int32)
n_ev, tm_d, off_d, slots, mom, box = slots_of(one)
k1 = device_ms(shapes(one), prepare)
print(json.dumps(dict({"variant": "k1: ablation: plain call, every event cell is event 1 (one flush per wave and row)"}, **med(k1))),
      flush=True)
n_ev, tm_d, off_d, slots, mom, box = keep
del one

# (i) the intensity kernel
g = torch.Generator(device=dev).manual_seed(2)
anom = torch.randn((T, C), generator=g, device=dev) + 1.5
cnt = torch.zeros((slots, 2), dtype=torch.int64, device=dev)
sums = torch.zeros((slots, 2), dtype=torch.float64, device=dev)
vmax = torch.zeros(slots, dtype=torch.int32, device=dev)
i = device_ms(lambda: eng.call("marex_event_intensity_f32", ids, anom, 0, T, C, n_ev, tm_d, off_d, slots, None, cnt, sums, vmax, status),
              lambda: [b.zero_() for b in (cnt, sums, vmax, status)])
print(json.dumps(dict({"variant": "i: marex_event_intensity_f32 alone (device events)"}, **med(i),
                      k_over_i=round(statistics.median(res["k"]) / statistics.median(i), 2),
                      ka_over_i=round(statistics.median(res["ka"]) / statistics.median(i), 2))), flush=True)
del anom, cnt, sums, vmax

# (m) the mesh object moments on the same field: its own spans and slots
o_tmin, _, o_off, o_total = eng._object_spans(ids, T, C, N, "measure", "spans")
o_slots = int(o_total.item())
o_acc = torch.zeros((o_slots, 5), dtype=torch.int64, device=dev)
q4 = q[:4].contiguous()
m = device_ms(lambda: eng.call("marex_mesh_object_moments_i64", ids, T, C, q4, o_tmin, o_off, o_slots, o_acc), o_acc.zero_)
print(json.dumps(dict({"variant": "m: marex_mesh_object_moments_i64 alone (device events)", "slots": o_slots}, **med(m),
                      k_over_m=round(statistics.median(res["k"]) / statistics.median(m), 2))), flush=True)
del o_acc, q4

# (c) device-to-device copy of the ID field
dst = torch.empty_like(ids)
cp = device_ms(lambda: dst.copy_(ids))
print(json.dumps(dict({"variant": "c: device-to-device copy of the ID field (reads 4, writes 4 bytes per cell)"}, **med(cp),
                      GB_per_s_read_plus_written=round(8 * n / statistics.median(cp) / 1e6, 1),
                      k_over_c=round(statistics.median(res["k"]) / statistics.median(cp), 2),
                      ka_over_c=round(statistics.median(res["ka"]) / statistics.median(cp), 2))), flush=True)
del dst, mom, box
torch.cuda.empty_cache()

# (r), (h) the whole call; (f) its host finish
out = {}
kw = dict(cell_areas=areas, edge_lengths=edges, mask=mask_h, per_timestep=False)
r = wall(lambda: out.__setitem__("r", marex_amd.mesh_event_shapes(ids, nbr_h + 1, lat, lon, **kw)))
print(json.dumps(dict({"variant": "r: mesh_event_shapes, resident field, every table, per_timestep=False"}, **med(r))), flush=True)
ids_h = ids.cpu().numpy()
h = wall(lambda: out.__setitem__("h", marex_amd.mesh_event_shapes(ids_h, nbr_h + 1, lat, lon, **kw)))
print(json.dumps(dict({"variant": "h: the same from a host field (uploads 4 bytes per cell)"}, **med(h))), flush=True)
same = all(np.asarray(out["r"][v].values).tobytes() == np.asarray(out["h"][v].values).tobytes() for v in out["r"].data_vars)
print(json.dumps({"resident_and_host_results_same_bytes": same, "rows": int(np.asarray(out["r"]["event_duration"].values).sum())}),
      flush=True)

p = sm._validate(ids, nbr_h + 1, lat, lon, areas, edges, mask_h, 6371.0, False)
sm.tracker_time(p, None)
Nn, tmin_h, off_h, mom_h, box_h = sm._device_slots(eng, ids, p, None)
f = wall(lambda: sm._finish(p, Nn, tmin_h, off_h, mom_h, box_h, False))
here = mom_h[mom_h[:, 0] > 0]
t0 = time.perf_counter()
for _ in range(REPS):
    for col, a, b in ((5, 2, 2), (6, 3, 3), (7, 4, 4), (8, 2, 3), (9, 2, 4), (10, 3, 4)):
        sm.exact_numerator(here[:, 1], here[:, col], here[:, a], here[:, b])
num_ms = (time.perf_counter() - t0) * 1e3 / REPS
t0 = time.perf_counter()
sm._validate(ids, nbr_h + 1, lat, lon, areas, edges, mask_h, 6371.0, False)
val_ms = (time.perf_counter() - t0) * 1e3
print(json.dumps(dict({"variant": "f: the host finish alone (per_timestep=False)", "rows": int(here.shape[0]),
                       "of_which_128_bit_numerators_ms": round(num_ms, 3), "validation_and_tables_ms": round(val_ms, 3)}, **med(f))),
      flush=True)
