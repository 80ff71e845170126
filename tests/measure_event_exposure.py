"""One-off measurement (not a pytest file): the event exposure (``marex_event_exposure_count_i32`` /
``marex_event_exposure_i32``) on a tracked field of the size of cfg2 (``EXP_STEPS`` x ``EXP_NY`` x ``EXP_NX``, default 1826 x
720 x 1440): the blobby 5 % mask of the other ``measure_*`` scripts, tracked by the basic tracker, its anomalies, cos-latitude
areas, and two region maps -- a dozen blocky basins and the 720 grid rows.

(k) per region map, resident inputs, between two device events: the count pass; the whole insert call (zeroing the table,
    the insert pass, the compaction) for the cells alone, with areas and with areas and anomalies; the last on one step at
    the same table size (zeroing and compaction alone, so that the insert pass is the difference); the runs, the distinct
    keys and the table's bytes;
(c) baseline: device-to-device copies of the ID field, and of the ID field plus the anomalies;
(i) ``marex_event_intensity_f32`` and (g) ``marex_regional_series_i32`` alone on the same inputs;
(r) ``marex_amd.event_exposure`` from resident and (h) from host inputs: tables, both passes, sort, host finish;
(e) the composition it replaces where the combined ID fits int32: ``(id - 1) (R + 1) + rank + 1`` materialised in torch,
    then ``event_intensity``;
(n) the NumPy oracle of the tests on the first ``EXP_ORACLE_STEPS`` steps (default 2), scaled.

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
T = int(os.environ.get("EXP_STEPS", 1826))
ny = int(os.environ.get("EXP_NY", 720))
nx = int(os.environ.get("EXP_NX", 1440))
ORACLE_STEPS = min(T, int(os.environ.get("EXP_ORACLE_STEPS", 2)))
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


field = blobby()
lat, lon = np.linspace(-89.875, 89.875, ny), np.linspace(0.125, 359.875, nx)
da = DeviceDataArray(field.view(T, ny, nx), ("time", "lat", "lon"), {"time": np.arange(T), "lat": lat, "lon": lon})
t0 = time.perf_counter()
events = marex_amd.tracker(da, np.ones((ny, nx), bool), R_fill=2, T_fill=2, area_filter_quartile=0.5, allow_merging=False).run()
print(json.dumps({"tracker_run_s": round(time.perf_counter() - t0, 2)}), flush=True)
del field, da
ids_h = np.ascontiguousarray(np.asarray(events["ID_field"].values).reshape(T, C), dtype=np.int32)
del events
ids = torch.from_numpy(ids_h).to(dev)
held = int((ids > 0).sum().item())
N = int(ids.max().item())
print(json.dumps({"events": N, "cells_with_an_event": held, "coverage": round(held / n, 4)}), flush=True)
g = torch.Generator(device=dev).manual_seed(2)
anom = torch.randn((T, C), generator=g, device=dev) + 1.5
area_y = np.cos(np.radians(lat)) * (111.195 * 0.25) ** 2
areas = np.repeat(area_y, nx)
e, q_h = area_weight_table(areas)
q, wf = eng._dev(q_h), eng._dev(areas.astype(np.float32))
MAPS = {"R=12 basins": ((np.repeat(np.arange(ny) // (ny // 3 + 1), nx) * 4 + np.tile(np.arange(nx) // (nx // 4 + 1), ny)).astype(np.int32), 12),
        "R=720 rows": (np.repeat(np.arange(ny, dtype=np.int32), nx), ny)}
status = torch.zeros(8, dtype=torch.int64, device=dev)
res = {}

# (k) the kernels
for mname, (reg_h, R) in MAPS.items():
    reg = eng._dev(reg_h)
    cms = device_ms(lambda: eng.call("marex_event_exposure_count_i32", ids, T, C, reg, R, status))
    s = status.cpu().numpy()
    runs = int(s[2])
    assert int(s[4]) == held and int(s[0]) == 0
    cap = HotPath.exposure_cap(runs)
    per = HotPath.exposure_entry_bytes(True, True)
    tab = {k: torch.empty((cap,) + tail, dtype=dt, device=dev) for k, tail, dt in (("keys", (), torch.int64), ("cnt", (), torch.int64),
                                                                                    ("area", (), torch.int64), ("sums", (2,), torch.float64),
                                                                                    ("vmax", (), torch.int32))}
    out = {k: torch.empty((runs,) + tuple(v.shape[1:]), dtype=v.dtype, device=dev) for k, v in tab.items()}

    def insert(x, a, steps, areas_on=True):
        on = a is not None
        return lambda: eng.call("marex_event_exposure_i32", x, steps, C, reg, R, q if areas_on else None, wf if on else None, a, cap,
                                tab["keys"], tab["cnt"], tab["area"] if areas_on else None, tab["sums"] if on else None,
                                tab["vmax"] if on else None, status, runs, out["keys"], out["cnt"], out["area"] if areas_on else None,
                                out["sums"] if on else None, out["vmax"] if on else None)

    bare = device_ms(insert(ids, None, T, False))
    with_area = device_ms(insert(ids, None, T))
    whole = device_ms(insert(ids, anom, T))
    s = status.cpu().numpy()
    keys = int(s[3])
    assert int(s[1]) == 0 and 0 < keys <= runs
    assert int((out["cnt"][:keys] & 0xFFFFFFFF).sum().item()) == held
    rest = device_ms(insert(ids[:1], anom[:1], 1))
    res[mname] = statistics.median(cms) + statistics.median(whole)
    print(json.dumps({"variant": f"k: {mname}", "runs": runs, "distinct_keys": keys, "cap": cap, "entry_bytes": per,
                      "table_bytes": per * cap, "compacted_bytes": per * runs, "count_pass": med(cms),
                      "insert_call_cells_only": med(bare), "insert_call_with_areas": med(with_area), "insert_call": med(whole),
                      "zeroing_and_compaction_alone": med(rest),
                      "insert_pass_ms_by_difference": round(statistics.median(whole) - statistics.median(rest), 3),
                      "count_GB_per_s_on_the_ids": round(4 * n / statistics.median(cms) / 1e6, 1),
                      "insert_GB_per_s_on_the_ids": round(4 * n / (statistics.median(whole) - statistics.median(rest)) / 1e6, 1)}), flush=True)
    del tab, out, reg
torch.cuda.empty_cache()

# (c) device-to-device copies
dst, dst2 = torch.empty_like(ids), torch.empty_like(anom)
cp = device_ms(lambda: dst.copy_(ids))
cp2 = device_ms(lambda: (dst.copy_(ids), dst2.copy_(anom)))
print(json.dumps({"variant": "c: device-to-device copy of the ID field; of the ID field and the anomalies", "ids": med(cp), "both": med(cp2),
                  "GB_per_s_read_plus_written": round(8 * n / statistics.median(cp) / 1e6, 1)}), flush=True)
del dst, dst2
torch.cuda.empty_cache()

# (i) the intensity kernel, (g) the regional series kernel
sp = eng.id_spans(ids)
tmin, tmax = sp[0].astype(np.int64), sp[1].astype(np.int64)
off = HotPath.event_slot_plan(tmin, tmax)
slots = max(int(off[-1]), 1)
tm_d, off_d = eng._dev(np.clip(tmin, 0, 2**31 - 1).astype(np.int32)), eng._dev(off)
cnt = torch.zeros((slots, 2), dtype=torch.int64, device=dev)
sums = torch.zeros((slots, 2), dtype=torch.float64, device=dev)
vmax = torch.zeros(slots, dtype=torch.int32, device=dev)
st1 = torch.zeros(1, dtype=torch.int64, device=dev)
i = device_ms(lambda: eng.call("marex_event_intensity_f32", ids, anom, 0, T, C, N, tm_d, off_d, slots, wf, cnt, sums, vmax, st1),
              lambda: [b.zero_() for b in (cnt, sums, vmax, st1)])
print(json.dumps(dict({"variant": "i: marex_event_intensity_f32 alone, weights (device events)", "slots": slots}, **med(i))), flush=True)
del cnt, sums, vmax
for mname, (reg_h, R) in MAPS.items():
    reg = eng._dev(reg_h)
    buf = {"area": torch.zeros((T, R), dtype=torch.int64, device=dev), "cnt": torch.zeros((T, R, 2), dtype=torch.int64, device=dev),
           "sums": torch.zeros((T, R, 2), dtype=torch.float64, device=dev), "vmax": torch.zeros((T, R), dtype=torch.int32, device=dev),
           "status": torch.zeros(2, dtype=torch.int64, device=dev)}
    gms = device_ms(lambda: eng.call("marex_regional_series_i32", ids, 0, T, C, T, 0, reg, R, q, wf, anom, None, None, 0, buf["area"],
                                     buf["cnt"], buf["sums"], buf["vmax"], None, None, buf["status"]),
                    lambda: [b.zero_() for b in buf.values()])
    print(json.dumps(dict({"variant": f"g: marex_regional_series_i32 alone, {mname}, areas + anomalies (device events)"}, **med(gms),
                          exposure_kernels_over_g=round(res[mname] / statistics.median(gms), 2),
                          exposure_kernels_over_i=round(res[mname] / statistics.median(i), 2))), flush=True)
    del buf, reg
torch.cuda.empty_cache()

# (r), (h) the whole call; (e) the composition it replaces
ids3, anom3 = ids.view(T, ny, nx), anom.view(T, ny, nx)
w32 = areas.astype(np.float32)
for mname, (reg_h, R) in MAPS.items():
    reg2 = reg_h.reshape(ny, nx)
    keep = {}
    r = wall(lambda: keep.__setitem__("ds", marex_amd.event_exposure(ids3, reg2, cell_areas=area_y, dat_anomaly=anom3)))
    ds = keep["ds"]
    print(json.dumps(dict({"variant": f"r: event_exposure, resident inputs, {mname}, areas + anomalies",
                           "pairs": int(np.asarray(ds["pair_ID"].values).size),
                           "cell_steps": int(np.asarray(ds["pair_cell_steps"].values).sum()), "cells_with_an_event": held}, **med(r))),
          flush=True)
    rank_d = eng._dev(reg_h)

    def composition():
        combined = torch.where(ids > 0, (ids - 1) * (R + 1) + rank_d[None, :] + 1, 0)
        return marex_amd.event_intensity(combined, anom, cell_areas=w32)

    if N * (R + 1) + R + 1 >= 2**31:
        print(json.dumps({"variant": f"e: the composition, {mname}", "skipped": "the combined ID does not fit int32"}), flush=True)
    elif N * (R + 1) > 2**22:  # event_intensity keeps dense tables per combined ID on the host: not at tens of millions
        print(json.dumps({"variant": f"e: the composition, {mname}", "combined_ids": N * (R + 1),
                          "skipped": "event_intensity's per-ID host tables for this many combined IDs exceed the host's memory"}),
              flush=True)
    else:
        try:
            ev = wall(composition)
            print(json.dumps(dict({"variant": f"e: the combined ID field materialised, then event_intensity, {mname}"}, **med(ev),
                                  r_over_e=round(statistics.median(r) / statistics.median(ev), 3),
                                  spread_r=round(max(r) - min(r), 1), spread_e=round(max(ev) - min(ev), 1))), flush=True)
        except Exception as err:  # the slots of the combined IDs may not fit
            print(json.dumps({"variant": f"e: the composition, {mname}", "failed": f"{type(err).__name__}: {err}"[:300]}), flush=True)
    del rank_d
    torch.cuda.empty_cache()
anom_h = anom.cpu().numpy().reshape(T, ny, nx)
reg2 = MAPS["R=12 basins"][0].reshape(ny, nx)
h = wall(lambda: marex_amd.event_exposure(ids_h.reshape(T, ny, nx), reg2, cell_areas=area_y, dat_anomaly=anom_h, block_steps="auto"))
print(json.dumps(dict({"variant": "h: event_exposure, host inputs, R=12 basins, areas + anomalies"}, **med(h))), flush=True)

# (n) the NumPy oracle of the tests on a slice
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import event_exposure_oracle as eo  # noqa: E402

ot = []
for _ in range(2):
    t0 = time.perf_counter()
    recs = eo.step_records(ids_h[:ORACLE_STEPS], MAPS["R=12 basins"][0], 12, q_h, w32, anom_h.reshape(T, C)[:ORACLE_STEPS])
    ot.append((time.perf_counter() - t0) * 1e3)
per = min(ot) / ORACLE_STEPS
print(json.dumps({"variant": "n: the NumPy oracle of the tests (tests/event_exposure_oracle.py), R=12 basins, areas + anomalies",
                  "steps_timed": ORACLE_STEPS, "records": len(recs), "ms_per_step": round(per, 1),
                  "ms_scaled_to_all_steps": round(per * T, 1), "kernels_over_n": round(res["R=12 basins"] / (per * T), 7)}), flush=True)
