"""One-off measurement (not a pytest file): the regional series (``marex_regional_series_u8`` / ``marex_regional_series_i32``)
on a field of the size of cfg2 (``REG_STEPS`` x ``REG_NY`` x ``REG_NX``, default 1826 x 720 x 1440): a 4-5 % mask of smoothed
device noise (the blobby mask of tests/measure_track.py), its anomalies and 366 rows of thresholds; the int32 field is the
mask times a block number, so its coverage is the mask's.  The coverage is reported.

(k) the library call alone, resident inputs, between two device events -- for the region maps R = 1, a dozen blocky basins
    and the 720 grid rows, for the uint8 mask and the int32 field, with and without areas, anomalies and categories;
(c) baseline: device-to-device copies of the mask, of the int32 field and of the anomalies;
(o) the composition it replaces for the counts: ``event_occurrence(zonal=True, zonal_by="step")``, resident mask;
(e) the composition it replaces for the sums: the ``(regions + 1) * mask`` int32 field materialised on the device, then
    ``event_intensity`` on it;
(r) ``marex_amd.regional_series`` on resident inputs with everything: tables, kernel, host finish;
(l) the composition it replaces for the categories: ``local_intensity(zonal=True, zonal_by="step")``, resident inputs;
(b) baseline: the lightest vectorised NumPy equivalent on the host (``np.bincount`` per step: cells and the two sums
    only), timed on the first ``REG_HOST_STEPS`` steps (default 16) and scaled;
(n) baseline: the NumPy oracle of the tests (``tests/regional_series_oracle.py``: integer areas, sums, maximum and
    categories), timed on the first ``REG_ORACLE_STEPS`` steps (default 4) and scaled.

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
from marex_amd.regional import area_weight_table

REPS = 5
T = int(os.environ.get("REG_STEPS", 1826))
ny = int(os.environ.get("REG_NY", 720))
nx = int(os.environ.get("REG_NX", 1440))
HOST_STEPS = min(T, int(os.environ.get("REG_HOST_STEPS", 16)))
C = ny * nx
n = T * C
eng = get_engine(0)
dev = eng.device
print(json.dumps({"device": torch.cuda.get_device_name(0), "reps": REPS, "T": T, "ny": ny, "nx": nx}), flush=True)


def blobby(frac=0.045, seed=1, chunk=128):
    """The mask in chunks of steps (the smoothing needs several copies of its input)."""
    g = torch.Generator(device=dev).manual_seed(seed)
    out = torch.empty((T, C), dtype=torch.uint8, device=dev)
    thr = None
    for a in range(0, T, chunk):
        b = min(T, a + chunk)
        f = torch.randn((1, 1, b - a, ny, nx), generator=g, device=dev)
        for _ in range(2):
            f = torch.nn.functional.avg_pool3d(f, (3, 13, 17), stride=1, padding=(1, 6, 8), count_include_pad=False)
        f = f.reshape(b - a, C)
        if thr is None:
            thr = torch.quantile(f.reshape(-1)[::113][:16_000_000], 1.0 - frac)
        out[a:b] = f > thr
    return out


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


def device_ms(fn, before=lambda: None):
    out = []
    for _ in range(REPS + 1):
        before()
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        eng.sync()
        a.record()
        fn()
        b.record()
        eng.sync()
        out.append(a.elapsed_time(b))
    return out[1:]


mask = blobby()
g = torch.Generator(device=dev).manual_seed(2)
anom = torch.randn((T, C), generator=g, device=dev) + 1.5
thr = torch.rand((366, C), generator=g, device=dev) * 1.5 + 0.3
doy_h = (np.arange(T) % 366).astype(np.int32)
block = (torch.arange(T, device=dev, dtype=torch.int32) // 30 + 1)[:, None]
ids = mask.to(torch.int32) * block
held = int(mask.sum().item())
lines = int(mask.view(T, C // 32, 32).any(dim=2).sum().item()) if C % 32 == 0 else None
print(json.dumps({"present_cells": held, "coverage": round(held / n, 4), "anomaly_lines_with_a_present_cell": lines,
                  "share_of_lines": None if lines is None else round(lines / (n / 32), 4)}), flush=True)

lat = np.linspace(-89.875, 89.875, ny)
area_y = np.cos(np.radians(lat)) * (111.195 * 0.25) ** 2
areas = np.repeat(area_y, nx)
e, q_h = area_weight_table(areas)
q, wf = eng._dev(q_h), eng._dev(areas.astype(np.float32))
MAPS = {"R=1": (np.zeros(C, np.int32), 1),
        "R=12 basins": ((np.repeat(np.arange(ny) // (ny // 3 + 1), nx) * 4 + np.tile(np.arange(nx) // (nx // 4 + 1), ny)).astype(np.int32), 12),
        "R=720 rows": (np.repeat(np.arange(ny, dtype=np.int32), nx), ny)}
doy = eng._dev(doy_h)
results = {}
for mname, (reg_h, R) in MAPS.items():
    reg = eng._dev(reg_h)
    buf = {"area": torch.zeros((T, R), dtype=torch.int64, device=dev), "cnt": torch.zeros((T, R, 2), dtype=torch.int64, device=dev),
           "sums": torch.zeros((T, R, 2), dtype=torch.float64, device=dev), "vmax": torch.zeros((T, R), dtype=torch.int32, device=dev),
           "cat_cnt": torch.zeros((T, R, 6), dtype=torch.int64, device=dev), "cat_area": torch.zeros((T, R, 6), dtype=torch.int64, device=dev),
           "status": torch.zeros(2, dtype=torch.int64, device=dev)}

    def zero():
        for b in buf.values():
            b.zero_()

    def call(x, areas_on, level):
        fn = "marex_regional_series_i32" if x.dtype == torch.int32 else "marex_regional_series_u8"
        an = level >= 1
        cats = level == 2
        eng.call(fn, x, 0, T, C, T, 0, reg, R, q if areas_on else None, wf if areas_on and an else None, anom if an else None,
                 thr if cats else None, doy if cats else None, 366 if cats else 0, buf["area"], buf["cnt"],
                 buf["sums"] if an else None, buf["vmax"] if an else None, buf["cat_cnt"] if cats else None,
                 buf["cat_area"] if cats and areas_on else None, buf["status"])

    for fname, x in (("uint8 mask", mask), ("int32 IDs", ids)):
        for vname, areas_on, level in (("cells", False, 0), ("cells + areas", True, 0), ("areas + anomalies", True, 1),
                                       ("areas + anomalies + categories", True, 2)):
            if x is ids and vname == "cells + areas":
                continue
            ms = device_ms(lambda: call(x, areas_on, level), zero)
            assert buf["status"].cpu().tolist() == [0, 0]
            assert int(buf["cnt"][..., 0].sum().item()) + int(buf["cnt"][..., 1].sum().item()) == held
            results[(mname, fname, vname)] = statistics.median(ms)
            print(json.dumps(dict({"variant": f"k: {fname}, {mname}, {vname}"}, **med(ms),
                                  GB_per_s_on_the_field=round(x.element_size() * n / statistics.median(ms) / 1e6, 1))), flush=True)
    del buf, reg

# (c) device-to-device copies
for name, src in (("uint8 mask", mask), ("int32 IDs", ids), ("float32 anomalies", anom)):
    dst = torch.empty_like(src)
    cp = device_ms(lambda: dst.copy_(src))
    print(json.dumps(dict({"variant": f"c: device-to-device copy of the {name}"}, **med(cp),
                          GB_per_s_read_plus_written=round(2 * src.element_size() * n / statistics.median(cp) / 1e6, 1))), flush=True)
    del dst
torch.cuda.empty_cache()

# (o), (e) the compositions
m3 = mask.view(T, ny, nx)
o = wall(lambda: marex_amd.event_occurrence(m3, zonal=True, zonal_by="step"))
print(json.dumps(dict({"variant": "o: event_occurrence(zonal=True, zonal_by='step'), resident mask (counts per row, with its per-cell maps)"},
                      **med(o))), flush=True)
basins = eng._dev(MAPS["R=12 basins"][0]) + 1
w32 = areas.astype(np.float32)


def composition():
    field = mask.to(torch.int32) * basins[None, :]
    return marex_amd.event_intensity(field, anom, cell_areas=w32)


ev = wall(composition)
print(json.dumps(dict({"variant": "e: (regions + 1) * mask materialised, then event_intensity (12 basins, areas)"}, **med(ev))), flush=True)

# (r) the public call with everything
reg12 = MAPS["R=12 basins"][0].reshape(ny, nx)
days = {"time": ("time", (np.datetime64("2000-01-01") + np.arange(T)).astype("datetime64[ns]"))}
fd = marex_amd.DataArray(m3, dims=("time", "lat", "lon"), coords=days)
res = {}
r = wall(lambda: res.__setitem__("r", marex_amd.regional_series(fd, regions=reg12, cell_areas=area_y, dat_anomaly=anom.view(T, ny, nx),
                                                               thresholds=thr.view(366, ny, nx), by="year")))
print(json.dumps(dict({"variant": "r: regional_series, resident inputs, 12 basins, areas + anomalies + categories, by='year'"}, **med(r))),
      flush=True)
li = wall(lambda: marex_amd.local_intensity(fd, anom.view(T, ny, nx), thresholds=thr.view(366, ny, nx), zonal=True, zonal_by="step"))
print(json.dumps(dict({"variant": "l: local_intensity(zonal=True, zonal_by='step'), resident inputs (category cells per row, with its per-cell maps)"},
                      **med(li))), flush=True)
tot = np.asarray(res["r"]["cells"].values).sum() + np.asarray(res["r"]["invalid_cells"].values).sum()
print(json.dumps({"cells_of_the_public_call": int(tot), "present_cells": held}), flush=True)

# (n) NumPy on the host
mask_h, anom_h = mask[:HOST_STEPS].cpu().numpy(), anom[:HOST_STEPS].cpu().numpy()
reg_h, w64 = MAPS["R=12 basins"][0], w32.astype(np.float64)


def numpy_steps(steps):
    out = []
    for t in range(steps):
        sel = np.nonzero(mask_h[t])[0]
        a = anom_h[t, sel]
        ok = np.isfinite(a)
        sel, a = sel[ok], a[ok].astype(np.float64)
        rr = reg_h[sel]
        out.append((np.bincount(rr, minlength=12), np.bincount(rr, weights=w64[sel], minlength=12),
                    np.bincount(rr, weights=w64[sel] * a, minlength=12)))
    return out


nt = []
for _ in range(3):
    t0 = time.perf_counter()
    numpy_steps(HOST_STEPS)
    nt.append((time.perf_counter() - t0) * 1e3)
per = statistics.median(nt[1:]) / HOST_STEPS
k = results[("R=12 basins", "uint8 mask", "areas + anomalies")]
print(json.dumps({"variant": "b: NumPy on the host, the lightest equivalent (bincount per step: cells, sum w, sum w a; float areas, no maximum, "
                             "no categories)",
                  "steps_timed": HOST_STEPS, "ms_per_step": round(per, 3), "ms_scaled_to_all_steps": round(per * T, 1),
                  "k_over_b": round(k / (per * T), 5)}), flush=True)

# (n) the NumPy oracle of the tests on a slice: integer areas, both sums, the maximum, the categories
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import regional_series_oracle as ro  # noqa: E402

ORACLE_STEPS = min(HOST_STEPS, int(os.environ.get("REG_ORACLE_STEPS", 4)))
thr_h = thr.cpu().numpy()
ot = []
for _ in range(3):
    t0 = time.perf_counter()
    st = ro.accumulate(mask_h[:ORACLE_STEPS], reg_h, 12, ORACLE_STEPS, 0, q_h, w32, anom_h[:ORACLE_STEPS], thr_h, doy_h)
    ot.append((time.perf_counter() - t0) * 1e3)
per = statistics.median(ot[1:]) / ORACLE_STEPS
kc = results[("R=12 basins", "uint8 mask", "areas + anomalies + categories")]
dev_cnt = res["r"]["cells"].values[:ORACLE_STEPS]
print(json.dumps({"variant": "n: the NumPy oracle of the tests (tests/regional_series_oracle.py), 12 basins, areas + anomalies + categories",
                  "steps_timed": ORACLE_STEPS, "ms_per_step": round(per, 3), "ms_scaled_to_all_steps": round(per * T, 1),
                  "k_over_n": round(kc / (per * T), 6),
                  "cells_equal_the_public_call": bool(np.array_equal(st["cnt"][..., 0], np.asarray(dev_cnt)))}), flush=True)
