"""One-off measurement (not a pytest file): the tracker's object stages on the device --
``calculate_object_properties(["area", "centroid"])`` (``HotPath.object_moments``) and ``find_overlapping_objects``
(``HotPath.overlap_pairs``) -- at the size of cfg2 (1826 x 720 x 1440 after trimming), against the NumPy oracle of
tests/objects_oracle.py on a subset of the slices.

* blobby 5 %: a 5 % mask of smoothed device noise (as tests/measure_track.py), labelled per timestep
  (identify_objects(time_connectivity=False), the input of the reference's merge tracker) and in (t, y, x) (run()'s events);
* worst case: the cfg2 extreme mask of the synthetic field closed with R_fill = 8, T_fill = 2: one giant object per
  timestep, or one event spanning every timestep.

Wall times are per call (the mean of K calls after a warm-up) and include the host side: the sort of the compacted
rows, the float64 division and the device-to-host copies.  Kernel times come from a separate run under
``rocprofv3 --kernel-trace --stats``; ``--skip-oracle`` leaves the host oracle out of such a run."""
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import numpy as np
import torch

import objects_oracle as oo
from marex_amd import binning, calendar, synth
from marex_amd.detect import get_engine

ny, nx, T, W = 720, 1440, 3652, 5
K = 3
ORACLE_SLICES = 20
skip_oracle = "--skip-oracle" in sys.argv
hot = get_engine(0)
tm = calendar.daily_time_axis("2015-01-01", T)
cal = calendar.build_calendar(tm, window_year_baseline=W)
dcal = hot.upload_calendar(cal)
bt = binning.hobday_bins()
x = hot.synth_field(synth.make_tables(tm, ny, nx))
r = hot.shifting_hobday(x, dcal, W=W, S=21, bins=bt, q=0.95, wd=11, ws=5, ny=ny, nx=nx)
ext, mask = r["extreme_events"], r["mask"]
del x, r
torch.cuda.empty_cache()
T_out = ext.shape[0]
CELLS = T_out * ny * nx


def blobby(frac=0.05, seed=1):
    g = torch.Generator(device=hot.device).manual_seed(seed)
    f = torch.randn((1, 1, T_out, ny, nx), generator=g, device=hot.device)
    for _ in range(2):  # two box passes ~ a Gaussian of (1, 6, 8) cells
        f = torch.nn.functional.avg_pool3d(f, (3, 13, 17), stride=1, padding=(1, 6, 8), count_include_pad=False)
    f = f.reshape(T_out, ny * nx)
    thr = torch.quantile(f.reshape(-1)[:: 113][: 16_000_000], 1.0 - frac)
    out = (f > thr).to(torch.uint8) * mask.reshape(1, -1)
    del f
    torch.cuda.empty_cache()
    return out


def timed(fn):
    fn()
    hot.sync()
    t0 = time.perf_counter()
    for _ in range(K):
        res = fn()
    hot.sync()
    return res, (time.perf_counter() - t0) / K


def measure(ids, case):
    ids_gb = ids.numel() * 4 / 1e9
    mom, t_mom = timed(lambda: hot.object_moments(ids, ny, nx, wrap=True))
    ovl, t_ovl = timed(lambda: hot.overlap_pairs(ids))
    row = {"case": case, "ID_field_GB": round(ids_gb, 2), "rows": int(mom["id"].size),
           "distinct_ids": int(np.unique(mom["id"]).size), "overlap_pairs": int(ovl.shape[0]),
           "props_ms": round(t_mom * 1e3, 1), "props_Gcells_per_s": round(CELLS / t_mom / 1e9, 1),
           "overlaps_ms": round(t_ovl * 1e3, 1), "overlaps_Gcells_per_s": round(CELLS / t_ovl / 1e9, 1)}
    if not skip_oracle:
        h = ids[:ORACLE_SLICES].cpu().numpy().reshape(ORACLE_SLICES, ny, nx)
        t0 = time.perf_counter()
        oid, oarea, oc = oo.object_properties(h)
        t1 = time.perf_counter()
        oov = oo.find_overlapping_objects(h)
        t2 = time.perf_counter()
        sub_rows = int(np.searchsorted(mom["t"], ORACLE_SLICES))
        assert np.array_equal(oid, mom["id"][:sub_rows]) and np.array_equal(oc, mom["centroid"][:, :sub_rows])
        sub = hot.overlap_pairs(ids[:ORACLE_SLICES].contiguous())
        assert np.array_equal(sub, oov)
        scale = T_out / ORACLE_SLICES
        row.update({"oracle_slices": ORACLE_SLICES, "oracle_props_ms_scaled": round((t1 - t0) * scale * 1e3),
                    "oracle_overlaps_ms_scaled": round((t2 - t1) * scale * 1e3)})
        if "per-timestep" in case:  # the reference's own form: ids == ID over the slice for every object of one slice
            t0 = time.perf_counter()
            oo.object_properties_slow(h[:1])
            row["oracle_objectwise_ms_per_slice"] = round((time.perf_counter() - t0) * 1e3)
    print(json.dumps(row), flush=True)


def labelled(xb, connect_t):
    lab = hot.label_objects_3d(xb, ny, nx, True, connect_t=connect_t)
    hot.sync()
    ids = lab["ids"]
    del lab
    return ids


worst = hot.fill_time_gaps(hot.fill_holes(ext, mask, ny, nx, 8), mask, ny, nx, 8, 2)
del ext
torch.cuda.empty_cache()
b = blobby()
for name, xb in (("blobby 5 %", b), ("worst: filled cfg2 extreme mask", worst)):
    for connect_t, what in ((False, "per-timestep objects"), (True, "events")):
        ids = labelled(xb, connect_t)
        measure(ids, f"{name}, {what}")
        del ids
        torch.cuda.empty_cache()
