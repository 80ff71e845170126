"""One-off measurement (not a pytest file): the merge tracker (``marex_amd.tracker(..., allow_merging=True)``) stage by
stage on a cfg2-sized grid (720 x 1440) of blobby extremes -- the 5 % mask of smoothed device noise of
tests/measure_track.py.  T = 120 keeps the dense (time x event) outputs small on the host.  Prints the seconds of
run_preprocess and of the three stages of track_objects: per-timestep objects and their properties, split_and_merge and
cluster_rename (stage times of one run after one warm-up run)."""
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch

import marex_amd
from marex_amd.detect import get_engine
from marex_amd.zarr_io import DeviceDataArray

ny, nx, T = 720, 1440, 120
hot = get_engine(0)


def blobby(frac=0.05, seed=1):
    g = torch.Generator(device=hot.device).manual_seed(seed)
    f = torch.randn((1, 1, T, ny, nx), generator=g, device=hot.device)
    for _ in range(2):  # two box passes ~ a Gaussian of (1, 6, 8) cells
        f = torch.nn.functional.avg_pool3d(f, (3, 13, 17), stride=1, padding=(1, 6, 8), count_include_pad=False)
    f = f.reshape(T, ny, nx)
    thr = torch.quantile(f.reshape(-1)[:: 113][: 16_000_000], 1.0 - frac)
    return f > thr


ev = blobby()
tm = np.arange(T).astype("datetime64[D]").astype("datetime64[ns]")
lat = np.linspace(-89.875, 89.875, ny).astype(np.float32)
lon = np.linspace(0.125, 359.875, nx).astype(np.float32)
da = DeviceDataArray(ev, ("time", "lat", "lon"), {"time": tm, "lat": lat, "lon": lon})
mask = np.ones((ny, nx), bool)
for nn in (False, True):
    for rep in range(2):
        trk = marex_amd.tracker(da, mask, R_fill=8, T_fill=2, nn_partitioning=nn, timechunks=10)
        t0 = time.perf_counter()
        pre, stats = trk.run_preprocess()
        hot.sync()
        t_pre = time.perf_counter() - t0
        ds, merges, n = trk.track_objects(pre)
        st = trk._stage_times
    print(f"nn_partitioning={nn}: preprocess {t_pre:.3f} s, objects {st['objects']:.3f} s, "
          f"split_and_merge {st['split_and_merge']:.3f} s, cluster_rename {st['cluster_rename']:.3f} s; "
          f"{stats[2]} objects kept, {n} events, {len(merges['n_parents'].values)} merges", flush=True)
