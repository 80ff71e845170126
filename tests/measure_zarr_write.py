"""One-off measurement (not a pytest file): writing cfg2-shaped arrays (1826 x 720 x 1440, chunks of 25 steps) from HBM
to a Zarr store through the host encoder (slab to host memory, 8 host threads) and through the device encoder (chunks
compressed in HBM, only the frames cross PCIe):

* the extreme mask of the synthetic cfg2 field (bool);
* the tracker's ID_field on a blobby 5 % mask (int32);
* the anomalies (float32).

Per array and path: end-to-end seconds of ``write_array``, compression ratio, bytes over PCIe, and the device
encoder's rate on its own (``HotPath.blosc_compress`` over every chunk, one wave per stream, and the one-lane-per-stream
variant on the first 10 chunks).  Kernel times come from a separate ``rocprofv3 --kernel-trace --stats`` run of this
script with ``--profile`` (device path only).  Files are written under ``--dir`` (default: a temporary directory) and
removed after each array."""
import argparse
import json
import os
import shutil
import sys
import tempfile
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch

from marex_amd import binning, calendar, synth, zarr_io
from marex_amd.detect import get_engine

ap = argparse.ArgumentParser()
ap.add_argument("--dir", default=None)
ap.add_argument("--profile", action="store_true", help="device path only, one pass (for rocprofv3)")
ap.add_argument("--T", type=int, default=3652)
args = ap.parse_args()

ny, nx, W = 720, 1440, 5
hot = get_engine(0)
tm = calendar.daily_time_axis("2015-01-01", args.T)
cal = calendar.build_calendar(tm, window_year_baseline=W)
x = hot.synth_field(synth.make_tables(tm, ny, nx))
r = hot.shifting_hobday(x, hot.upload_calendar(cal), W=W, S=21, bins=binning.hobday_bins(), q=0.95, wd=11, ws=5, ny=ny, nx=nx)
T_out = r["extreme_events"].shape[0]
ext = r["extreme_events"].view(T_out, ny, nx).to(torch.bool)
anom = r["dat_anomaly"].view(T_out, ny, nx)
mask = r["mask"].reshape(1, -1)
del x, r
torch.cuda.empty_cache()


def blobby_ids(frac=0.05, seed=1):
    g = torch.Generator(device=hot.device).manual_seed(seed)
    f = torch.randn((1, 1, T_out, ny, nx), generator=g, device=hot.device)
    for _ in range(2):
        f = torch.nn.functional.avg_pool3d(f, (3, 13, 17), stride=1, padding=(1, 6, 8), count_include_pad=False)
    f = f.reshape(T_out, ny * nx)
    thr = torch.quantile(f.reshape(-1)[:: 113][: 16_000_000], 1.0 - frac)
    b = (f > thr).to(torch.uint8) * mask
    del f
    torch.cuda.empty_cache()
    lab = hot.label_objects_3d(b, ny, nx, True)
    ids = lab["ids"].view(T_out, ny, nx).clone()
    del lab, b
    torch.cuda.empty_cache()
    return ids


ids = blobby_ids()
hot.sync()
chunks = (25, ny, nx)
root = args.dir or tempfile.mkdtemp(prefix="zarr_write_")


def files_bytes(path):
    return sum(os.path.getsize(os.path.join(path, f)) for f in os.listdir(path) if not f.startswith("."))


def encoder_rate(t, variant, n_chunks=None):
    nbytes = int(np.prod(chunks)) * t.element_size()
    n_all = (t.shape[0] + chunks[0] - 1) // chunks[0]
    n = n_all if n_chunks is None else min(n_chunks, n_all)
    B = max(1, zarr_io.DEVICE_BATCH_BYTES // nbytes)
    full = t.shape[0] // chunks[0]
    flat = t[: full * chunks[0]].reshape(full, -1).view(torch.uint8)
    n = min(n, full)
    wsp = {}
    hot.blosc_compress(flat[:1].contiguous(), t.element_size(), variant=variant, wsp=wsp)  # warm-up
    hot.sync()
    t0 = time.perf_counter()
    out = 0
    for b0 in range(0, n, B):
        _, lens = hot.blosc_compress(flat[b0: min(n, b0 + B)], t.element_size(), variant=variant, wsp=wsp)
        out += int(lens.sum())
    dt = time.perf_counter() - t0
    return {"variant": "wave" if variant == 0 else "lane", "chunks": n, "s": round(dt, 3),
            "GB_per_s": round(n * nbytes / dt / 1e9, 1), "ratio": round(n * nbytes / out, 2)}


for name, t in (("extreme mask (bool)", ext), ("ID_field blobby 5 % (int32)", ids), ("anomalies (float32)", anom)):
    raw = t.numel() * t.element_size()
    res = {"array": name, "shape": list(t.shape), "raw_GB": round(raw / 1e9, 3)}
    paths = [("device", True)] if args.profile else [("host", False), ("device", True), ("auto", None)]
    for label, dc in paths:
        p = os.path.join(root, label)
        shutil.rmtree(p, ignore_errors=True)
        hot.sync()
        t0 = time.perf_counter()
        zarr_io.write_array(p, t, chunks, ("time", "lat", "lon"), device_compress=dc)
        dt = time.perf_counter() - t0
        fb = files_bytes(p)
        res[label] = {"s": round(dt, 3), "file_GB": round(fb / 1e9, 4), "ratio": round(raw / fb, 2),
                      "pcie_GB": round((raw if label == "host" else fb) / 1e9, 4)}
    if not args.profile:
        hd, dd = os.path.join(root, "host"), os.path.join(root, "device")
        same = sorted(os.listdir(hd)) == sorted(os.listdir(dd)) and all(
            open(os.path.join(hd, f), "rb").read() == open(os.path.join(dd, f), "rb").read() for f in os.listdir(hd))
        res["identical_files"] = same
        res["encoder"] = [encoder_rate(t, 0), encoder_rate(t, 1, 10), encoder_rate(t, 0, 10)]
    for label, _ in paths:
        shutil.rmtree(os.path.join(root, label), ignore_errors=True)
    print(json.dumps(res), flush=True)
if args.dir is None:
    shutil.rmtree(root, ignore_errors=True)
