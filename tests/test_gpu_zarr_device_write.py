"""GPU: stores written from device tensors (compressed in HBM, only the frames cross PCIe) are identical file for file,
metadata included, to stores written through the host encoder -- write_array, write_dataset and to_zarr, bool / int32 /
float32 with NaN, edge chunks in every dimension, the tracker's run_preprocess output on the reference fixture, the
decoded reference fixture arrays and a 120 x 720 x 1440 field -- and read back with read_array and read_array_to_device."""
import os
import sys

import numpy as np
import pytest
import torch

import marex_amd
from marex_amd import zarr_io
from marex_amd.exceptions import DataValidationError
from marex_amd.xr_compat import DataArray, _MiniDataArray, _MiniDataset

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
FIX = os.path.join(HERE, "golden", "ref_fixtures")

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def hot():
    from marex_amd.detect import get_engine

    return get_engine(0)


def tree(root):
    out = {}
    for d, _, files in os.walk(root):
        for f in files:
            p = os.path.join(d, f)
            out[os.path.relpath(p, root)] = open(p, "rb").read()
    return out


def same_trees(a, b):
    ta, tb = tree(a), tree(b)
    assert sorted(ta) == sorted(tb)
    for k in ta:
        assert ta[k] == tb[k], k
    return ta


def fields(rng, shape):
    f = rng.normal(size=shape).astype(np.float32)
    f[rng.random(shape) < 0.1] = np.nan
    f[..., :3] = np.nan
    m = rng.random(shape) < 0.07
    i = np.where(m, rng.integers(1, 500, shape), 0).astype(np.int32)
    return {"mask": m, "ids": i, "anom": f}


def test_write_array_device_equals_host(hot, tmp_path):
    rng = np.random.default_rng(0)
    for name, a in fields(rng, (53, 37, 61)).items():
        t = torch.from_numpy(a).to(hot.device)
        for ch in [(25, 37, 61), (10, 16, 32), (53, 37, 61), (7, 37, 20)]:
            d, h = str(tmp_path / f"{name}_{ch}_d"), str(tmp_path / f"{name}_{ch}_h")
            md = zarr_io.write_array(d, t, ch, ("time", "lat", "lon"), {"a": 1}, device_compress=True)
            mh = zarr_io.write_array(h, t, ch, ("time", "lat", "lon"), {"a": 1}, device_compress=False)
            assert md == mh
            same_trees(d, h)
            assert np.array_equal(zarr_io.read_array(d), a, equal_nan=True)
            if ch[1:] == a.shape[1:]:
                back = zarr_io.read_array_to_device(d, hot).cpu().numpy()
                assert np.array_equal(back.astype(a.dtype), a, equal_nan=True)
        # the automatic choice gives the same files too
        auto = str(tmp_path / f"{name}_auto")
        zarr_io.write_array(auto, t, (25, 37, 61), ("time", "lat", "lon"), {"a": 1})
        same_trees(auto, str(tmp_path / f"{name}_(25, 37, 61)_h"))


def test_device_compress_true_needs_a_gpu_tensor(tmp_path):
    with pytest.raises(DataValidationError):
        zarr_io.write_array(str(tmp_path / "a"), np.zeros((4, 4), np.float32), device_compress=True)
    t = torch.zeros((4, 4), device="cuda")
    with pytest.raises(DataValidationError):
        zarr_io.write_array(str(tmp_path / "b"), t, compress=False, device_compress=True)
    zarr_io.write_array(str(tmp_path / "c"), t, compress=False)  # uncompressed: the host path, as before
    assert np.array_equal(zarr_io.read_array(str(tmp_path / "c")), np.zeros((4, 4), np.float32))


def _dataset(arrs, dev):
    tm = np.arange("2000-01-01", "2000-02-23", dtype="datetime64[D]")
    lat, lon = np.linspace(-60, 60, 37), np.linspace(0, 358, 61)
    coords = {"time": tm, "lat": lat, "lon": lon}
    vars_ = {}
    for k, a in arrs.items():
        data = torch.from_numpy(a).to(dev)
        vars_[k] = _MiniDataArray(data, ("time", "lat", "lon"), coords, k, {"units": k})
    return _MiniDataset(vars_, {k: _MiniDataArray(v, (k,), None, k, {}) for k, v in coords.items()}, {"source": "test"})


def test_write_dataset_and_to_zarr_device_equals_host(hot, tmp_path):
    ds = _dataset(fields(np.random.default_rng(1), (53, 37, 61)), hot.device)
    zarr_io.write_dataset(str(tmp_path / "d.zarr"), ds, device_compress=True)
    zarr_io.write_dataset(str(tmp_path / "h.zarr"), ds, device_compress=False)
    same_trees(str(tmp_path / "d.zarr"), str(tmp_path / "h.zarr"))
    ds.to_zarr(str(tmp_path / "z.zarr"), mode="w", chunks={"time": 10})
    zarr_io.write_dataset(str(tmp_path / "zh.zarr"), ds, {"time": 10}, device_compress=False)
    files = same_trees(str(tmp_path / "z.zarr"), str(tmp_path / "zh.zarr"))
    assert "mask/5.0.0" in files
    back = zarr_io.read_dataset(str(tmp_path / "z.zarr"))
    assert np.array_equal(back["ids"].values, ds["ids"].data.cpu().numpy())


def test_tracker_preprocess_output_and_reference_fixture_arrays(hot, tmp_path):
    from test_track_host import load_fixture

    ev, mask, lat, lon, tm = load_fixture(False)
    da = DataArray(ev, dims=("time", "lat", "lon"), coords={"time": tm, "lat": lat, "lon": lon})
    trk = marex_amd.tracker(da, DataArray(mask, dims=("lat", "lon")), R_fill=2, T_fill=2, area_filter_quartile=0.5,
                            allow_merging=False)
    pre, _ = trk.run_preprocess()
    t = pre.device_tensor
    assert t.is_cuda
    for ch in [(25,) + tuple(t.shape[1:]), (4, 20, 30)]:
        d, h = str(tmp_path / f"pre{ch}_d"), str(tmp_path / f"pre{ch}_h")
        zarr_io.write_array(d, t, ch, pre.dims, device_compress=True)
        zarr_io.write_array(h, t, ch, pre.dims, device_compress=False)
        same_trees(d, h)
        assert np.array_equal(zarr_io.read_array(d).astype(bool), t.cpu().numpy().astype(bool))
    for store in ("extremes_gridded.zarr", "sst_gridded.zarr"):
        root = os.path.join(FIX, store)
        for v in sorted(os.listdir(root)):
            p = os.path.join(root, v)
            if not os.path.exists(os.path.join(p, ".zarray")):
                continue
            a = zarr_io.read_array(p)
            if a.ndim == 0 or a.dtype.kind not in "biuf":
                continue
            t = torch.from_numpy(np.ascontiguousarray(a)).to(hot.device)
            ch = tuple(min(25, n) if k == 0 else n for k, n in enumerate(a.shape))
            d, h = str(tmp_path / f"{store}_{v}_d"), str(tmp_path / f"{store}_{v}_h")
            zarr_io.write_array(d, t, ch, device_compress=True)
            zarr_io.write_array(h, a, ch)
            same_trees(d, h)
            assert np.array_equal(zarr_io.read_array(d), a, equal_nan=True)


def test_full_size_fields(hot, tmp_path):
    """120 x 720 x 1440 int32 IDs (blobby, mostly zeros) and float32 anomalies: byte-identical to the host path."""
    g = torch.Generator(device=hot.device).manual_seed(3)
    shape = (120, 720, 1440)
    blob = torch.nn.functional.avg_pool2d(torch.rand(shape, device=hot.device, generator=g), 9, 1, 4) > 0.56
    ids = torch.where(blob, (torch.arange(shape[0] * shape[1] * shape[2], device=hot.device, dtype=torch.int64).view(shape)
                             // 100003 % 7000 + 1).to(torch.int32), torch.zeros((), dtype=torch.int32, device=hot.device))
    anom = torch.round(torch.randn(shape, device=hot.device, generator=g) * 100) / 100
    anom[:, :60] = float("nan")
    for name, t in (("ids", ids), ("anom", anom)):
        d, h = str(tmp_path / f"{name}_d"), str(tmp_path / f"{name}_h")
        zarr_io.write_array(d, t, (25, 720, 1440), device_compress=True)
        zarr_io.write_array(h, t, (25, 720, 1440), device_compress=False)
        files = same_trees(d, h)
        assert len(files) == 2 + 5
        del files
