"""A host stand-in for the engine calls behind ``marex_amd.nearest_cell_index`` and ``marex_amd.resample_nearest``
(``HotPath.nearest_index``, ``HotPath.resample_nearest``), in NumPy on CPU tensors, built on tests/nearest_oracle.py: the
public path -- validation, rectilinear expansion, masks, ``max_distance_km``, windows, labels -- runs without a GPU in
tests/test_nearest_resample_host.py.  Not collected by pytest."""
import numpy as np
import torch

import nearest_oracle as no


class HostEngine:
    device = torch.device("cpu")

    def __init__(self):
        self.calls = []

    def nearest_index(self, src, ids, dst, method="brute", voxels=None, max_rings=None, qmax=float("inf")):
        src, dst, ids = np.asarray(src), np.asarray(dst), np.asarray(ids)
        assert src.dtype == np.float64 and src.ndim == 2 and src.shape[0] == 3 and src.flags.c_contiguous
        assert dst.dtype == np.float64 and dst.ndim == 2 and dst.shape[0] == 3 and dst.flags.c_contiguous
        assert ids.dtype == np.int32 and ids.shape == (src.shape[1],) and not np.isnan(src).any()
        assert method in ("brute", "voxel") and qmax >= 0
        assert method == "brute" or (1 <= voxels <= 1024 and 0 <= max_rings <= voxels)
        self.calls.append(("nearest_index", method, voxels if method == "voxel" else 0, max_rings, qmax, src.shape[1], dst.shape[1]))
        index, q = no.brute(src, ids, dst)
        return {"index": index, "q": q, "fallback": 0, "voxels": voxels if method == "voxel" else 0}

    def resample_nearest(self, x, index, out, fill):
        a, i, o = x.numpy(), index.numpy(), out.numpy()
        assert a.ndim == 2 and a.dtype in (np.uint8, np.int32, np.float32) and o.dtype == a.dtype and x.is_contiguous()
        assert i.dtype == np.int32 and i.ndim == 1 and o.shape == (a.shape[0], i.size) and out.is_contiguous()
        assert i.size == 0 or (i.min() >= -1 and i.max() < a.shape[1])
        self.calls.append(("resample_nearest", a.shape[0], a.dtype.name, fill))
        o[...] = no.gather(a, i, fill)
