"""A host stand-in for the engine calls behind ``marex_amd.cell_trends`` (``HotPath.trend_stats`` / ``HotPath.trend_select``),
answered from the NumPy oracle on CPU tensors: the public path -- validation, the abscissae, the conversion, the ranks, the
host finish, the way back to the spatial dimensions -- runs without a GPU in tests/test_cell_trends_host.py.  Not collected
by pytest."""
import numpy as np
import torch

import trends_oracle as to


class HostEngine:
    device = torch.device("cpu")

    def __init__(self):
        self.calls = []

    @staticmethod
    def _check(y, x):
        assert isinstance(y, torch.Tensor) and isinstance(x, torch.Tensor)
        assert y.dtype == torch.float64 and x.dtype == torch.float64 and y.dim() == 2 and x.dim() == 1
        assert y.is_contiguous() and x.is_contiguous() and x.shape[0] == y.shape[0]
        return y.numpy(), x.numpy()

    def trend_stats(self, y, x):
        yv, xv = self._check(y, x)
        self.calls.append(("trend_stats", tuple(yv.shape), y.data_ptr()))
        return {k: torch.from_numpy(np.ascontiguousarray(v)) for k, v in to.stats(yv, xv).items()}

    def trend_select(self, y, x, ranks):
        yv, xv = self._check(y, x)
        r = ranks.numpy() if isinstance(ranks, torch.Tensor) else np.asarray(ranks)
        assert r.dtype == np.int32 and r.ndim == 2 and r.shape[1] == yv.shape[1]
        self.calls.append(("trend_select", tuple(r.shape), y.data_ptr()))
        return torch.from_numpy(to.select(yv, xv, r))
