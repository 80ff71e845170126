"""A host stand-in for the engine call behind ``marex_amd.regional_series`` (``HotPath.regional_series``), in NumPy on CPU
tensors: the public path -- validation, region ranks, the area table, threshold layouts, windows, the carried slots, the
host finish -- runs without a GPU in tests/test_regional_series_host.py.  Not collected by pytest."""
import numpy as np
import torch

from marex_amd.engine import HotPath

import regional_series_oracle as ro


class HostEngine:
    device = torch.device("cpu")
    regional_slot_bytes = staticmethod(HotPath.regional_slot_bytes)

    def __init__(self):
        self.calls = []

    def regional_series(self, x, reg, R, T, t0=0, q=None, wf=None, anom=None, thr=None, doy=None, match=0, acc=None, finish=True):
        a = x.numpy()
        assert a.dtype in (np.uint8, np.int32, np.bool_) and a.ndim == 2
        Tb, C = a.shape
        an = None
        if anom is not None:
            an = anom.numpy()
            assert an.dtype == np.float32 and an.shape == a.shape
        h = None
        if thr is not None:
            assert thr.dtype == torch.float32 and thr.dim() == 2 and thr.shape[1] == C and thr.is_contiguous()
            h = thr.numpy()
        assert np.asarray(reg).dtype == np.int32 and np.asarray(reg).shape == (C,) and 0 < R <= 32767 and t0 + Tb <= T
        assert q is None or (np.asarray(q).dtype == np.int64 and np.asarray(q).shape == (C,))
        assert wf is None or (np.asarray(wf).dtype == np.float32 and an is not None)
        self.calls.append(("regional_series", str(a.dtype), t0, Tb, R, None if h is None else h.shape[0]))
        acc = ro.accumulate(a, reg, R, T, t0, q, wf, an, h, doy, match, state=acc)
        out = {"acc": acc}
        if finish:
            if acc["status"][0]:
                from marex_amd.exceptions import create_data_validation_error

                raise create_data_validation_error("Object IDs must be non-negative")
            assert acc["status"] == [0, 0]
            out.update({k: v for k, v in ro.finish(acc).items() if k != "status"})
        return out
