"""A host stand-in for the engine call behind ``marex_amd.local_intensity`` (``HotPath.local_intensity``), in NumPy on CPU
tensors: the public path -- validation, labels, threshold layouts, windows, the carried accumulators, the host finish --
runs without a GPU in tests/test_local_intensity_host.py.  Not collected by pytest."""
import numpy as np
import torch

import local_intensity_oracle as lo


class HostEngine:
    device = torch.device("cpu")

    def __init__(self):
        self.calls = []

    def local_intensity(self, x, anom, t0=0, grp=None, G=1, thr=None, doy=None, sgrp=None, G2=0, cls=None, R=0, acc=None,
                        finish=True, match=0):
        a, an = x.numpy(), anom.numpy()
        assert a.dtype in (np.uint8, np.int32, np.bool_) and a.ndim == 2 and an.dtype == np.float32 and an.shape == a.shape
        Tb, C = a.shape
        h = None
        if thr is not None:
            assert thr.dtype == torch.float32 and thr.dim() == 2 and thr.shape[1] == C and thr.is_contiguous()
            h = thr.numpy()
        self.calls.append(("local_intensity", str(a.dtype), t0, Tb, None if h is None else h.shape[0]))
        acc = lo.accumulate(a, an, t0, grp, G, h, doy, sgrp, G2, cls, R, match, state=acc)
        out = {"acc": acc}
        if finish:
            assert acc["status"] == [0, 0] or acc["status"][0]
            if acc["status"][0]:
                from marex_amd.exceptions import create_data_validation_error

                raise create_data_validation_error("Object IDs must be non-negative")
            f = lo.finish(acc)
            out.update(days=f["days"], invalid=f["invalid"], sum=f["sum"], vmax=f["vmax"], tmax=f["tmax"], cat_days=f["cat_days"],
                       sec_cnt=f["sec_cnt"])
        return out
