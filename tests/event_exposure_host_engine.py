"""A host stand-in for the engine call behind ``marex_amd.event_exposure`` (``HotPath.event_exposure``), in NumPy on CPU
tensors: the public path -- validation, region ranks, the area table, windows, the sort and the host finish -- runs without a
GPU in tests/test_event_exposure_host.py.  Not collected by pytest."""
import numpy as np
import torch

from marex_amd.engine import HotPath

import event_exposure_oracle as eo


class HostEngine:
    device = torch.device("cpu")
    exposure_entry_bytes = staticmethod(HotPath.exposure_entry_bytes)

    def __init__(self):
        self.calls = []

    @staticmethod
    def exposure_layout():
        return {"piece": 64, "wave": 512, "wg": 2048, "row_stride": 32, "id_bits": 31, "rank_bits": 16, "step_bits": 17}

    def event_exposure(self, ids, rank, R, t0=0, q=None, wf=None, anom=None, cap=None):
        a = ids.numpy()
        assert a.dtype == np.int32 and a.ndim == 2 and cap is None
        Tb, C = a.shape
        assert 0 < Tb <= 2**17 and 0 < R <= 32767
        rk = rank.numpy()
        assert rk.dtype == np.int32 and rk.shape == (C,)
        an = None
        if anom is not None:
            an = anom.numpy()
            assert an.dtype == np.float32 and an.shape == a.shape
        qh = None if q is None else q.numpy()
        wh = None if wf is None else wf.numpy()
        assert qh is None or (qh.dtype == np.int64 and qh.shape == (C,))
        assert wh is None or (wh.dtype == np.float32 and an is not None)
        self.calls.append(("event_exposure", t0, Tb, R, q is not None, wf is not None, anom is not None))
        if (a < 0).any():
            from marex_amd.exceptions import create_data_validation_error

            raise create_data_validation_error("Object IDs must be non-negative")
        return eo.as_arrays(eo.step_records(a, rk, R, qh, wh, an, t0), an is not None)
