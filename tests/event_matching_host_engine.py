"""A host stand-in for the engine call behind ``marex_amd.event_matching`` (``HotPath.event_matching``), in NumPy on CPU
tensors: the public path -- validation, the area table, windows, the sort and the host finish -- runs without a GPU in
tests/test_event_matching_host.py.  Not collected by pytest."""
import numpy as np
import torch

from marex_amd.engine import HotPath

import event_matching_oracle as mo


class HostEngine:
    device = torch.device("cpu")
    matching_entry_bytes = staticmethod(HotPath.matching_entry_bytes)
    matching_widths = staticmethod(HotPath.matching_widths)

    def __init__(self):
        self.calls = []

    def event_matching(self, ids_a, ids_b, t0=0, q=None, cap=None):
        a, b = ids_a.numpy(), ids_b.numpy()
        assert a.dtype == np.int32 and b.dtype == np.int32 and a.ndim == 2 and a.shape == b.shape and cap is None
        Tb, C = a.shape
        assert Tb > 0 and C > 0
        qh = None if q is None else q.numpy()
        assert qh is None or (qh.dtype == np.int64 and qh.shape == (C,))
        self.calls.append(("event_matching", t0, Tb, q is not None))
        for x, name in ((a, "ID_field_a"), (b, "ID_field_b")):
            if (x < 0).any():
                from marex_amd.exceptions import create_data_validation_error

                raise create_data_validation_error("Object IDs must be non-negative",
                                                   details=f"{name}: {int((x < 0).sum())} negative cells; 0 is background")
        r = mo.as_arrays(mo.step_records(a, b, qh, t0))
        widths = self.matching_widths(int(a.max()), int(b.max()), Tb) if r["t"].size else None
        return dict(r, runs=int(r["t"].size), cap=0, table_bytes=0, widths=widths)
