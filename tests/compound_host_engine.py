"""A host stand-in for the engine call behind ``marex_amd.compound_events`` (``HotPath.compound``), in NumPy on CPU
tensors: the public path -- validation, labels, windows, the carried state, the joint mask, the host finish -- runs without
a GPU in tests/test_compound_events_host.py.  It also answers ``occurrence`` (tests/occurrence_host_engine.py), so that the
joint mask can go on to ``event_occurrence``.  Not collected by pytest."""
import numpy as np
import torch

import compound_oracle as co
from occurrence_host_engine import HostEngine as OccurrenceHostEngine


class HostEngine(OccurrenceHostEngine):
    def compound(self, a, b, t0=0, max_lag=0, tolerance=0, grp=None, G=1, sgrp=None, G2=0, cls=None, R=0, mask=None, acc=None,
                 finish=True):
        x, y = a.numpy(), b.numpy()
        assert x.dtype in (np.uint8, np.bool_) and y.dtype in (np.uint8, np.bool_) and x.ndim == 2 and x.shape == y.shape
        Tb, C = x.shape
        self.calls.append(("compound", str(x.dtype), str(y.dtype), t0, Tb))
        seen = 0 if acc is None else acc["state"]["A"].shape[0]
        assert seen == t0, "the windows must follow each other"
        r = co.compound(x, y, max_lag, tolerance, grp, G, sgrp, G2, cls, R, state=None if acc is None else acc["state"])
        if mask is not None:
            assert mask.dtype == torch.uint8 and tuple(mask.shape)[1] == C and mask.shape[0] >= t0 + Tb
            mask[t0:t0 + Tb] = torch.from_numpy(((x != 0) & (y != 0)).astype(np.uint8))
        out = {"acc": {"state": r.pop("state")}}
        if finish:
            out.update(r)
        return out
