"""A host stand-in for the engine call behind ``marex_amd.event_occurrence`` (``HotPath.occurrence``), in NumPy on CPU
tensors: the public path -- validation, labels, windows, the carried state, the host finish -- runs without a GPU in
tests/test_event_occurrence_host.py.  Not collected by pytest."""
import numpy as np
import torch

import occurrence_oracle as oo


class HostEngine:
    device = torch.device("cpu")

    def __init__(self):
        self.calls = []

    def occurrence(self, x, t0=0, grp=None, G=1, sgrp=None, G2=0, cls=None, R=0, runs=True, event_ids=(), acc=None, finish=True):
        a = x.numpy()
        assert a.dtype in (np.uint8, np.int32, np.bool_) and a.ndim == 2
        Tb, C = a.shape
        self.calls.append(("occurrence", str(a.dtype), t0, Tb))
        ids = [int(k) for k in event_ids]
        if acc is None:
            acc = {"cell_cnt": np.zeros((G, C), np.uint32), "runs": np.zeros((3, C), np.uint32) if runs else None,
                   "sec_cnt": np.zeros((G2, R), np.uint64) if sgrp is not None else None, "dur": np.zeros((len(ids), C), np.uint32),
                   "neg": 0}
        g = None if grp is None else np.asarray(grp)[t0:t0 + Tb]
        acc["cell_cnt"] += oo.cell_counts(a, g, G)
        if runs:
            acc["runs"] = oo.run_stats(a, state=acc["runs"])
        if sgrp is not None:
            acc["sec_cnt"] += oo.section_counts(a, np.asarray(sgrp)[t0:t0 + Tb], G2, cls, R)
        for k, e in enumerate(ids):
            acc["dur"][k] += oo.cell_counts(a, match=e)[0]
        acc["neg"] += int((a.astype(np.int64) < 0).sum())
        out = {"acc": acc}
        if finish:
            assert acc["neg"] == 0
            out.update(cell_cnt=acc["cell_cnt"], runs=acc["runs"], sec_cnt=acc["sec_cnt"], dur=acc["dur"])
        return out
