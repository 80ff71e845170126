"""A host stand-in for the engine call behind ``marex_amd.event_composites`` (``HotPath.event_composites``), in NumPy on CPU
tensors: the public path -- validation, labels, windows with their halo, the host finish -- runs without a GPU in
tests/test_event_composites_host.py.  It sees only the rows it is given, asserts that they cover the halo and that the
windows follow each other.  Not collected by pytest."""
import numpy as np
import torch

import event_composites_oracle as eo


class HostEngine:
    device = torch.device("cpu")

    def __init__(self):
        self.calls = []

    def event_composites(self, x, v, r0, a, b, T, max_lag=10, anchor="onset", grp=None, G=1, acc=None, finish=True):
        xs, vs = x.numpy(), v.numpy()
        assert xs.dtype in (np.uint8, np.bool_) and vs.dtype == np.float32 and xs.ndim == 2 and xs.shape == vs.shape
        Tr, C = xs.shape
        self.calls.append(("event_composites", str(xs.dtype), r0, Tr, a, b))
        H = max(max_lag, 1)
        assert 0 <= a < b <= T and r0 <= max(0, a - H) and r0 + Tr >= min(T, b + H), "the rows must cover the halo"
        assert r0 == max(0, a - H) and r0 + Tr == min(T, b + H), "no more than the halo is fetched"
        if acc is None:
            acc = {"next": 0, "plan": (T, C, max_lag, anchor, G), **eo.zeros(G, C, max_lag)}
        assert acc["next"] == a, "the windows must follow each other"
        assert acc["plan"] == (T, C, max_lag, anchor, G)
        eo.accumulate(acc, xs, vs, r0, a, b, T, max_lag, anchor, grp, G)
        acc["next"] = b
        out = {"acc": acc}
        if finish:
            assert b == T and acc["lost"] == 0
            out.update({k: acc[k] for k in ("anchors", "count", "sum", "sumsq")})
        return out
