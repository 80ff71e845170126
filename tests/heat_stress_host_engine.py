"""A host stand-in for the engine calls behind ``marex_amd.heat_stress`` and ``marex_amd.monthly_maximum_climatology``
(``HotPath.group_mean``, ``HotPath.heat_stress``), in NumPy on CPU tensors, built on the row loops of
tests/heat_stress_oracle.py: the public path -- validation, labels, windows with their history rows, the carried state, the
host finish -- runs without a GPU in tests/test_heat_stress_host.py.  Not collected by pytest."""
import numpy as np
import torch

import heat_stress_oracle as ho


class HostEngine:
    device = torch.device("cpu")

    def __init__(self):
        self.calls = []

    def group_mean(self, x, lab, G, t0=0, acc=None, finish=True):
        a = x.numpy()
        assert a.dtype == np.float32 and a.ndim == 2
        self.calls.append(("group_mean", t0, a.shape[0]))
        acc = ho.group_walk(a, t0, lab, G, state=acc)
        out = {"acc": acc}
        if finish:
            assert acc["status"] == 0
            out.update(sum=acc["sum"], cnt=acc["cnt"])
        return out

    def heat_stress(self, x, mmm, t0=0, lead=0, window=84, hotspot_min=1.0, steps_per_week=7.0, levels=(4.0, 8.0), grp=None, G=1,
                    dhw=None, alert=None, summary=True, acc=None, finish=True):
        a = x.numpy()
        assert a.dtype == np.float32 and a.ndim == 2 and lead == min(window, t0) and a.shape[0] > lead
        assert np.asarray(mmm).dtype == np.float32 and np.asarray(mmm).shape == (a.shape[1],)
        assert dhw is None or (dhw.dtype == torch.float32 and dhw.shape[0] >= t0 + a.shape[0] - lead)
        assert alert is None or (alert.dtype == torch.uint8 and alert.shape[0] >= t0 + a.shape[0] - lead)
        if acc is not None:
            assert acc["next"] == t0
        self.calls.append(("heat_stress", t0, lead, a.shape[0] - lead))
        nxt = t0 + a.shape[0] - lead
        acc = ho.walk(a, np.asarray(mmm), t0, lead, window, hotspot_min, steps_per_week, levels, grp, G,
                      None if dhw is None else dhw.numpy(), None if alert is None else alert.numpy(), state=acc)
        acc["next"] = nxt
        out = {"acc": acc}
        if finish:
            assert acc["status"] == 0
            out.update({k: acc[k] for k in ho.SUMMARY})
        return out
