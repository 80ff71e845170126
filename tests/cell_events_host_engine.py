"""A host stand-in for the engine calls behind ``marex_amd.cell_events`` (``HotPath.cell_events`` and
``HotPath.cell_event_records``), in NumPy on CPU tensors: the public path -- validation, labels, windows, the carried state,
the two passes, the rates, the host finish -- runs without a GPU in tests/test_cell_events_host.py.  Not collected by
pytest."""
import numpy as np
import torch

import cell_events_oracle as co


class HostEngine:
    device = torch.device("cpu")

    def __init__(self):
        self.calls = []

    def cell_event_records(self, acc):
        assert acc["finished"] and not acc["second"]
        return {"off": torch.from_numpy(co.finish(acc["st"])["rec"]["off"]), "sum": acc["st"]["anomalies"]}

    def cell_events(self, x, anom=None, t0=0, min_duration=5, max_gap=2, grp=None, G=1, mask=None, records=None, acc=None,
                    finish=True):
        a = x.numpy()
        assert a.dtype in (np.uint8, np.bool_) and a.ndim == 2
        an = None if anom is None else anom.numpy()
        assert an is None or (an.dtype == np.float32 and an.shape == a.shape)
        Tb, C = a.shape
        second = records is not None
        self.calls.append(("cell_events", "records" if second else "summary", t0, Tb))
        if mask is not None:
            assert not second and mask.dtype == torch.uint8 and mask.shape[1] == C and mask.shape[0] >= t0 + Tb
        plan = (G, C, an is not None, min_duration, max_gap)
        if acc is None:
            acc = {"st": None, "plan": plan, "second": second, "finished": False}
        assert acc["plan"] == plan and acc["second"] == second and not acc["finished"]
        acc["st"] = co.walk(a, an, t0, min_duration, max_gap, grp, G, None if mask is None else mask.numpy(), finish, acc["st"])
        out = {"acc": acc}
        if finish:
            acc["finished"] = True
            assert acc["st"]["status"] == [0, 0]
            f = co.finish(acc["st"])
            if second:
                assert np.array_equal(f["rec"]["off"], records["off"].numpy())
                out.update(rec={k: v for k, v in f["rec"].items() if k != "cell"}, records=records)
            else:
                out.update({k: v for k, v in f.items() if k != "rec"})
        return out
