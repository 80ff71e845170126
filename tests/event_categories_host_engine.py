"""A host stand-in for the two engine calls behind ``marex_amd.event_categories`` (``id_spans`` and ``event_categories``), in
NumPy on CPU tensors: the public path -- validation, threshold layouts, windows, slot plan, the host finish -- runs without
a GPU in tests/test_event_categories_host.py.  Not collected by pytest."""
import numpy as np
import torch

from marex_amd.engine import HotPath

from event_categories_oracle import classify
from intensity_host_engine import HostEngine as _SpanEngine


class HostEngine(_SpanEngine):
    def event_categories(self, ids, anom, ev_tmin, ev_tmax, thr, doy, weights=None, t0=0, field=None, acc=None, finish=False):
        i, a, h = ids.numpy(), anom.numpy(), thr.numpy()
        assert i.dtype == np.int32 and a.dtype == np.float32 and i.shape == a.shape
        assert h.dtype == np.float32 and h.ndim == 2 and h.shape[1] == i.shape[1] and thr.is_contiguous()
        doy = np.asarray(doy)
        assert doy.dtype.kind == "i" and doy.size >= t0 + i.shape[0]
        tmin = np.asarray(ev_tmin, np.int64)
        n_ev = tmin.size - 1
        off = HotPath.event_slot_plan(ev_tmin, ev_tmax)
        n = int(off[-1])
        self.calls.append(("event_categories", t0, i.shape[0]))
        if acc is None:
            acc = {"cnt": np.zeros((n, 7), np.int64), "area": None if weights is None else np.zeros((n, 6)), "plan": off}
        assert np.array_equal(acc["plan"], off) and (acc["area"] is None) == (weights is None)
        for r in range(i.shape[0]):
            d = int(doy[t0 + r])
            assert 0 <= d < h.shape[0]
            sel = np.nonzero((i[r] > 0) & (i[r] <= n_ev))[0]
            e = i[r][sel]
            s = off[e] + (t0 + r) - tmin[e]
            assert ((s >= off[e]) & (s < off[e + 1])).all()
            k = classify(a[r][sel], h[d][sel])
            np.add.at(acc["cnt"], (s, k), 1)
            if weights is not None:
                cl = k < 6
                np.add.at(acc["area"], (s[cl], k[cl]), weights.numpy()[sel][cl].astype(np.float64))
            if field is not None:
                assert field.dtype.is_floating_point is False and field.shape[1] == i.shape[1]
                row = np.zeros(i.shape[1], np.uint8)
                row[sel] = k + 1
                field[t0 + r] = torch.from_numpy(row)
        out = {"off": off, "acc": acc}
        if finish:
            out.update(cat_cnt=acc["cnt"], cat_area=acc["area"])
        return out
