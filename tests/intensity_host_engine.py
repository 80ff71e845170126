"""A host stand-in for the two engine calls behind ``marex_amd.event_intensity`` (``id_spans`` and ``event_intensity``), in
NumPy on CPU tensors: the public path -- validation, windows, slot plan, the host finish -- runs without a GPU in
tests/test_event_intensity_host.py.  Not collected by pytest."""
import numpy as np
import torch

from marex_amd.engine import HotPath


class HostEngine:
    device = torch.device("cpu")

    def __init__(self):
        self.calls = []

    def id_spans(self, ids):
        a = ids.numpy()
        assert a.dtype == np.int32 and a.ndim == 2
        if a.min() < 0:
            raise AssertionError("negative ID")
        hi = int(a.max())
        self.calls.append(("id_spans", a.shape[0]))
        if hi <= 0:
            return None
        tmin, tmax = np.full(hi + 1, 2**31 - 1, np.int32), np.full(hi + 1, -1, np.int32)
        for t in range(a.shape[0]):
            u = np.unique(a[t])
            tmin[u] = np.minimum(tmin[u], t)
            tmax[u] = np.maximum(tmax[u], t)
        return tmin, tmax

    def event_intensity(self, ids, anom, ev_tmin, ev_tmax, weights=None, t0=0, acc=None, finish=True):
        i, a = ids.numpy(), anom.numpy()
        assert i.dtype == np.int32 and a.dtype == np.float32 and i.shape == a.shape
        tmin = np.asarray(ev_tmin, np.int64)
        n_ev = tmin.size - 1
        off = HotPath.event_slot_plan(ev_tmin, ev_tmax)
        n = int(off[-1])
        self.calls.append(("event_intensity", t0, i.shape[0]))
        if acc is None:
            acc = {"cnt": np.zeros((n, 2), np.int64), "sums": np.zeros((n, 2)), "key": np.zeros(n, np.uint32), "plan": off}
        assert np.array_equal(acc["plan"], off)
        w = np.ones(i.shape[1]) if weights is None else weights.numpy().astype(np.float64)
        b = a.view(np.uint32)
        key = np.where(b & np.uint32(0x80000000), ~b, b | np.uint32(0x80000000))
        for r in range(i.shape[0]):
            sel = np.nonzero((i[r] > 0) & (i[r] <= n_ev))[0]
            e = i[r][sel]
            s = off[e] + (t0 + r) - tmin[e]
            assert ((s >= off[e]) & (s < off[e + 1])).all()
            ok = np.isfinite(a[r][sel])
            np.add.at(acc["cnt"][:, 0], s[ok], 1)
            np.add.at(acc["cnt"][:, 1], s[~ok], 1)
            np.add.at(acc["sums"][:, 0], s[ok], w[sel][ok])
            np.add.at(acc["sums"][:, 1], s[ok], w[sel][ok] * a[r][sel][ok].astype(np.float64))
            np.maximum.at(acc["key"], s[ok], key[r][sel][ok])
        out = {"off": off, "acc": acc}
        if finish:
            k = acc["key"]
            bits = np.where(k & np.uint32(0x80000000), k & np.uint32(0x7FFFFFFF), ~k).astype(np.uint32)
            out.update(cnt=acc["cnt"], sums=acc["sums"], vmax=bits.view(np.float32))
        return out
