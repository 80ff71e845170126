"""A host stand-in for the two engine calls behind ``marex_amd.mesh_event_shapes`` (``id_spans`` and ``mesh_event_shapes``),
in NumPy on CPU tensors: the public path -- validation, tables, windows, slot plan, the host finish -- runs without a GPU in
tests/test_mesh_event_shapes_host.py.  The sums follow the layout of ``marex_mesh_event_shapes_i64`` (include/marex_hip.h).
Not collected by pytest."""
import numpy as np
import torch

from marex_amd.engine import HotPath

from intensity_host_engine import HostEngine as _SpansEngine


class HostEngine(_SpansEngine):
    def _dev(self, a, dtype=None):
        return torch.from_numpy(np.ascontiguousarray(a if dtype is None else a.astype(dtype)))

    def mesh_event_shapes(self, ids, nbr, q, ev_tmin, ev_tmax, mask=None, len_q=None, lat_k=None, lon_k=None, t0=0, acc=None,
                          finish=True):
        i, nb, qh = ids.numpy(), nbr.numpy().astype(np.int64), q.numpy()
        C = i.shape[1]
        assert i.dtype == np.int32 and nb.shape == (3, C) and qh.shape == (10, C) and qh.dtype == np.int64
        tmin = np.asarray(ev_tmin, np.int64)
        n_ev = tmin.size - 1
        off = HotPath.event_slot_plan(ev_tmin, ev_tmax)
        n = int(off[-1])
        self.calls.append(("mesh_event_shapes", t0, i.shape[0]))
        if acc is None:
            box = np.empty((n, 6), np.int32)
            box[:, 0::2], box[:, 1::2] = 2**31 - 1, -2**31
            acc = {"mom": np.zeros((n, 16), np.int64), "box": box, "plan": off}
        assert np.array_equal(acc["plan"], off)
        mom, box = acc["mom"], acc["box"]
        land = None if mask is None else mask.numpy() == 0
        lq = None if len_q is None else len_q.numpy()
        there = (nb >= 0) & (nb < C)
        j = np.where(there, nb, 0)
        for r in range(i.shape[0]):
            g = i[r].astype(np.int64)
            ev = (g > 0) & (g <= n_ev)
            e = np.where(ev, g, 0)
            s = off[e] + (t0 + r) - tmin[e]
            assert ((s >= off[e]) & (s < off[e + 1]))[ev].all()
            sl = s[ev]

            def add(col, v):
                np.add.at(mom[:, col], sl, np.broadcast_to(v, (C,))[ev].astype(np.int64))

            add(0, 1)
            for k in range(10):
                add(1 + k, qh[k])
            other = there & (g[j] != g[None, :])
            exposed = ~there | other
            add(11, exposed.sum(0)), add(12, (~there).sum(0)), add(15, (other & (g[j] > 0)).sum(0))
            if land is not None:
                add(13, (other & land[j]).sum(0))
            if lq is not None:
                add(14, np.where(exposed, lq, 0).sum(0))
            if lat_k is not None:
                la, lo = lat_k.numpy()[ev], lon_k.numpy()[ev]
                np.minimum.at(box[:, 0], sl, la)
                np.maximum.at(box[:, 1], sl, la)
                w = lo < 0
                np.minimum.at(box[:, 2], sl[w], lo[w])
                np.maximum.at(box[:, 3], sl[w], lo[w])
                np.minimum.at(box[:, 4], sl[~w], lo[~w])
                np.maximum.at(box[:, 5], sl[~w], lo[~w])
        out = {"off": off, "acc": acc}
        if finish:
            out.update(mom=mom, box=box)
        return out
