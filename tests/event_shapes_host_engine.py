"""A host stand-in for the two engine calls behind ``marex_amd.event_shapes`` (``id_spans`` and ``event_shapes``), in NumPy on
CPU tensors: the public path -- validation, windows, slot plan, the host finish -- runs without a GPU in
tests/test_event_shapes_host.py.  The sums follow the layout of ``marex_event_shapes_i32`` (include/marex_hip.h).  Not
collected by pytest."""
import numpy as np
import torch

from marex_amd.engine import HotPath

from intensity_host_engine import HostEngine as _SpansEngine


class HostEngine(_SpansEngine):
    def _dev(self, a, dtype=None):
        return torch.from_numpy(np.ascontiguousarray(a if dtype is None else a.astype(dtype)))

    def event_shapes(self, ids, ny, nx, ev_tmin, ev_tmax, regional=False, mask=None, area_q=None, ns_q=None, ew_q=None, t0=0,
                     acc=None, finish=True):
        i = ids.numpy()
        assert i.dtype == np.int32 and i.shape[1] == ny * nx
        tmin = np.asarray(ev_tmin, np.int64)
        n_ev = tmin.size - 1
        off = HotPath.event_slot_plan(ev_tmin, ev_tmax)
        n = int(off[-1])
        self.calls.append(("event_shapes", t0, i.shape[0]))
        if acc is None:
            box = np.empty((n, 6), np.int32)
            box[:, 0::2], box[:, 1::2] = 2**31 - 1, -1
            acc = {"mom": np.zeros((n, 16), np.int64), "box": box, "plan": off}
        assert np.array_equal(acc["plan"], off)
        mom, box = acc["mom"], acc["box"]
        m = None if mask is None else mask.numpy().reshape(ny, nx)
        aq = None if area_q is None else area_q.numpy().reshape(ny, nx)
        nsq = None if ns_q is None else ns_q.numpy()
        ewq = None if ew_q is None else ew_q.numpy()
        yy, xx = np.meshgrid(np.arange(ny, dtype=np.int64), np.arange(nx, dtype=np.int64), indexing="ij")
        for r in range(i.shape[0]):
            g = i[r].reshape(ny, nx).astype(np.int64)
            ev = (g > 0) & (g <= n_ev)
            s = np.where(ev, off[np.where(ev, g, 0)] + (t0 + r) - tmin[np.where(ev, g, 0)], 0)
            assert ((s >= off[np.where(ev, g, 0)]) & (s < off[np.where(ev, g, 0) + 1]))[ev].all()
            pad = np.full((ny + 2, nx + 2), -1, np.int64)  # -1: outside the domain
            land = np.zeros((ny + 2, nx + 2), bool)
            pad[1:-1, 1:-1] = g
            if m is not None:
                land[1:-1, 1:-1] = m == 0
            if not regional:
                pad[1:-1, 0], pad[1:-1, -1] = g[:, -1], g[:, 0]
                land[1:-1, 0], land[1:-1, -1] = land[1:-1, -2].copy(), land[1:-1, 1].copy()
            sides = {}
            for name, (a, b) in {"n": (slice(0, -2), slice(1, -1)), "s": (slice(2, None), slice(1, -1)),
                                 "w": (slice(1, -1), slice(0, -2)), "e": (slice(1, -1), slice(2, None))}.items():
                nb = pad[a, b]
                sides[name] = (ev & (nb != g), nb == -1, land[a, b])
            right = xx > nx // 2
            sel = ev.reshape(-1)
            sl = s.reshape(-1)[sel]

            def add(col, v):
                np.add.at(mom[:, col], sl, np.broadcast_to(v, (ny, nx)).reshape(-1)[sel].astype(np.int64))

            add(0, 1), add(1, yy), add(2, xx), add(3, right), add(5, yy * yy), add(6, xx * xx), add(7, xx * yy)
            add(8, xx * right), add(9, yy * right)
            np.bitwise_or.at(mom[:, 4], sl, ((xx < 100) * 1 + (xx >= nx - 100) * 2).reshape(-1)[sel])
            add(10, sides["n"][0] * 1 + sides["s"][0] * 1)
            add(11, sides["w"][0] * 1 + sides["e"][0] * 1)
            add(12, sum((x & o) * 1 for x, o, _ in sides.values()))
            add(13, sum((x & ~o & c) * 1 for x, o, c in sides.values()))
            if nsq is not None:
                add(14, sides["n"][0] * nsq[:-1, None] + sides["s"][0] * nsq[1:, None]
                    + (sides["w"][0] * 1 + sides["e"][0] * 1) * ewq[:, None])
            if aq is not None:
                add(15, aq)
            yv, xv = yy.reshape(-1)[sel].astype(np.int32), xx.reshape(-1)[sel].astype(np.int32)
            rv = right.reshape(-1)[sel]
            np.minimum.at(box[:, 0], sl, yv)
            np.maximum.at(box[:, 1], sl, yv)
            np.minimum.at(box[:, 2], sl[~rv], xv[~rv])
            np.maximum.at(box[:, 3], sl[~rv], xv[~rv])
            np.minimum.at(box[:, 4], sl[rv], xv[rv])
            np.maximum.at(box[:, 5], sl[rv], xv[rv])
        out = {"off": off, "acc": acc}
        if finish:
            out.update(mom=mom, box=box)
        return out
