"""A NumPy stand-in for the engine calls of ``tracker.split_and_merge_objects_parallel``, so that the stage's host side --
chunk snapshots, queues, temporary IDs, limits -- runs in the CPU tests exactly as it runs over the device engine.  Every
call answers with the oracle's functions on CPU tensors.  Test support only: the package itself has no CPU path."""
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import mesh_merge_oracle as mm  # noqa: E402
import mesh_objects_oracle as mo  # noqa: E402


class HostEngine:
    device = torch.device("cpu")

    def __init__(self):
        self.nn_calls = []

    def sync(self):
        pass

    def mesh_overlap_pairs(self, ids, q, e):
        return mo.find_overlapping_objects(ids.numpy(), q.numpy(), e)

    def mesh_object_moments(self, ids, q, e):
        t, i, cells, area, cen = mo.object_properties(ids.numpy(), q.numpy(), e)
        return {"t": t, "id": i, "cells": cells, "area": area, "centroid": cen}

    def id_spans(self, ids):
        a = ids.numpy()
        hi = int(a.max())
        if hi <= 0:
            return None
        tmin = np.full(hi + 1, np.iinfo(np.int32).max, np.int32)
        tmax = np.full(hi + 1, -1, np.int32)
        for t in range(a.shape[0]):
            u = np.unique(a[t][a[t] > 0])
            tmin[u] = np.minimum(tmin[u], t)
            tmax[u] = np.maximum(tmax[u], t)
        return tmin, tmax

    def relabel(self, ids, vals, keys=None):
        a = ids.numpy()  # shares memory
        keys, vals = np.asarray(keys, np.int64), np.asarray(vals, np.int32)
        pos = np.clip(np.searchsorted(keys, a), 0, keys.size - 1)
        hit = keys[pos] == a
        a[hit] = vals[pos][hit]

    def mesh_partition_centroid(self, cur, child_keys, off, parent_vectors, labels, u):
        a, un, lab = cur.numpy(), u.numpy(), np.asarray(labels, np.int32)
        pv = np.asarray(parent_vectors, np.float64)
        masks = [a == c for c in child_keys]
        for k, m in enumerate(masks):
            j0, j1 = int(off[k]), int(off[k + 1])
            a[m] = lab[j0:j1][mm.nearest_centroid(un[:, m], pv[:, j0:j1])]

    def mesh_partition_nn(self, cur, prev, nbr, child, parents, parent_vectors, labels, max_hops, u, hops_per_read=None):
        a, p = cur.numpy(), prev.numpy()
        owner = np.full(a.size, 255, np.uint8)
        for j, par in enumerate(parents):
            owner[p == par] = j
        m = a == child
        owner, info = mm.partition_nn(m, owner, nbr.numpy(), int(max_hops), u.numpy(), np.asarray(parent_vectors, np.float64))
        a[m] = np.asarray(labels, np.int32)[owner[m]]
        self.nn_calls.append(info)
        reason = 2 if info["early_stop"] else 3 if info["capped"] else 1
        return {"hops": info["hops"], "leftover": info["leftover"], "reason": reason, "launches": 0, "reads": 0}


def use_host_engine(monkeypatch, trk):
    """Make ``trk`` run its device stages on a :class:`HostEngine`; returns the engine."""
    eng = HostEngine()
    monkeypatch.setattr(trk, "_engine", lambda: eng)
    monkeypatch.setattr(type(trk), "_check_fits", staticmethod(lambda eng, need, what: None))
    return eng
