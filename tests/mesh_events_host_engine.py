"""The NumPy stand-in for the engine (tests/mesh_merge_host_engine.py) extended by the calls ``tracker.track_objects`` and
``tracker.cluster_rename_objects_and_props`` make on a mesh: per-timestep labelling, IDs unique in time and the event
rename pass, answered by the oracles on CPU tensors.  The rename pass is answered by the very function the events oracle
uses, so CPU tests over this engine check the host side of the stage -- event table, presence, ledger, finish, dims, the
chaining -- and not the arithmetic of the device pass; tests/test_gpu_mesh_events.py checks the kernel against NumPy.  Test
support only: the package itself has no CPU path."""
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import mesh_events_oracle as me  # noqa: E402
import mesh_objects_oracle as mo  # noqa: E402
from mesh_merge_host_engine import HostEngine  # noqa: E402


class EventsHostEngine(HostEngine):
    def __init__(self):
        super().__init__()
        self.calls = []

    def label_objects_mesh(self, x, mask, nbr, max_block_cells=None):
        self.calls.append("label_objects_mesh")
        ids = mo.identify_objects(x.numpy().astype(bool), mask.numpy().astype(bool), nbr.numpy())
        return {"ids": torch.from_numpy(np.ascontiguousarray(ids, dtype=np.int32)),
                "n_t": torch.from_numpy(ids.max(axis=1).astype(np.int32))}

    def unique_ids_in_time(self, ids):
        self.calls.append("unique_ids_in_time")
        return torch.from_numpy(np.ascontiguousarray(mo.unique_ids_in_time(ids.numpy()), dtype=np.int32))

    def mesh_event_rename(self, ids, lut, n_ev, q, e):
        self.calls.append("mesh_event_rename")
        a = ids.numpy()  # shares memory: relabelled in place
        new, sums, gid = me.rename_and_sums(a, lut, int(n_ev), q.numpy())
        a[...] = new
        return {"mom": sums, "gid": gid}


def use_events_host_engine(monkeypatch, trk):
    """Make ``trk`` run its device stages on an :class:`EventsHostEngine`; returns the engine."""
    eng = EventsHostEngine()
    monkeypatch.setattr(trk, "_engine", lambda: eng)
    monkeypatch.setattr(type(trk), "_check_fits", staticmethod(lambda eng, need, what: None))
    return eng
