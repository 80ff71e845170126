"""Seeded synthetic inputs of the mesh merge tests and of tests/measure_mesh_merge.py: ring-with-chords meshes and fields of
drifting runs of cells whose objects fuse and separate.  Not a test module."""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import mesh_objects_oracle as mo  # noqa: E402


def ring_mesh(rng, C, chords=True):
    """Cells on a ring with one random chord each, some neighbours missing, some listed from one end only (``_tri_mesh`` of
    test_gpu_mesh_objects.py) and coordinates along a wavy band: ``nb0`` 0-based [3, C], ``mask``, ``areas``, ``lat``, ``lon``."""
    nb = np.full((3, C), -1, dtype=np.int32)
    nb[0] = (np.arange(C) + 1) % C
    nb[1] = (np.arange(C) - 1) % C
    if chords:
        nb[2] = rng.integers(0, C, C)
        nb[2][rng.random(C) < 0.2] = -1
        nb[1][rng.random(C) < 0.05] = -1
    ang = 2 * np.pi * np.arange(C) / C
    return {"nb0": nb, "mask": np.ones(C, bool), "areas": (10.0 ** rng.uniform(5, 7, C)).astype(np.float32),
            "lat": 40.0 * np.sin(3 * ang) + rng.uniform(-1, 1, C), "lon": np.degrees(ang) - 180.0 + rng.uniform(-0.2, 0.2, C)}


def drifting_runs(seed, C, T=8, n_runs=7):
    """``(mesh, ids int32 [T, C] unique in time)``: ``n_runs`` runs of cells on the ring, each drifting and changing its
    length from step to step, so that neighbours fuse into one object and separate again; positions scale with C / 200.
    The objects are the connected runs (ring edges only: the chords of the mesh do not join objects here)."""
    rng = np.random.default_rng(seed)
    mesh = ring_mesh(rng, C)
    sc = max(C // 200, 1)
    start = 8 + 26 * np.arange(n_runs) + rng.integers(0, 6, n_runs)
    length = rng.integers(10, 22, n_runs)
    x = np.zeros((T, C), bool)
    for t in range(T):
        for s, n in zip(start, length):
            x[t, (np.arange(s * sc, (s + n) * sc)) % C] = True
        start = start + rng.integers(-3, 5, n_runs)
        length = np.clip(length + rng.integers(-9, 10, n_runs), 4, 30)
    ring = np.full((3, C), -1, np.int32)
    ring[0], ring[1] = (np.arange(C) + 1) % C, (np.arange(C) - 1) % C
    ids = mo.unique_ids_in_time(mo.identify_objects(x, mesh["mask"], ring)).astype(np.int32)
    return mesh, ids
