"""Meshes, geometries and event fields shared by tests/test_mesh_event_shapes_host.py and tests/test_gpu_mesh_event_shapes.py.
Neighbour tables here are 0-based with -1 for "none" (the oracle's and the kernel's convention); the public function takes
``nbr0 + 1``.  Not collected by pytest."""
import numpy as np


def ring(C):
    """Cell c between c + 1 and c - 1 (periodic), third slot empty: the mesh of ``_small()`` in test_mesh_tracker_host.py."""
    c = np.arange(C)
    return np.stack([(c + 1) % C, (c - 1) % C, np.full(C, -1)]).astype(np.int32)


def triangular(ny, nx):
    """Cells in rows of nx: left and right in the row, and up (even columns) or down (odd columns) -- the row-triangular mesh
    of tests/measure_mesh_objects.py."""
    c = np.arange(ny * nx, dtype=np.int64)
    y, x = c // nx, c % nx
    left = np.where(x > 0, c - 1, -1)
    right = np.where(x < nx - 1, c + 1, -1)
    vert = np.where(x % 2 == 0, np.where(y > 0, c - nx, -1), np.where(y < ny - 1, c + nx, -1))
    return np.stack([left, right, vert]).astype(np.int32)


def permuted(nbr0, seed):
    """The same mesh with its cells renumbered at random: ``(nbr0', new)`` with ``new[c]`` the new number of cell c."""
    C = nbr0.shape[1]
    new = np.random.default_rng(seed).permutation(C)
    out = np.full_like(nbr0, -1)
    out[:, new] = np.where(nbr0 >= 0, new[np.maximum(nbr0, 0)], -1)
    return out, new


def ragged(nbr0, seed):
    """Some slots emptied and some neighbours listed twice."""
    rng = np.random.default_rng(seed)
    out = nbr0.copy()
    C = out.shape[1]
    drop = rng.random(C) < 0.15
    out[2, drop] = -1
    twice = (rng.random(C) < 0.15) & (out[0] >= 0)
    out[1, twice] = out[0, twice]
    return out


def geometry(C, seed, grid=None):
    """``lat``, ``lon`` in degrees: random points of the sphere (longitudes on both sides of the date line, a few cells at
    the poles), or with ``grid = (ny, nx)`` a regular patch, so that blobs of the mesh are blobs on the sphere."""
    rng = np.random.default_rng(seed)
    if grid is not None:
        ny, nx = grid
        la = np.repeat(np.linspace(-35.0, 40.0, ny), nx) + rng.uniform(-0.2, 0.2, C)
        lo = np.tile(np.linspace(150.0, 215.0, nx), ny) + rng.uniform(-0.2, 0.2, C)  # across the date line
        return la, lo
    la = np.degrees(np.arcsin(rng.uniform(-1, 1, C)))
    lo = rng.uniform(-180, 360, C)
    la[rng.random(C) < 0.02] = 90.0
    la[rng.random(C) < 0.02] = -90.0
    return la, lo


def tables(C, seed):
    rng = np.random.default_rng(seed)
    return dict(mask=rng.random(C) > 0.25, cell_areas=10.0 ** rng.uniform(-3, 3, C), edge_lengths=10.0 ** rng.uniform(-3, 3, (3, C)))


def make_field(T, nbr0, seed, n_ev=8, big=30):
    """Sparse event numbers (1, 4, 7, ...), blobs grown over the neighbour table that drift, overwrite and so touch each
    other, steps on which an event is absent inside its span, a background value above every event next to an event, and the
    largest number in the last cell of the last slice."""
    rng = np.random.default_rng(seed)
    C = nbr0.shape[1]
    ids = np.zeros((T, C), np.int32)
    for k in range(n_ev):
        e = 1 + 3 * k
        t0, t1 = sorted(int(v) for v in rng.integers(0, T, 2))
        c = int(rng.integers(0, C))
        for t in range(t0, t1 + 1):
            if t0 < t < t1 and rng.random() < 0.2:
                continue
            blob, front = {c}, [c]
            size = int(rng.integers(1, big + 1))
            while front and len(blob) < size:
                for j in nbr0[:, front.pop(0)]:
                    if 0 <= j < C and j not in blob and rng.random() < 0.85:
                        blob.add(int(j))
                        front.append(int(j))
            ids[t, sorted(blob)] = e
            step = nbr0[int(rng.integers(0, 3)), c]
            c = int(step) if 0 <= step < C else c
    ids[T - 1, C - 1] = 3 * n_ev + 2
    return ids
