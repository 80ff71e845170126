"""Host restatement of the labelling in time blocks (``HotPath.label_objects_3d(..., max_block_cells=...)``, DESIGN.md
section 4) for the tests, beside the whole-field labelling it has to equal.  Not a test module (no ``test_`` prefix).

* :func:`label_whole`: one ``scipy.ndimage.label`` over the field (3 x 3 x 3 structure; its t-1 / t+1 planes empty
  when ``connect_t`` is off), the x seam emulated as tests/track_oracle.py does, IDs 1..N by first cell in C order.
* :func:`label_blocked`: the algorithm itself -- label blocks of timesteps on their own, offset the block labels in time
  order, union the provisional IDs over the 3 x 3 neighbourhoods across every seam, rank the roots.
* :func:`seam_cases`: the hand-built fields both the host and the device tests walk.
"""
import numpy as np


def _structure(connect_t: bool) -> np.ndarray:
    s = np.ones((3, 3, 3), dtype=bool)
    if not connect_t:
        s[0] = s[2] = False
    return s


def label_whole(data_bin, wrap_x: bool = True, connect_t: bool = True):
    """``(ids int32 [T, ny, nx], N)`` of the whole field in one labelling."""
    from scipy import ndimage as ndi
    from scipy.sparse import coo_matrix
    from scipy.sparse.csgraph import connected_components

    d = np.asarray(data_bin).astype(bool)
    T, ny, nx = d.shape
    lab, n = ndi.label(d, structure=_structure(connect_t))
    if n == 0:
        return np.zeros(d.shape, dtype=np.int32), 0
    if wrap_x and nx > 1:
        a, b = [], []
        left, right = lab[:, :, 0], lab[:, :, nx - 1]
        for dt in ((-1, 0, 1) if connect_t else (0,)):
            for dy in (-1, 0, 1):
                t0, t1 = max(0, -dt), min(T, T - dt)
                y0, y1 = max(0, -dy), min(ny, ny - dy)
                if t1 <= t0 or y1 <= y0:
                    continue
                L = left[t0:t1, y0:y1]
                R = right[t0 + dt:t1 + dt, y0 + dy:y1 + dy]
                ok = (L > 0) & (R > 0)
                a.append(L[ok])
                b.append(R[ok])
        a, b = np.concatenate(a), np.concatenate(b)
        g = coo_matrix((np.ones(a.size, dtype=np.int8), (a, b)), shape=(n + 1, n + 1))
        _, comp = connected_components(g, directed=False)
        lab = np.where(lab > 0, comp[lab] + 1, 0)
    flat = lab.reshape(-1)
    nz = flat > 0
    vals = flat[nz]
    uniq, first = np.unique(vals, return_index=True)
    order = np.argsort(first, kind="stable")
    new = np.empty(uniq.size, dtype=np.int64)
    new[order] = np.arange(1, uniq.size + 1)
    out = np.zeros(flat.shape, dtype=np.int32)
    out[nz] = new[np.searchsorted(uniq, vals)]
    return out.reshape(d.shape), int(uniq.size)


def _find(parent, i):
    while parent[i] != i:
        parent[i] = parent[parent[i]]
        i = parent[i]
    return i


def label_blocked(data_bin, block_steps: int, wrap_x: bool = True, connect_t: bool = True):
    """``(ids int32, N, areas int64 [N])`` by the blocked algorithm with blocks of ``block_steps`` timesteps."""
    d = np.asarray(data_bin).astype(bool)
    T, ny, nx = d.shape
    blocks = [(t0, min(T, t0 + block_steps)) for t0 in range(0, T, block_steps)]
    prov = np.zeros(d.shape, dtype=np.int64)
    offs, counts = [], []
    n_prov = 0
    for t0, t1 in blocks:  # local IDs 1..n_k by first cell inside the block, provisional = off_k + local
        lab, nk = label_whole(d[t0:t1], wrap_x, connect_t)
        prov[t0:t1] = np.where(lab > 0, lab.astype(np.int64) + n_prov, 0)
        offs.append(n_prov)
        counts.append(nk)
        n_prov += nk
    parent = np.arange(n_prov + 1)
    if connect_t:
        for (_, seam) in blocks[:-1]:
            prev, nxt = prov[seam - 1], prov[seam]
            for y, x in zip(*np.nonzero(nxt)):
                for dy in (-1, 0, 1):
                    for dx in (-1, 0, 1):
                        yy, xx = y + dy, x + dx
                        if not 0 <= yy < ny:
                            continue
                        if not 0 <= xx < nx:
                            if not (wrap_x and nx > 1):
                                continue
                            xx %= nx
                        if prev[yy, xx]:
                            a, b = _find(parent, prev[yy, xx]), _find(parent, nxt[y, x])
                            if a != b:
                                parent[max(a, b)] = min(a, b)  # hook the larger root under the smaller
    root = np.array([_find(parent, g) for g in range(n_prov + 1)])
    is_root = root == np.arange(n_prov + 1)
    final = np.cumsum(is_root)[root] - 1  # entry 0 is a root: 1 + roots below root(g) without it, final[0] = 0
    n = int(is_root.sum()) - 1
    ids = final[prov].astype(np.int32)
    areas = np.bincount(ids.reshape(-1), minlength=n + 1)[1:].astype(np.int64)
    return ids, n, areas


def blobby(rng, shape, dens):
    """A random field of smooth blobs covering about ``dens`` of the cells."""
    from scipy import ndimage as ndi

    f = ndi.gaussian_filter(rng.normal(0, 1, shape), sigma=(0.8, 1.2, 1.5), mode="wrap")
    return f > np.quantile(f, 1.0 - dens)


def seam_cases():
    """``[(name, field bool [9, 8, 10], wrap_x, expected N or None)]``: with blocks of 1, 2, 3, 7 or 8 steps every
    case has its contact on at least one seam."""
    T, ny, nx = 9, 8, 10
    out = []

    def z():
        return np.zeros((T, ny, nx), dtype=bool)

    for t in range(T - 1):  # one diagonal contact (dt, dy, dx) = (1, 1, 1), on every possible seam in turn
        x = z()
        x[t, 3, 4] = x[t + 1, 4, 5] = True
        out.append((f"diagonal t={t}", x, True, 1))
        x = z()
        x[t, 3, nx - 1] = x[t + 1, 4, 0] = True  # the same diagonal through the x seam
        out.append((f"diagonal through the x seam t={t}, periodic", x, True, 1))
        out.append((f"diagonal through the x seam t={t}, regional", x, False, 2))
        x = z()
        x[t, 4, 0] = x[t + 1, 3, nx - 1] = True  # and the other way round
        out.append((f"diagonal through the x seam westwards t={t}, periodic", x, True, 1))
        out.append((f"diagonal through the x seam westwards t={t}, regional", x, False, 2))
    for t in range(1, T - 1):
        x = z()  # two events up to step t joined only by a bar at step t + 1; later IDs all shift down by one
        x[:t + 1, 2, 2] = x[:t + 1, 2, 6] = True
        x[t + 1, 2, 2:7] = True
        x[0, 6, 3] = x[t, 6, 8] = x[t + 1, 6, 5] = x[T - 1, 7, 0] = True
        out.append((f"joined only through the later block, bar at t={t + 1}", x, False, None))
        x = z()  # the mirror: a bar at step t, two arms from t + 1 on that never touch again
        x[t, 2, 2:7] = True
        x[t + 1:, 2, 2] = x[t + 1:, 2, 6] = True
        x[0, 6, 3] = x[t, 6, 8] = x[t + 1, 6, 5] = x[T - 1, 7, 0] = True
        out.append((f"joined only through the earlier block, bar at t={t}", x, False, None))
    x = z()
    x[:, 5, 5] = True
    x[2, 1, 1] = x[6, 1, 8] = True
    out.append(("one event through every block", x, True, 3))
    x = z()
    x[0, 1, 1] = x[1, 1, 2] = x[7, 3, 3] = x[8, 3, 4] = x[8, 6, 6] = True
    out.append(("empty blocks in the middle", x, True, 3))
    x = z()
    x[0, 1, 1] = x[8, 1, 1] = True
    out.append(("seams between empty slices", x, True, 2))
    out.append(("all ones", np.ones((T, ny, nx), dtype=bool), True, 1))
    out.append(("all ones, regional", np.ones((T, ny, nx), dtype=bool), False, 1))
    out.append(("empty field", z(), True, 0))
    return out
