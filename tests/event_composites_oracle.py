"""NumPy oracle of the lagged composites (``marex_event_composites_u8``, ``marex_amd.event_composites``): the anchors of
every cell, and per (group, lag, cell) the count, the sum and the sum of squares of the finite values around them, added
strictly in ascending anchor step -- one step after the other, vectorised over the cells that have an anchor at that step
(each cell at most once per step, so the order of the additions of a cell is the order of its anchors).  ``accumulate``
works on a window of rows with its halo, as the library does; ``composites`` is the one-window call.  ``variables`` is what
the public call returns, flat in space.  Not collected by pytest."""
import numpy as np

ANCHORS = ("onset", "end")


def presence(x):
    x = np.asarray(x)
    return x.astype(bool) if x.dtype.kind in "bu" else x > 0


def anchor_steps(x, anchor):
    """bool ``[T, C]``: the anchors.  A run that touches step 0 has no onset, one that touches step ``T - 1`` no end."""
    p = presence(x)
    out = np.zeros(p.shape, bool)
    if anchor == "onset":
        out[1:] = p[1:] & ~p[:-1]
    else:
        assert anchor == "end"
        out[:-1] = p[:-1] & ~p[1:]
    return out


def zeros(G, C, L):
    W = 2 * L + 1
    return {"anchors": np.zeros((G, C), np.uint32), "count": np.zeros((G, W, C), np.uint32), "sum": np.zeros((G, W, C), np.float64),
            "sumsq": np.zeros((G, W, C), np.float64), "lost": 0}


def accumulate(acc, x, v, r0, a, b, T, L, anchor="onset", grp=None, G=1):
    """The anchors at the steps ``a .. b - 1`` added to ``acc`` (of :func:`zeros`) in place.  ``x`` and ``v`` are the rows
    ``r0 .. r0 + Tr - 1`` of the record of ``T`` steps; every row that is needed must be among them."""
    p = presence(x)
    v = np.asarray(v).astype(np.float32)  # the device reads float32
    Tr = p.shape[0]
    assert v.shape == p.shape and 0 <= r0 and r0 + Tr <= T and 0 <= a <= b <= T and anchor in ANCHORS

    def row(t):
        assert r0 <= t < r0 + Tr, f"step {t} is not among the rows {r0} .. {r0 + Tr - 1}"
        return t - r0

    for t in range(a, b):
        if anchor == "onset":
            if t == 0:
                continue
            here = p[row(t)] & ~p[row(t - 1)]
        else:
            if t == T - 1:
                continue
            here = p[row(t)] & ~p[row(t + 1)]
        cells = np.nonzero(here)[0]
        if not cells.size:
            continue
        g = 0 if grp is None else int(np.asarray(grp)[t])
        if not 0 <= g < G:  # addresses nothing, and is counted
            acc["lost"] += int(cells.size)
            continue
        acc["anchors"][g, cells] += 1
        for j in range(2 * L + 1):
            tt = t + j - L
            if 0 <= tt < T:
                d = v[row(tt), cells].astype(np.float64)
                ok = np.isfinite(d)
                cc, d = cells[ok], d[ok]
                acc["count"][g, j, cc] += 1
                acc["sum"][g, j, cc] += d
                acc["sumsq"][g, j, cc] += d * d  # the product of two float32 values is exact in float64
    return acc


def composites(x, v, L, anchor="onset", grp=None, G=1):
    x = np.asarray(x)
    T, C = x.shape
    return accumulate(zeros(G, C, L), x, v, 0, 0, T, T, L, anchor, grp, G)


def derived(count, total, sumsq):
    """``(mean, std, t)``: the float64 expressions of the public call's docstring."""
    n = count.astype(np.float64)
    with np.errstate(divide="ignore", invalid="ignore"):
        mean = np.where(count > 0, total / n, np.nan)
        std = np.where(count >= 2, np.sqrt(np.maximum(0.0, (sumsq - total * total / n) / (n - 1.0))), np.nan)
        t = np.where((count >= 2) & (std != 0), mean / (std / np.sqrt(n)), np.nan)
    return mean, std, t


def variables(x, v, L, anchor="onset", grp=None, G=1):
    """The data variables of ``marex_amd.event_composites`` as ``{name: array}``, flat in space."""
    r = composites(x, v, L, anchor, grp, G)
    assert r["lost"] == 0
    if grp is None:
        mean, std, t = derived(r["count"][0], r["sum"][0], r["sumsq"][0])
        return {"anchors": r["anchors"][0], "composite_count": r["count"][0], "composite_sum": r["sum"][0],
                "composite_sumsq": r["sumsq"][0], "composite_mean": mean, "composite_std": std, "composite_t": t}
    mean, std, t = derived(r["count"], r["sum"], r["sumsq"])
    return {"anchors": r["anchors"].sum(axis=0, dtype=np.uint32), "anchors_by": r["anchors"], "composite_count_by": r["count"],
            "composite_sum_by": r["sum"], "composite_sumsq_by": r["sumsq"], "composite_mean_by": mean, "composite_std_by": std,
            "composite_t_by": t, "steps_by": np.bincount(np.asarray(grp), minlength=G).astype(np.int64)}
