"""NumPy oracle of the occurrence statistics (``marex_occurrence_u8`` / ``marex_occurrence_i32``,
``marex_amd.event_occurrence``): plain loops and ``np.add.at`` over the notebook idioms.  Not collected by pytest."""
import numpy as np


def present(x, match=0):
    x = np.asarray(x)
    x = x.astype(np.int64) if x.dtype != bool else x.astype(np.int64)
    return (x == match) if match else (x > 0)


def cell_counts(x, grp=None, G=1, match=0):
    """uint32 ``[G, C]``: per group the steps at which a cell is present; labels outside ``0 .. G - 1`` count nowhere."""
    p = present(x, match)
    T, C = p.shape
    out = np.zeros((G, C), np.uint32)
    for t in range(T):
        g = 0 if grp is None else int(grp[t])
        if 0 <= g < G:
            out[g] += p[t].astype(np.uint32)
    return out


def run_stats(x, match=0, state=None):
    """uint32 ``[3, C]``: per cell the run open after the last row, the runs begun and the longest run -- one cell and one
    step after the other.  ``state``: the result of the rows before."""
    p = present(x, match)
    T, C = p.shape
    out = np.zeros((3, C), np.uint32) if state is None else np.array(state, np.uint32)
    for c in range(C):
        run, n, longest = (int(v) for v in out[:, c])
        for t in range(T):
            if p[t, c]:
                if run == 0:
                    n += 1
                run += 1
                longest = max(longest, run)
            else:
                run = 0
        out[:, c] = (run, n, longest)
    return out


def section_counts(x, sgrp, G2, cls, R, match=0):
    """uint64 ``[G2, R]``: present cells per (step label, cell class); a class or a label outside its range counts nowhere."""
    p = present(x, match)
    out = np.zeros((G2, R), np.uint64)
    cls = np.asarray(cls)
    ok = (cls >= 0) & (cls < R)
    for t in range(p.shape[0]):
        g = int(sgrp[t])
        if 0 <= g < G2:
            np.add.at(out[g], cls[ok & p[t]], np.uint64(1))
    return out


def status(x, grp=None, G=1, sgrp=None, G2=0, cls=None, R=0, match=0):
    """``[negative cells, present cells under a label outside its range]`` as the kernel counts them."""
    x = np.asarray(x)
    p = present(x, match)
    neg = int((x.astype(np.int64) < 0).sum()) if x.dtype != bool else 0
    lost = 0
    for t in range(p.shape[0]):
        if grp is not None and not 0 <= int(grp[t]) < G:
            lost += int(p[t].sum())
        if sgrp is not None and not 0 <= int(sgrp[t]) < G2:
            c = np.asarray(cls)
            lost += int((p[t] & (c >= 0) & (c < R)).sum())
    return [neg, lost]


def lat_bin(lat, edges):
    """Bin r holds ``edges[r] < lat <= edges[r + 1]``; -1 elsewhere and for a non-finite latitude.  One cell after the other."""
    out = np.full(len(lat), -1, np.int32)
    for c, v in enumerate(np.asarray(lat, np.float64)):
        for r in range(len(edges) - 1):
            if edges[r] < v <= edges[r + 1]:
                out[c] = r
    return out


def ratio(num, den):
    num, den = np.broadcast_arrays(np.asarray(num, np.float64), np.asarray(den, np.float64))
    out = np.full(num.shape, np.nan)
    np.divide(num, den, out=out, where=den != 0)
    return out


def occurrence(x, grp=None, G=1, sgrp=None, G2=0, cls=None, R=0, class_cells=None, event_ids=()):
    """The variables of ``marex_amd.event_occurrence`` over a ``[T, C]`` field, flat in space."""
    x = np.asarray(x)
    T = x.shape[0]
    cc = cell_counts(x, grp, G)
    rs = run_stats(x)
    occ = cc.sum(axis=0, dtype=np.uint32)
    out = {"occurrence": occ, "frequency": ratio(occ, T), "n_runs": rs[1], "longest_run": rs[2], "mean_run": ratio(occ, rs[1])}
    if grp is not None:
        steps = np.bincount(np.asarray(grp), minlength=G).astype(np.int64)
        out.update(occurrence_by=cc, steps_by=steps, frequency_by=ratio(cc, steps[:, None]))
    if sgrp is not None:
        sc = section_counts(x, sgrp, G2, cls, R)
        steps = np.bincount(np.asarray(sgrp), minlength=G2).astype(np.int64)
        out.update(presence_cells=sc, class_cells=np.asarray(class_cells, np.int64),
                   presence=ratio(sc, steps[:, None] * np.asarray(class_cells, np.int64)[None, :]))
    if event_ids:
        out["local_duration"] = np.stack([cell_counts(x, match=int(e))[0] for e in event_ids])
    return out
