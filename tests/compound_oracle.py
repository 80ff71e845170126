"""NumPy oracle of the compound-event statistics (``marex_compound_u8``, ``marex_amd.compound_events``), vectorised over
the cells: the definitions and nothing else.  With ``A[t]``, ``B[t]`` the presence of a cell at step ``t``:

* the counts are boolean sums of ``A``, ``B`` and ``A & B`` (per time group, per (time group, cell class));
* ``lag_days[l] = #{t : A[t] and B[t + l]}`` comes from shifted slices, so pairs that reach outside the record do not exist;
* a run ``[s, e]`` of A is coincident when any ``B`` lies in the clipped ``[s - K, e + K]``, tested per run;
* the run statistics of ``A & B`` are those of tests/occurrence_oracle.py.

The per-run test needs whole runs, so the state that goes in and out of :func:`compound` is the record seen so far: a
window is appended and the statistics are those of the record up to its end.  Not collected by pytest."""
import numpy as np

import occurrence_oracle as oo


def present(x):
    """Nonzero for a mask (bool, uint8), ``> 0`` for an ID field."""
    return oo.present(x)


def day_counts(A, B, grp=None, G=1):
    """uint32 ``[3, G, C]``: per group the steps with A, with B, with both; labels outside ``0 .. G - 1`` count nowhere."""
    T, C = A.shape
    g = np.zeros(T, np.int64) if grp is None else np.asarray(grp, np.int64)[:T]
    out = np.zeros((3, G, C), np.uint32)
    for k, P in enumerate((A, B, A & B)):
        for q in range(G):
            out[k, q] = P[g == q].sum(axis=0)
    return out


def lag_days(A, B, L):
    """uint32 ``[2 L + 1, C]``: row ``L + l`` counts the steps ``t`` with ``A[t]`` and ``B[t + l]``, both inside the record."""
    T, C = A.shape
    out = np.zeros((2 * L + 1, C), np.uint32)
    for l in range(-L, L + 1):
        if abs(l) < T:
            a, b = (A[:T - l], B[l:]) if l >= 0 else (A[-l:], B[:T + l])
            out[L + l] = (a & b).sum(axis=0)
    return out


def run_coincidence(A, B, K):
    """uint32 ``[2, C]``: the runs of A per cell, and those with any B in ``[max(0, s - K), min(T - 1, e + K)]``."""
    T, C = A.shape
    out = np.zeros((2, C), np.uint32)
    if T == 0:
        return out
    At = A.T  # [C, T]: nonzero() lists the runs cell by cell in time order, starts and ends in step
    prev = np.concatenate([np.zeros((C, 1), bool), At[:, :-1]], axis=1)
    nxt = np.concatenate([At[:, 1:], np.zeros((C, 1), bool)], axis=1)
    c, s = np.nonzero(At & ~prev)
    c2, e = np.nonzero(At & ~nxt)
    assert np.array_equal(c, c2) and (e >= s).all()
    nb = np.concatenate([np.zeros((C, 1), np.int64), np.cumsum(B.T, axis=1, dtype=np.int64)], axis=1)  # B in steps < t
    lo, hi = np.maximum(s - K, 0), np.minimum(e + K, T - 1)
    hit = nb[c, hi + 1] - nb[c, lo] > 0
    out[0] = np.bincount(c, minlength=C)
    out[1] = np.bincount(c[hit], minlength=C)
    return out


def section_counts(A, B, sgrp, G2, cls, R):
    """uint64 ``[3, G2, R]``: present cells of A, of B and of both per (step label, cell class)."""
    lab = np.asarray(sgrp)[:A.shape[0]]
    return np.stack([oo.section_counts(P, lab, G2, cls, R) for P in (A, B, A & B)])


def compound(a, b, L=0, K=0, grp=None, G=1, sgrp=None, G2=0, cls=None, R=0, state=None):
    """The arrays of ``HotPath.compound`` after the rows ``a``, ``b`` ``[Tb, C]`` were appended to ``state`` (None: the
    record starts here), and the new state.  ``grp`` / ``sgrp`` label the global steps."""
    A, B = present(a), present(b)
    if state is not None:
        A, B = np.concatenate([state["A"], A]), np.concatenate([state["B"], B])
    ra, rb = run_coincidence(A, B, K), run_coincidence(B, A, K)
    return {"days": day_counts(A, B, grp, G), "runs": oo.run_stats(A & B), "co": np.concatenate([ra, rb]),
            "lag_days": lag_days(A, B, L) if L else None,
            "sec_cnt": None if sgrp is None else section_counts(A, B, sgrp, G2, cls, R), "state": {"A": A, "B": B}}


def lost(a, b, grp=None, G=1, sgrp=None, G2=0, cls=None, R=0):
    """What the kernel adds to ``status[1]``: the cells of A and those of B under a step label outside its range."""
    A, B = present(a), present(b)
    n = 0
    for t in range(A.shape[0]):
        if grp is not None and not 0 <= int(grp[t]) < G:
            n += int(A[t].sum()) + int(B[t].sum())
        if sgrp is not None and not 0 <= int(sgrp[t]) < G2:
            ok = (np.asarray(cls) >= 0) & (np.asarray(cls) < R)
            n += int((A[t] & ok).sum()) + int((B[t] & ok).sum())
    return n


def variables(a, b, L=0, K=0, grp=None, G=1, sgrp=None, G2=0, cls=None, R=0, class_cells=None):
    """The variables of ``marex_amd.compound_events`` over two ``[T, C]`` fields, flat in space (without the mask)."""
    r = compound(a, b, L, K, grp, G, sgrp, G2, cls, R)
    T = np.asarray(a).shape[0]
    d = r["days"].astype(np.int64)
    na, nb, both = (d[k].sum(axis=0) for k in range(3))
    u32 = lambda v: v.astype(np.uint32)  # noqa: E731
    out = {"days_a": u32(na), "days_b": u32(nb), "days_both": u32(both), "n_runs": r["runs"][1], "longest_run": r["runs"][2],
           "mean_run": oo.ratio(both, r["runs"][1]), "lmf": oo.ratio(both * T, na * nb), "jaccard": oo.ratio(both, na + nb - both),
           "runs_a": r["co"][0], "runs_a_coincident": r["co"][1], "runs_b": r["co"][2], "runs_b_coincident": r["co"][3],
           "coincidence_a": oo.ratio(r["co"][1], r["co"][0]), "coincidence_b": oo.ratio(r["co"][3], r["co"][2])}
    if L:
        out["lag_days"] = r["lag_days"]
    if grp is not None:
        steps = np.bincount(np.asarray(grp), minlength=G).astype(np.int64)
        out.update(days_a_by=r["days"][0], days_b_by=r["days"][1], days_both_by=r["days"][2], steps_by=steps,
                   lmf_by=oo.ratio(d[2] * steps[:, None], d[0] * d[1]))
    if sgrp is not None:
        steps = np.bincount(np.asarray(sgrp), minlength=G2).astype(np.int64)
        cc = np.asarray(class_cells, np.int64)
        out.update(cells_a=r["sec_cnt"][0], cells_b=r["sec_cnt"][1], cells_both=r["sec_cnt"][2],
                   share_both=oo.ratio(r["sec_cnt"][2], steps[:, None] * cc[None, :]), class_cells=cc)
    return out
