"""NumPy oracle of cluster_rename_objects_and_props on a mesh (marEx/track.py:2809-3331 with ``is_unstructured=True``) under
the fixed-point contract of tests/mesh_objects_oracle.py, restated from the reference's text: the events are the connected
components of the overlap pairs over the IDs of the field and of the pair list, numbered by their smallest ID; per
(timestep, event) the largest original ID (what the reference's loop over the sorted ``unique_pairs`` leaves behind,
track.py:2964-2969), the area and the centroid on the sphere from int64 sums of ``q``; presence, time_start / time_end and
the merge ledger with the reference's broadcast.  Imports nothing from marex_amd.  Not a test module."""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import mesh_objects_oracle as mo  # noqa: E402


def event_table(field, pairs):
    """``(lut int32 [max ID + 1], N)``: ID -> event 1..N (0: no such ID), track.py:2839-2897.  An ID of the pair list above
    the largest ID of the field has no entry (the reference's table ends at the field's maximum); it still takes part in
    the components."""
    field = np.asarray(field)
    pairs = np.asarray(pairs, dtype=np.int64).reshape(-1, 2)
    ids = sorted({int(v) for v in np.unique(field) if v > 0} | {int(v) for v in pairs.reshape(-1) if v > 0})
    root = {i: i for i in ids}

    def find(a):
        while root[a] != a:
            a = root[a]
        return a

    for a, b in pairs.tolist():
        if a in root and b in root:
            ra, rb = find(a), find(b)
            root[max(ra, rb)] = min(ra, rb)
    number = {}
    for i in ids:  # ascending: scipy's connected_components numbers a component when it meets its first node
        number.setdefault(find(i), len(number) + 1)
    lut = np.zeros(max(int(field.max()), 0) + 1, np.int32)
    for i in ids:
        if i < lut.size:
            lut[i] = number[find(i)]
    return lut, len(number)


def rename_and_sums(field, lut, n_ev, q):
    """``(event field int32, sums int64 [T, n_ev, 5], global_ID int32 [T, n_ev])``: the relabelled field
    (map_IDs_to_indices, track.py:2908-2913), per (timestep, event) the cells and the sums of ``q[0..3]`` over them, and the
    largest original ID; one loop over (timestep, event) as calculate_area_centroid_for_slice walks them."""
    field = np.asarray(field)
    lut = np.asarray(lut)
    ok = (field > 0) & (field < lut.size)
    new = np.zeros(field.shape, np.int32)
    new[ok] = lut[field[ok]]
    new[(new < 0) | (new > n_ev)] = 0
    T = field.shape[0]
    sums = np.zeros((T, n_ev, 5), np.int64)
    gid = np.zeros((T, n_ev), np.int32)
    for t in range(T):
        for ev in range(1, n_ev + 1):
            m = new[t] == ev
            if not m.any():
                continue
            sums[t, ev - 1, 0] = int(m.sum())
            for k in range(4):
                sums[t, ev - 1, k + 1] = q[k][m].sum(dtype=np.int64)
            gid[t, ev - 1] = field[t][m].max()
    return new, sums, gid


def cluster_rename(field, pairs, events, q, e, time_values):
    """Every variable of the events Dataset: ``ID_field`` int32 ``[T, C]``, ``global_ID`` int32, ``area`` float32 and
    ``presence`` bool ``[T, N]``, ``centroid`` float32 ``[2, T, N]`` (degrees), ``time_start`` / ``time_end`` ``[N]``,
    ``merge_ledger`` int32 ``[T, N, siblings]``, and ``N``.  ``events``: the dict of mesh_merge_oracle.merge_events."""
    field = np.asarray(field)
    time_values = np.asarray(time_values)
    T = field.shape[0]
    lut, N = event_table(field, pairs)
    new, sums, gid = rename_and_sums(field, lut, N, q)
    pres = gid > 0
    area = np.full((T, N), np.nan, np.float32)
    cen = np.full((2, T, N), np.nan, np.float32)
    for t in range(T):
        for k in np.nonzero(pres[t])[0]:
            a, c = mo._finish(sums[t, k, 1:].reshape(4, 1), e)
            area[t, k], cen[:, t, k] = a[0], c[:, 0]
    t_first = np.argmax(pres, axis=0)
    t_last = T - 1 - np.argmax(pres[::-1], axis=0)
    P = np.asarray(events["parent_IDs"])
    ledger = np.full((T, N + 1, P.shape[1]), -1, np.int32)  # event IDs 0 .. N; the column of 0 is dropped below
    for row, t in zip(P, np.asarray(events["merge_tidx"]).tolist()):
        old = np.where(row > 0, row, 0)
        mapped = lut[np.minimum(old, lut.size - 1)] * (old < lut.size)
        for p in mapped[mapped > 0]:  # result.loc[time, ID = parents] = parents broadcast over sibling_ID (track.py:3086-3093)
            ledger[t, p, :] = p
    return {"ID_field": new, "global_ID": gid, "area": area, "centroid": cen, "presence": pres,
            "time_start": time_values[t_first], "time_end": time_values[t_last], "merge_ledger": ledger[:, 1:, :], "N": N}
