"""Host oracle of the tracker's object stages (marEx.tracker methods compute_area, calculate_centroid,
calculate_object_properties, check_overlap_slice, find_overlapping_objects, enforce_overlap_threshold; gridded data),
restated in NumPy from their documented semantics for the tests.  Not a test module (no ``test_`` prefix).

The reference computes object properties with scikit-image's ``regionprops_table`` (not installed here).  Assumed
behaviour, that of scikit-image 0.20 or later:

* ``label`` is an integer column (int64 here); labels <= 0 are background;
* ``area`` is float64: the number of cells of the label;
* ``centroid`` is float64 ``(row, col)``: the mean of the cell indices, i.e. an integer sum divided once in float64
  (every partial sum is an integer below 2^53, so float64 accumulation is exact).

The reference processes one (y, x) slice per timestep and concatenates the tables in time order, so an ID occurs once
per timestep it lives in.  Its seam rule (calculate_centroid) replaces the column mean of an object that has a cell in
``mask[:, :100]`` and one in ``mask[:, -100:]`` -- bands that overlap for nx < 200 -- by the mean of the columns with
those right of ``nx // 2`` shifted by ``-nx``, plus ``nx`` when that mean is negative; not in ``regional_mode``.
"""
import logging

import numpy as np

I32_MAX = 2**31 - 1


def compute_area(data_bin) -> np.ndarray:
    """Cells per timestep of a (time, y, x) boolean array, int64."""
    return np.asarray(data_bin).astype(bool).sum(axis=(1, 2), dtype=np.int64)


def centroid(mask, regional_mode: bool = False):
    """``(y, x)`` centroid of one object's 2-D mask, object by object, with ``np.mean`` (the slow, literal form)."""
    m = np.asarray(mask).astype(bool)
    ys, xs = np.nonzero(m)
    y = np.mean(ys)
    if regional_mode or not (m[:, :100].any() and m[:, -100:].any()):
        return y, np.mean(xs)
    nx = m.shape[1]
    adj = np.where(xs > nx // 2, xs - nx, xs)
    x = np.mean(adj)
    return y, (x + nx if x < 0 else x)


def _slices(ids):
    a = np.asarray(ids)
    return a[None] if a.ndim == 2 else a


def object_properties_slow(ids, regional_mode: bool = False):
    """``(ID int64, area float64, centroid float64 [2, n])`` one object at a time (``ids == ID`` over the slice, as the
    reference does); only for small fields."""
    out_id, out_area, out_c = [], [], []
    for s in _slices(ids):
        for lab in np.unique(s[s > 0]):
            m = s == lab
            out_id.append(int(lab))
            out_area.append(float(m.sum()))
            out_c.append(centroid(m, regional_mode))
    c = np.array(out_c, dtype=np.float64).reshape(-1, 2).T
    return np.array(out_id, dtype=np.int64), np.array(out_area, dtype=np.float64), c


def object_properties(ids, regional_mode: bool = False):
    """The same table as :func:`object_properties_slow`, per slice with ``np.unique`` + ``np.bincount`` (float64 sums of
    integers, exact below 2^53) -- fast enough for whole fixtures."""
    out_id, out_area, out_c0, out_c1 = [], [], [], []
    for s in _slices(ids):
        ny, nx = s.shape
        ys, xs = np.nonzero(s > 0)
        if ys.size == 0:
            continue
        labs, inv = np.unique(s[ys, xs], return_inverse=True)
        k = labs.size
        n = np.bincount(inv, minlength=k).astype(np.float64)
        c0 = np.bincount(inv, weights=ys, minlength=k) / n
        c1 = np.bincount(inv, weights=xs, minlength=k) / n
        if not regional_mode:
            left = np.bincount(inv, weights=(xs < 100), minlength=k) > 0
            right = np.bincount(inv, weights=(xs >= nx - 100), minlength=k) > 0
            seam = left & right
            adj = np.bincount(inv, weights=np.where(xs > nx // 2, xs - nx, xs), minlength=k) / n
            adj = np.where(adj < 0, adj + nx, adj)
            c1 = np.where(seam, adj, c1)
        out_id.append(labs.astype(np.int64))
        out_area.append(n)
        out_c0.append(c0)
        out_c1.append(c1)
    if not out_id:
        return np.zeros(0, np.int64), np.zeros(0, np.float64), np.zeros((2, 0), np.float64)
    return np.concatenate(out_id), np.concatenate(out_area), np.stack([np.concatenate(out_c0), np.concatenate(out_c1)])


def check_overlap_slice(ids_t0, ids_next) -> np.ndarray:
    """``(n, 3)`` int32 ``[id_t0, id_next, cells]`` over the cells where both are > 0, sorted lexicographically."""
    a, b = np.asarray(ids_t0).astype(np.int64), np.asarray(ids_next).astype(np.int64)
    both = (a > 0) & (b > 0)
    if not both.any():
        return np.zeros((0, 3), np.int32)
    keys, counts = np.unique((a[both] << 32) | b[both], return_counts=True)
    return np.stack([keys >> 32, keys & 0xFFFFFFFF, counts], axis=1).astype(np.int32)


def find_overlapping_objects(ids) -> np.ndarray:
    """Pairs of slice t with slice t + 1 for t < T - 1, counts of equal pairs summed over time (int64, checked against
    int32), sorted lexicographically."""
    s = _slices(ids)
    parts = [check_overlap_slice(s[t], s[t + 1]).astype(np.int64) for t in range(s.shape[0] - 1)]
    parts = [p for p in parts if len(p)]
    if not parts:
        return np.zeros((0, 3), np.int32)
    allp = np.concatenate(parts)
    keys = (allp[:, 0] << 32) | allp[:, 1]
    uk, inv = np.unique(keys, return_inverse=True)
    tot = np.zeros(uk.size, np.int64)
    np.add.at(tot, inv.reshape(-1), allp[:, 2])
    assert tot.max() <= I32_MAX
    return np.stack([uk >> 32, uk & 0xFFFFFFFF, tot], axis=1).astype(np.int32)


def overlaps_brute_force(ids) -> np.ndarray:
    """:func:`find_overlapping_objects` by a double loop over timesteps and cells with a dict; tiny fields only."""
    s = _slices(ids)
    acc = {}
    for t in range(s.shape[0] - 1):
        for a, b in zip(s[t].reshape(-1).tolist(), s[t + 1].reshape(-1).tolist()):
            if a > 0 and b > 0:
                acc[(a, b)] = acc.get((a, b), 0) + 1
    rows = [(a, b, c) for (a, b), c in sorted(acc.items())]
    return np.array(rows, dtype=np.int32).reshape(-1, 3)


def enforce_overlap_threshold(overlaps, ids, areas, overlap_threshold, logger=None) -> np.ndarray:
    """Rows of ``overlaps`` whose IDs both have an area and whose ``overlap / min(area_0, area_1)`` is at least the
    threshold, in the input's dtype; ``(0, 3)`` int32 when none remain; fractions > 1 logged as a warning.  ``ids``
    must be unique."""
    ov = np.asarray(overlaps)
    if len(ov) == 0:
        return np.empty((0, 3), np.int32)
    area_of = dict(zip(np.asarray(ids).tolist(), np.asarray(areas, dtype=np.float64).tolist()))
    assert len(area_of) == len(ids)
    keep = np.array([r[0] in area_of and r[1] in area_of for r in ov.tolist()])
    if not keep.any():
        return np.empty((0, 3), np.int32)
    v = ov[keep]
    frac = np.array([float(r[2]) / min(area_of[r[0]], area_of[r[1]]) for r in v.tolist()])
    if (frac > 1.0).any():
        (logger or logging.getLogger("marex_amd")).warning(f"Found {int((frac > 1.0).sum())} overlap fractions > 1.0")
    return v[frac >= overlap_threshold]
