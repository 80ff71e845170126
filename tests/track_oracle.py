"""Host oracle of the basic tracker (marEx.tracker(..., allow_merging=False).run(), track.py:1162-1497) for the tests:
the pre-processing functions of ``oracle.marex_oracle`` followed by a 3-D labelling with ``scipy.ndimage``.  Not a test
module (no ``test_`` prefix); the repository's ``oracle/`` package is left untouched."""
import numpy as np

from oracle import marex_oracle as orc


def label_3d(data_bin: np.ndarray, wrap_x: bool = True):
    """26-connected components in (time, y, x) (track.py:2006-2048, ``time_connectivity=True``), periodic in x when
    ``wrap_x``: ``ndi.label`` with a 3x3x3 structure of ones, then unions across the x seam for every (dt, dy) in
    {-1, 0, 1}^2, then IDs renumbered 1..N by each component's first cell in C order.  Returns ``(ids int32, N)``."""
    from scipy import ndimage as ndi
    from scipy.sparse import coo_matrix
    from scipy.sparse.csgraph import connected_components

    d = np.asarray(data_bin).astype(bool)
    T, ny, nx = d.shape
    lab, n = ndi.label(d, structure=np.ones((3, 3, 3), dtype=bool))
    if n == 0:
        return np.zeros(d.shape, dtype=np.int32), 0
    if wrap_x and nx > 1:
        a, b = [], []
        left, right = lab[:, :, 0], lab[:, :, nx - 1]
        for dt in (-1, 0, 1):
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
        lab = np.where(lab > 0, comp[lab] + 1, 0)  # any distinct positive value per component; renumbered below
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


def preprocess(extreme_events, mask, R_fill, T_fill, area_filter_quartile=0.5, area_filter_absolute=None, regional_mode=False):
    """``tracker.run_preprocess`` (track.py:1283-1368) on the host: ``(filtered, (total_area_IDed, N_objects_prefiltered,
    N_objects_filtered, area_threshold, accepted_area_fraction, preprocessed_area_fraction))``, areas in cells."""
    ev = np.asarray(extreme_events).astype(bool)
    a = orc.fill_holes(ev, mask, R_fill, regional_mode)
    g = orc.fill_time_gaps(a, mask, R_fill, T_fill, regional_mode)
    e, thr, areas, n0, n1 = orc.filter_small_objects(g, area_filter_quartile, area_filter_absolute, regional_mode)
    total = float(areas.sum())
    accepted = float(areas[areas > thr].sum())
    return e, (total, n0, n1, thr, accepted / total, float(ev.sum()) / float(e.sum()))


def run(extreme_events, mask, R_fill, T_fill, area_filter_quartile=0.5, area_filter_absolute=None, regional_mode=False):
    """The whole basic tracker: ``(ID_field int32, attrs)`` with the attrs of track.py:1451-1460."""
    e, st = preprocess(extreme_events, mask, R_fill, T_fill, area_filter_quartile, area_filter_absolute, regional_mode)
    ids, n = label_3d(e, wrap_x=not regional_mode)
    attrs = {"allow_merging": 0, "N_objects_prefiltered": st[1], "N_objects_filtered": st[2], "N_events_final": n,
             "R_fill": R_fill, "T_fill": T_fill,
             "area_filter_quartile": 0.0 if area_filter_absolute is not None else area_filter_quartile,
             "area_threshold (cells)": st[3], "accepted_area_fraction": st[4], "preprocessed_area_fraction": st[5]}
    return ids, attrs
