"""NumPy oracle of the severity categories of tracked events (``marex_event_categories_f32``,
``marex_amd.event_categories``): a direct restatement -- classify every cell, ``np.add.at`` into ``(t, ID)``, then the
per-event reductions.  Not collected by pytest."""
import numpy as np

CATEGORIES = ("below", "moderate", "strong", "severe", "extreme", "undefined")


def classify(anom, h):
    """The class of every element of ``anom`` float32 under the thresholds ``h`` float32 of the same shape: 6 for a
    non-finite anomaly, 5 where ``h`` is NaN, infinite or not positive, else how many of ``h``, ``2 h``, ``3 h``, ``4 h``
    (float32 products, one rounding each) the anomaly reaches."""
    a, h = np.asarray(anom, np.float32), np.asarray(h, np.float32)
    assert a.dtype == np.float32 and h.dtype == np.float32 and a.shape == h.shape
    with np.errstate(invalid="ignore", over="ignore"):
        h2, h3, h4 = np.float32(2) * h, np.float32(3) * h, np.float32(4) * h
        assert h2.dtype == np.float32
        k = (a >= h).astype(np.int8) + (a >= h2) + (a >= h3) + (a >= h4)
        k = np.where(np.isfinite(h) & (h > 0), k, 5)
    return np.where(np.isfinite(a), k, 6).astype(np.int8)


def step_peak(cells):
    """``cells [..., 7]`` -> the peak of the step: the highest of 1..4 with a cell, else 0 with a cell below, else 5."""
    peak = np.where(cells[..., 0] > 0, 0, 5).astype(np.uint8)
    for k in (1, 2, 3, 4):
        peak = np.where(cells[..., k] > 0, np.uint8(k), peak)
    return peak


def categories(ids, anom, thr, doy, w=None, n_ev=None, spans=None):
    """``ids`` int ``[T, C]``, ``anom`` float32 ``[T, C]``, ``thr`` float32 ``[n_doy, C]``, ``doy`` int ``[T]``, ``w`` float32
    ``[C]`` or None.  Events are 1 .. ``n_ev`` (default: the largest ID); anything else is background.  ``spans``:
    ``(tmin, tmax)`` per event 0..n_ev -- a cell of an event outside its span is lost (``status[0]``); every event cell of a
    row whose ``doy`` is outside ``0 .. n_doy - 1`` is lost (``status[1]``).  Lost cells count nowhere and are 0 in ``field``."""
    ids, anom, thr, doy = np.asarray(ids), np.asarray(anom, np.float32), np.asarray(thr, np.float32), np.asarray(doy)
    T, C = ids.shape
    N = int(max(ids.max(initial=0), 0)) if n_ev is None else int(n_ev)
    n_doy = thr.shape[0]
    cells = np.zeros((T, N + 1, 7), np.int64)
    area = np.zeros((T, N + 1, 6), np.float64)
    field = np.zeros((T, C), np.uint8)
    status = [0, 0]
    wd = np.ones(C) if w is None else np.asarray(w, np.float32).astype(np.float64)
    for t in range(T):
        ev = (ids[t] > 0) & (ids[t] <= N)
        if not 0 <= doy[t] < n_doy:
            status[1] += int(ev.sum())
            continue
        if spans is not None:
            e = np.where(ev, ids[t], 0)
            out = ev & ((t < np.asarray(spans[0])[e]) | (t > np.asarray(spans[1])[e]))
            status[0] += int(out.sum())
            ev &= ~out
        c = np.nonzero(ev)[0]
        k = classify(anom[t, c], thr[doy[t], c])
        np.add.at(cells[t], (ids[t, c], k), 1)
        cl = k < 6
        np.add.at(area[t], (ids[t, c][cl], k[cl]), wd[c][cl])
        field[t, c] = k + 1
    cells, area = cells[:, 1:], area[:, 1:]
    here = cells.sum(axis=2) > 0
    peak = np.where(here, step_peak(cells), 0).astype(np.uint8)
    warm = here & (peak >= 1) & (peak <= 4)
    ecat = np.where(warm, peak, 0).max(axis=0, initial=0).astype(np.uint8)
    step = np.full(N, -1, np.int64)
    for e in range(N):
        if ecat[e]:
            step[e] = int(np.argmax(warm[:, e] & (peak[:, e] == ecat[e])))
    steps = np.zeros((N, 6), np.int32)
    for t in range(T):  # one step after the other
        for e in np.nonzero(here[t])[0]:
            steps[e, step_peak(cells[t, e])] += 1
    earea = np.zeros((N, 6))
    for t in range(T):  # in ascending time, as the host finish adds the slots
        earea += area[t]
    return {"category_peak": peak, "category_cells": cells[..., :6].astype(np.uint32), "category_area": area,
            "slot_cells": cells, "event_category": ecat, "event_step_of_category": step,
            "event_category_cell_steps": cells[..., :6].sum(axis=0), "event_category_area": earea,
            "event_category_steps": steps, "event_invalid_cells": cells[..., 6].sum(axis=0),
            "category_field": field, "status": status, "event_duration": here.sum(axis=0).astype(np.int32)}
