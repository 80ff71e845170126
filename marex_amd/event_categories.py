"""Severity categories of tracked events: which category every event of a tracker's ``ID_field`` reached, when, over how much
area, and the category map of every timestep.

Hobday et al. (2018) classify a marine heatwave by the multiples of the threshold its anomaly reaches: moderate, strong,
severe, extreme.  ``local_intensity(..., thresholds=)`` applies that rule per cell; here it is applied per event -- the join of
``ID_field``, ``dat_anomaly`` and ``thresholds`` that is otherwise a groupby loop on the host.  It is one streaming pass on the
device (``marex_event_categories_f32``) into the compact (timestep, event) slots of
:func:`marex_amd.event_intensity`: per slot the cells of every class and their area, and, optionally, one byte per cell of
the category field.  The host turns the slots into the Dataset, in ascending time.
"""
from __future__ import annotations

from typing import Optional

import numpy as np

from . import _stream, calendar, occurrence as mo
from ._stream import _I32_MAX, _Windows, _check_block_steps, event_spans, pad_events, slot_index, tracker_time, walk_event_slots
from .exceptions import TrackingError
from .intensity import _time_of_max_values, _validate
from .local_intensity import CATEGORIES, _device_thresholds, _threshold_layout, _thresholds_copied
from .track import _tensor_of

#: bytes of the device accumulators per (timestep, event) slot: seven uint64 counts and six float64 areas
SLOT_BYTES = 7 * 8 + 6 * 8


def _plan(ID_field, dat_anomaly, thresholds, cell_areas, block_steps, time: Optional[tuple]):
    """Everything that can be refused or derived without a device."""
    p = {"block_steps": _check_block_steps(block_steps), **_validate(ID_field, dat_anomaly, cell_areas)}
    tracker_time(p, time)
    shape, T, C, tv = p["shape"], p["T"], p["C"], p["tv"]
    dims = tuple(getattr(ID_field, "dims", ()) or ()) or tuple(getattr(dat_anomaly, "dims", ()) or ())
    kind = _threshold_layout(thresholds, shape[1:], dims[1:] if dims else None)
    doy = np.zeros(T, np.int32)
    if kind != "none":
        mo._calendar(tv, "thresholds by dayofyear")
        if T:
            doy = calendar._to_year_doy(tv)[1].astype(np.int32) - 1  # the row preprocess_data compares with
    if T and C and (C >= _I32_MAX or T >= _I32_MAX):
        raise TrackingError(f"event_categories: a timestep of {C} cells or a record of {T} steps reaches 2^31 - 1",
                            details="the field may hold any number of cells, a single timestep and the time axis may not")
    p.update(tv=np.asarray(tv), kind=kind, doy=doy,
             n_doy=1 if kind == "none" else calendar.N_DOY,
             sdims=dims[1:] if dims else (("y", "x") if len(shape) == 3 else ("cells",)))
    return p


def _device_pass(p, ID_field, dat_anomaly, thresholds, return_field: bool, device):
    """The two passes over the field: the events' spans, then the categories.  ``(N, tmin, off, cnt, area, field)``; the
    field stays on the device."""
    import torch

    from .detect import get_engine
    from .engine import HotPath

    eng = get_engine(device)
    T, C, w, n_doy = p["T"], p["C"], p["w"], p["n_doy"]
    ids_w = _Windows(eng, ID_field, T, C, np.int32, True)
    an_w = _Windows(eng, dat_anomaly, T, C, np.float32, False)
    per_step = ids_w.upload_bytes_per_step + an_w.upload_bytes_per_step
    thr_copy = _thresholds_copied(eng, thresholds, p["kind"])
    fixed = (4 * n_doy * C if thr_copy else 0) + (T * C if return_field else 0)

    def plan(slots: int) -> int:
        """The steps per window beside ``slots`` slots; :class:`TrackingError` when not even one fits."""
        return _stream._window_steps(
            eng, "event_categories", T, C, per_step, fixed + SLOT_BYTES * slots, p["block_steps"],
            f"{n_doy} x {C} float32 thresholds{'' if thr_copy else ' (resident already)'}, {slots} (timestep, event) "
            f"slots of {SLOT_BYTES} bytes, {'the category field of ' + str(T) + ' x ' + str(C) + ' bytes, ' if return_field else ''}"
            f"and the ID field and the anomalies of {T} timesteps, 4 bytes per cell each, as far as they are not on "
            "the device already", ["Pass return_field=False"] if return_field else [])

    B = plan(0)  # before anything is uploaded: the windows of both passes
    N, tmin, tmax, wins, kept = event_spans(eng, ids_w, T, B)
    if N <= 0:
        field = torch.zeros((T, C), dtype=torch.uint8, device=eng.device) if return_field else None
        return 0, tmin, np.zeros(2, np.int64), np.zeros((0, 7), np.int64), None, field
    plan(int(HotPath.event_slot_plan(tmin, tmax)[-1]))  # once more now that the slots are known, for its refusal alone
    thr = _device_thresholds(eng, thresholds, p["kind"], n_doy, C)
    wd = None if w is None else torch.from_numpy(w).to(eng.device)
    field = HotPath._buf(None, "cat_field", (T, C), torch.uint8, eng.device) if return_field else None
    r = walk_event_slots(ids_w, wins, kept, lambda x, a, b, acc, finish: eng.event_categories(
        x, an_w.get(a, b), tmin, tmax, thr, p["doy"], wd, t0=a, field=field, acc=acc, finish=finish))
    return N, tmin, r["off"], r["cat_cnt"], r["cat_area"], field


def step_peak(cnt: np.ndarray) -> np.ndarray:
    """The peak class of every slot of ``cnt [n, 7]``: the highest of 1..4 with a cell, else 0 where a cell was below the
    threshold, else 5 (undefined: only cells without a usable threshold or anomaly)."""
    peak = np.where(cnt[:, 0] > 0, 0, 5).astype(np.uint8)
    for k in (1, 2, 3, 4):
        peak[cnt[:, k] > 0] = k
    return peak


def _finish(p, N: int, tmin, off, cnt, area, per_timestep: bool):
    """The Dataset from the compact slots, in ascending time per event (the slots of an event are in time order, and
    ``np.add.at`` adds one element after the other)."""
    from .xr_compat import DataArray, Dataset

    T, tname, tv = p["T"], p["tname"], p["tv"]
    idc = {"ID": ("ID", np.arange(1, N + 1, dtype=np.int32))}
    cc = {"category": ("category", np.array(CATEGORIES))}
    tid = {p["tcoord"] or tname: (tname, tv), **idc, **cc}
    e_of, t_of = slot_index(off, tmin, N)
    cnt = cnt.astype(np.int64)
    here = cnt.sum(axis=1) > 0
    peak = step_peak(cnt)
    data = {}
    if per_timestep:
        def dense(v, dt):
            d = np.zeros((T, N) + v.shape[1:], dt)
            d[t_of[here], e_of[here] - 1] = v[here]
            return DataArray(d, dims=(tname, "ID") + (("category",) if v.ndim == 2 else ()), coords=tid)

        data["category_peak"] = dense(peak, np.uint8)
        data["category_cells"] = dense(cnt[:, :6], np.uint32)
        if area is not None:
            data["category_area"] = dense(area, np.float64)
    warm = here & (peak >= 1) & (peak <= 4)
    ecat = np.zeros(N + 1, np.uint8)
    np.maximum.at(ecat, e_of[warm], peak[warm])
    first = np.full(N + 1, np.iinfo(np.int64).max, np.int64)
    at = warm & (peak == ecat[e_of])
    np.minimum.at(first, e_of[at], t_of[at])
    cells = np.zeros((N + 1, 6), np.int64)
    np.add.at(cells, e_of, cnt[:, :6])
    earea = np.zeros((N + 1, 6), np.float64)
    if area is not None:
        np.add.at(earea, e_of, area)
    else:
        earea = cells.astype(np.float64)
    steps = np.zeros((N + 1, 6), np.int32)
    np.add.at(steps, (e_of[here], peak[here]), 1)
    invalid = np.zeros(N + 1, np.int64)
    np.add.at(invalid, e_of, cnt[:, 6])
    ic = {**idc, **cc}
    data["event_category"] = DataArray(ecat[1:], dims=("ID",), coords=idc)
    data["event_time_of_category"] = DataArray(_time_of_max_values(tv, first[1:], ecat[1:] > 0), dims=("ID",), coords=idc)
    data["event_category_cell_steps"] = DataArray(cells[1:], dims=("ID", "category"), coords=ic)
    data["event_category_area"] = DataArray(earea[1:], dims=("ID", "category"), coords=ic)
    data["event_category_steps"] = DataArray(steps[1:], dims=("ID", "category"), coords=ic)
    data["event_invalid_cells"] = DataArray(invalid[1:], dims=("ID",), coords=idc)
    return Dataset(data, coords=tid)


def _event_categories(ID_field, dat_anomaly, thresholds, cell_areas, per_timestep, return_field, block_steps, device,
                      n_events: Optional[int] = None, time: Optional[tuple] = None):
    from .xr_compat import DataArray

    p = _plan(ID_field, dat_anomaly, thresholds, cell_areas, block_steps, time)
    T, C, weighted = p["T"], p["C"], p["w"] is not None
    field = None
    if T == 0 or C == 0:
        N, tmin, off, cnt, area = 0, np.zeros(1, np.int64), np.zeros(2, np.int64), np.zeros((0, 7), np.int64), None
        if return_field:
            field = np.zeros((T, C), np.uint8)
    else:
        N, tmin, off, cnt, area, field = _device_pass(p, ID_field, dat_anomaly, thresholds, bool(return_field), device)
    if area is None and weighted:
        area = np.zeros((cnt.shape[0], 6), np.float64)
    N, tmin, off = pad_events("event_categories", N, n_events, tmin, off)
    ds = _finish(p, N, tmin, off, cnt, area, bool(per_timestep))
    if return_field:
        on_device = type(field).__module__.startswith("torch")  # an empty field has a NumPy one
        if not (on_device and _tensor_of(ID_field) is not None):
            field = field.cpu().numpy() if on_device else field
        ds["category_field"] = DataArray(field.reshape(p["shape"]), dims=(p["tname"],) + tuple(p["sdims"]),
                                         coords={p["tcoord"] or p["tname"]: (p["tname"], p["tv"])})
    return ds


def event_categories(ID_field, dat_anomaly, thresholds, cell_areas=None, per_timestep: bool = False, return_field: bool = False,
                     block_steps=None, device: int = 0):
    """Which severity category (Hobday et al. 2018) every tracked event reached, when, and over how many cells and how
    much area, from one pass over the event field, the anomaly field and the thresholds on the device.

    ``ID_field``, ``dat_anomaly``, ``cell_areas``, ``block_steps``: as in :func:`marex_amd.event_intensity` (host or device
    resident, ``(time, y, x)`` or ``(time, cells)``; the results do not depend on ``block_steps``).  ``thresholds``: the
    ``thresholds`` of ``preprocess_data`` in any of its layouts, as in :func:`marex_amd.local_intensity` --
    ``(*space, dayofyear)``, ``(dayofyear, *space)`` (both need a datetime64 time coordinate) or ``(*space)`` alone
    (``global_extreme``; float64 is rounded to float32).  Everything is checked before any device work; the device memory
    the call needs (thresholds, 104 bytes per (timestep, event) slot, one byte per cell of the returned field, the windows)
    is checked before it is allocated (:class:`TrackingError` with the figures).

    With the threshold ``h`` of the step and cell and the float32 products ``2 h``, ``3 h``, ``4 h`` a cell of an event with
    a finite anomaly ``a`` is *below* for ``a < h``, *moderate* for ``h <= a < 2 h``, *strong* up to ``3 h``, *severe* up to
    ``4 h``, *extreme* from ``4 h``, and *undefined* where ``h`` is NaN, infinite or not positive -- the rule of
    ``local_intensity``.  A cell whose anomaly is NaN or infinite is counted in ``event_invalid_cells`` only.

    Returns a Dataset over ``ID = 1 .. N`` (N: the largest event number) and ``category`` (the six names above):
    ``event_category`` (uint8: the highest of 1..4 that any cell of the event reached at any step, else 0),
    ``event_time_of_category`` (the first time value at which it was reached; NaT, or NaN on a non-datetime axis, where the
    category is 0), ``event_category_cell_steps`` (int64 ``[ID, category]``: cells x timesteps), ``event_category_area``
    (float64 ``[ID, category]``: area x timesteps; the counts as float64 without ``cell_areas``), ``event_category_steps``
    (int32 ``[ID, category]``: the timesteps by their peak -- the highest of 1..4 present at the step, else 0 if a cell was
    below the threshold, else 5; its sum over ``category`` is ``event_duration`` of ``event_intensity``) and
    ``event_invalid_cells`` (int64).

    ``per_timestep=True`` adds ``category_peak`` (uint8 ``(time, ID)``: the step peak, 0 where the event is absent),
    ``category_cells`` (uint32 ``(time, ID, category)``) and, with ``cell_areas``, ``category_area`` (float64 ``(time, ID,
    category)``).  These are dense and six times the size of ``event_intensity``'s per-timestep arrays, which is why the
    default here is False.

    ``return_field=True`` adds ``category_field`` (uint8 over ``(time, *space)``): 0 where a cell belongs to no event, else
    1 + the class (1 below .. 5 extreme, 6 undefined, 7 a non-finite anomaly) -- the category map of every day.  It is a
    device tensor when ``ID_field`` was device resident, a NumPy array otherwise.

    Counts and the field are exact; the areas are float64 sums of exact terms under the contract of ``event_intensity``."""
    return _event_categories(ID_field, dat_anomaly, thresholds, cell_areas, per_timestep, return_field, block_steps, device)
