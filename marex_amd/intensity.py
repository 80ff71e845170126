"""Per-event intensity metrics: the events of a tracker's ``ID_field`` joined with the anomaly field they were detected in.

The reference leaves this step to notebook code (``groupby`` / ``where`` over ``ID_field`` and ``dat_anomaly``; its docs
list "statistical summaries (event frequency, duration, intensity)" as the third step of the workflow).  Here it is one
streaming pass on the device (``marex_event_intensity_f32``): per (timestep, event) the finite cells,
the sum of the cell weights, the sum of weight x anomaly and the largest anomaly, into compact slots -- one per timestep
between an event's first and last.  The host turns the slots into the Dataset in float64, in ascending time.
"""
from __future__ import annotations

from typing import Optional

import numpy as np

from ._keys import float_key, key_float  # noqa: F401 -- public here
from ._stream import (_I32_MAX, _Windows, _check_block_steps, _dtype_name, _kind, _plan_windows, _time_of, event_spans,
                      pad_events, slot_index, spatial, tracker_time, walk_event_slots, weighted_mean)
from .exceptions import TrackingError, create_data_validation_error


def _validate(ID_field, dat_anomaly, cell_areas):
    """Everything that can be refused without a device: the plan -- ``shape``, ``T``, ``C``, the time axis ``tname`` / ``tv``
    and the weights ``w``, float32 ``[C]`` or None."""
    shape = tuple(int(k) for k in ID_field.shape)
    if len(shape) not in (2, 3):
        raise create_data_validation_error("ID_field must be (time, y, x) or (time, cells)", details=f"got shape {shape}")
    ashape = tuple(int(k) for k in dat_anomaly.shape)
    if ashape != shape:
        raise create_data_validation_error("ID_field and dat_anomaly differ in shape", details=f"ID_field {shape}, dat_anomaly {ashape}")
    d_i, d_a = tuple(getattr(ID_field, "dims", ()) or ()), tuple(getattr(dat_anomaly, "dims", ()) or ())
    if d_i and d_a and d_i != d_a:
        raise create_data_validation_error("ID_field and dat_anomaly differ in their dimensions",
                                           details=f"ID_field {d_i}, dat_anomaly {d_a}; the order must agree too")
    if _kind(ID_field) != "i":
        raise create_data_validation_error("Object IDs must be integers", details=f"Found dtype {_dtype_name(ID_field)}",
                                           data_info={"actual_dtype": _dtype_name(ID_field)})
    if _kind(dat_anomaly) != "f":
        raise create_data_validation_error("dat_anomaly must be a floating-point field",
                                           details=f"Found dtype {_dtype_name(dat_anomaly)}",
                                           data_info={"actual_dtype": _dtype_name(dat_anomaly)})
    T = shape[0]
    tname, tv = _time_of(ID_field, T)
    _, tv_a = _time_of(dat_anomaly, T)
    if tv is not None and tv_a is not None and not np.array_equal(tv, tv_a):
        raise create_data_validation_error("ID_field and dat_anomaly differ in their time coordinate",
                                           details=f"the first difference is at step {int(np.argmax(tv != tv_a))}")
    tv = tv if tv is not None else tv_a if tv_a is not None else np.arange(T)
    w = None
    if cell_areas is not None:
        w = spatial(cell_areas, {"shape": shape, "labelled": bool(d_i), "sdims": d_i[1:]}, "cell_areas", True,
                    "cell_areas do not match the spatial shape of ID_field", numbers=True).astype(np.float32)
        if not np.isfinite(w).all() or (w < 0).any():
            raise create_data_validation_error("cell_areas must be finite and non-negative",
                                               details=f"{int((~np.isfinite(w)).sum())} non-finite, {int((w < 0).sum())} negative")
    return {"shape": shape, "T": T, "C": int(np.prod(shape[1:])), "tname": tname, "tv": tv, "w": w}


def _no_slots():
    return 0, np.zeros(1, np.int64), np.zeros(2, np.int64), np.zeros((0, 2), np.int64), np.zeros((0, 2)), np.zeros(0, np.float32)


def _device_slots(eng, ID_field, dat_anomaly, w, T: int, C: int, block_steps):
    """The two passes over the field: the events' spans, then the sums.  ``(N, tmin, off, cnt, sums, vmax)`` on the host."""
    import torch

    ids_w = _Windows(eng, ID_field, T, C, np.int32, True)
    an_w = _Windows(eng, dat_anomaly, T, C, np.float32, False)
    B = _plan_windows(eng, T, C, ids_w.upload_bytes_per_step + an_w.upload_bytes_per_step, block_steps)

    N, tmin, tmax, wins, kept = event_spans(eng, ids_w, T, B)
    if N <= 0:
        return _no_slots()
    wd = None if w is None else torch.from_numpy(w).to(eng.device)
    r = walk_event_slots(ids_w, wins, kept, lambda x, a, b, acc, finish: eng.event_intensity(
        x, an_w.get(a, b), tmin, tmax, wd, t0=a, acc=acc, finish=finish))
    return N, tmin, r["off"], r["cnt"], r["sums"], r["vmax"]


def _time_of_max_values(tv: np.ndarray, t_idx: np.ndarray, has: np.ndarray) -> np.ndarray:
    """``tv[t_idx]`` with a missing value where ``has`` is False: NaT for dates, NaN otherwise (an integer axis then
    becomes float64)."""
    out = tv[np.where(has, t_idx, 0)] if tv.size else tv[:0]
    if has.all():
        return out
    if out.dtype.kind in "mM":
        out = out.copy()
        out[~has] = np.array("NaT", dtype=out.dtype)
        return out
    out = out.astype(np.float64)
    out[~has] = np.nan
    return out


def _finish(N: int, T: int, tmin, off, cnt, sums, vmax, tname: str, tv, per_timestep: bool, tcoord: Optional[str] = None):
    """The Dataset from the compact slots, in float64 and in ascending time per event (the slots of an event are in time
    order, and ``np.add.at`` adds one element after the other)."""
    from .xr_compat import DataArray, Dataset

    tv = np.asarray(tv)
    ids = np.arange(1, N + 1, dtype=np.int32)
    idc = {"ID": ("ID", ids)}
    tid = {tcoord or tname: (tname, tv), **idc}
    e_of, t_of = slot_index(off, tmin, N)
    fin, bad = cnt[:, 0], cnt[:, 1]
    W, S = sums[:, 0], sums[:, 1]
    here = (fin + bad) > 0
    some = fin > 0
    ratio = weighted_mean(some, W, S)
    data = {}
    if per_timestep:
        def dense(v, dt, fill):
            d = np.full((T, N), fill, dt)
            d[t_of[here], e_of[here] - 1] = v[here]
            return DataArray(d, dims=(tname, "ID"), coords=tid)

        data["intensity_max"] = dense(np.where(some, vmax, np.float32(np.nan)).astype(np.float32), np.float32, np.nan)
        data["intensity_mean"] = dense(ratio.astype(np.float32), np.float32, np.nan)
        data["intensity_integral"] = dense(np.where(some, S, np.nan), np.float64, np.nan)
        data["intensity_cells"] = dense(fin.astype(np.int64), np.int64, 0)
    duration = np.bincount(e_of[here], minlength=N + 1)[1:N + 1].astype(np.int32)
    emax = np.full(N + 1, -np.inf, np.float64)
    np.maximum.at(emax, e_of[some], vmax[some].astype(np.float64))
    has = np.zeros(N + 1, bool)
    has[e_of[some]] = True
    first = np.full(N + 1, np.iinfo(np.int64).max, np.int64)
    at_max = some & (vmax.astype(np.float64) == emax[e_of])
    np.minimum.at(first, e_of[at_max], t_of[at_max])
    sS, sW, cum = np.zeros(N + 1), np.zeros(N + 1), np.zeros(N + 1)
    np.add.at(sS, e_of[some], S[some])
    np.add.at(sW, e_of[some], W[some])
    ok = ~np.isnan(ratio)
    np.add.at(cum, e_of[ok], ratio[ok])
    has_w = np.zeros(N + 1, bool)
    has_w[e_of[ok]] = True
    emean = weighted_mean(has, sW, sS)
    invalid = np.zeros(N + 1, np.int64)
    np.add.at(invalid, e_of, bad)
    data["event_duration"] = DataArray(duration, dims=("ID",), coords=idc)
    data["event_intensity_max"] = DataArray(np.where(has, emax, np.nan)[1:].astype(np.float32), dims=("ID",), coords=idc)
    data["event_time_of_max"] = DataArray(_time_of_max_values(tv, first[1:], has[1:]), dims=("ID",), coords=idc)
    data["event_intensity_mean"] = DataArray(emean[1:].astype(np.float32), dims=("ID",), coords=idc)
    data["event_intensity_cumulative"] = DataArray(np.where(has_w, cum, np.nan)[1:].astype(np.float32), dims=("ID",), coords=idc)
    data["event_invalid_cells"] = DataArray(invalid[1:], dims=("ID",), coords=idc)
    return Dataset(data, coords=tid)


def _event_intensity(ID_field, dat_anomaly, cell_areas, per_timestep, block_steps, device, n_events: Optional[int] = None,
                     time: Optional[tuple] = None):
    block_steps = _check_block_steps(block_steps)
    p = _validate(ID_field, dat_anomaly, cell_areas)
    tracker_time(p, time)
    T, C = p["T"], p["C"]
    if T == 0 or C == 0:
        N, tmin, off, cnt, sums, vmax = _no_slots()
    else:
        if C >= _I32_MAX or T >= _I32_MAX:
            raise TrackingError(f"event_intensity: a timestep of {C} cells or a record of {T} steps reaches 2^31 - 1",
                                details="the field may hold any number of cells, a single timestep and the time axis may not")
        from .detect import get_engine

        N, tmin, off, cnt, sums, vmax = _device_slots(get_engine(device), ID_field, dat_anomaly, p["w"], T, C, block_steps)
    N, tmin, off = pad_events("event_intensity", N, n_events, tmin, off)
    return _finish(N, T, tmin, off, cnt, sums, vmax, p["tname"], p["tv"], bool(per_timestep), p["tcoord"])


def event_intensity(ID_field, dat_anomaly, cell_areas=None, per_timestep: bool = True, block_steps=None, device: int = 0):
    """How strong every tracked event was: maximum, mean and cumulative intensity and duration, from one pass over the
    event field and the anomaly field on the device.

    ``ID_field``: an integer event field of the trackers, ``(time, y, x)`` or ``(time, cells)``; the positive values are
    the event numbers (a negative value is refused, as by the trackers' other methods).  ``dat_anomaly``: the anomalies,
    float32 (other float types are cast), same shape and dimension order.  Either may be a host array or DataArray, or
    device resident (then it is read in place).  ``cell_areas``: None (every cell weighs 1), or non-negative float32 areas
    per cell -- ``[C]``, ``[ny, nx]`` or ``[ny]`` (broadcast along x), an array or a DataArray.

    ``block_steps``: None takes the field whole (:class:`TrackingError` with both numbers when it does not fit the device
    memory); a number uploads host inputs one window of that many timesteps at a time, and walks resident inputs in those
    windows; ``"auto"`` takes the largest window the free memory allows.  The results do not depend on it.

    Returns a Dataset over ``time`` and ``ID = 1 .. N`` (N: the largest event number).  With ``per_timestep``, dense
    ``(time, ID)`` like the trackers' ``area``, NaN where the event is absent: ``intensity_max`` (float32),
    ``intensity_mean`` (float32 of S / W; NaN without a finite cell or with W = 0), ``intensity_integral`` (float64 S, the
    sum of anomaly x area -- anomaly x cells without areas) and ``intensity_cells`` (int64, the finite cells; 0 where
    absent).  Always, per ``ID``: ``event_duration`` (int32, timesteps with at least one cell, finite or not),
    ``event_intensity_max`` (float32), ``event_time_of_max`` (the first time value reaching it), ``event_intensity_mean``
    (float32 of sum S / sum W), ``event_intensity_cumulative`` (float32 of the float64 sum of S_t / W_t in ascending t over
    the steps with W_t > 0: anomaly x timesteps, degree-days on a daily axis) and ``event_invalid_cells`` (int64, cells
    whose anomaly is NaN or infinite: they count for the duration and for nothing else).  S and W are float64 sums of exact
    terms (DESIGN.md section 4 has the bound); counts and maxima are exact."""
    return _event_intensity(ID_field, dat_anomaly, cell_areas, per_timestep, block_steps, device)
