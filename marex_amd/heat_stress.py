"""Accumulated heat stress: the Degree Heating Week (DHW) of NOAA Coral Reef Watch (Liu et al. 2014, Skirving et al. 2020)
and its bleaching alert levels, per cell, from the raw SST.

The percentile statistics of this package -- ``cell_events``, ``local_intensity``, ``event_categories`` -- all accumulate
under a presence field.  The DHW is the other standard measure of marine heat and needs none: the HotSpot is the SST
minus the maximum of the monthly mean climatology (MMM), counted from 1 K on, and the DHW its running sum over twelve
weeks, in K-weeks.  Both come from streaming passes on the device (``marex_group_mean_f32`` and ``marex_heat_stress_f32``,
DESIGN.md section 4): a lane owns a cell, the running sum is exact in float64, and the results do not depend on the time
windows the field is walked in, not in any bit.  The month of every step, the baseline and the group labels are derived on
the host.
"""
from __future__ import annotations

import numpy as np

from . import _stream, occurrence as mo
from ._stream import _Windows, _check_block_steps
from .exceptions import ConfigurationError, create_data_validation_error
from .track import _host, _tensor_of

MAX_WINDOW, MAX_LEVELS = 366, 6
HOTSPOT_MIN_LOW, HOTSPOT_LIMIT = 2.0 ** -10, 1024.0


def accumulator_bytes(G: int, C: int, L: int) -> int:
    """The per-cell accumulators of the device pass: the two maxima, the step of the first and the invalid steps (4 bytes
    each), ``3 + L`` class counts and ``max(L, 1)`` onsets."""
    return int(G) * int(C) * (16 + 4 * (3 + int(L)) + 4 * max(int(L), 1))


def _check_args(window, steps_per_week, hotspot_min, levels) -> dict:
    """The arguments of the accumulation; their bounds are what makes the running sum exact."""
    w = window.item() if isinstance(window, np.generic) else window
    if isinstance(w, bool) or not isinstance(w, int) or not 1 <= w <= MAX_WINDOW:
        raise ConfigurationError(f"window must be an integer in 1 .. {MAX_WINDOW} timesteps", details=f"window={window!r}")
    try:
        spw = float(steps_per_week)
    except (TypeError, ValueError):
        spw = np.nan
    if isinstance(steps_per_week, bool) or not (np.isfinite(spw) and spw > 0):
        raise ConfigurationError("steps_per_week must be a finite number above 0", details=f"steps_per_week={steps_per_week!r}")
    try:
        hmin = float(np.float32(hotspot_min))
    except (TypeError, ValueError):
        hmin = np.nan
    if isinstance(hotspot_min, bool) or not HOTSPOT_MIN_LOW <= hmin < HOTSPOT_LIMIT:
        raise ConfigurationError("hotspot_min must satisfy 2^-10 <= hotspot_min < 1024",
                                 details=f"hotspot_min={hotspot_min!r}; the bounds keep the running sum exact")
    try:
        lev = np.asarray(levels, dtype=np.float32).reshape(-1)
    except (TypeError, ValueError):
        lev = np.full(1, np.nan, np.float32)
    if lev.size > MAX_LEVELS or not np.isfinite(lev).all() or not (np.diff(lev) > 0).all():
        raise ConfigurationError(f"levels must be 0 .. {MAX_LEVELS} finite float32 values, strictly increasing",
                                 details=f"levels={levels!r}")
    return {"window": int(w), "spw": spw, "hmin": hmin, "levels": lev}


def month_labels(p: dict, baseline, months, what: str) -> np.ndarray:
    """int32 ``[T]``: the month 0 .. 11 of every step of the planned field, -1 outside the ``baseline``."""
    T, tv = p["T"], p["tv"]
    dated = tv is not None and np.asarray(tv).dtype.kind == "M"
    if months is not None:
        a = np.asarray(_host(months))
        if a.ndim != 1 or a.shape[0] != T or a.dtype.kind not in "iu":
            raise create_data_validation_error("months must be one integer per timestep", details=f"got {a.dtype} {a.shape} for {T} timesteps")
        if a.size and (int(a.min()) < 1 or int(a.max()) > 12):
            raise create_data_validation_error("months must hold 1 .. 12", details=f"found {int(a.min())} .. {int(a.max())}")
        lab = a.astype(np.int64) - 1
    elif dated:
        lab = mo._calendar(tv, what)[1] - 1
    else:
        raise ConfigurationError(f"{what} needs a datetime time coordinate or months=, the month 1 .. 12 of every timestep",
                                 details="the field carries no calendar")
    if baseline is not None:
        b = baseline
        if isinstance(b, (tuple, list)) and len(b) == 2 and all(isinstance(k, (int, np.integer)) and not isinstance(k, bool) for k in b):
            if b[0] > b[1]:
                raise ConfigurationError("baseline=(first_year, last_year) must be ascending", details=f"baseline={baseline!r}")
            year = mo._calendar(tv, "baseline=(first_year, last_year)")[0]
            keep = (year >= b[0]) & (year <= b[1])
        else:
            keep = np.asarray(_host(b))
            if keep.dtype != np.bool_ or keep.shape != (T,):
                raise ConfigurationError("baseline must be None, (first_year, last_year) or one bool per timestep",
                                         details=f"got {getattr(keep, 'dtype', None)} {getattr(keep, 'shape', None)} for {T} timesteps")
        lab = np.where(keep, lab, -1)
    if T and not (lab >= 0).any():
        raise create_data_validation_error("baseline selects no timestep", details=f"baseline={baseline!r} over {T} timesteps")
    return lab.astype(np.int32)


def climatology_of(total, cnt):
    """``(monthly_mean float64 [12, C], mmm float32 [C], mmm_month uint8 [C])`` of the float64 sums and the counts: one
    division per (month, cell), NaN without a sample; the maximum over the months that have one, rounded to float32, and the
    first month 1 .. 12 that attains it (NaN and 0 where no month has a sample)."""
    has = cnt > 0
    with np.errstate(invalid="ignore", divide="ignore"):
        mean = np.where(has, total / np.where(has, cnt, 1).astype(np.float64), np.nan)
    some = has.any(axis=0)
    low = np.where(has, mean, -np.inf)
    top = low.max(axis=0)
    first = (has & (low == top[None])).argmax(axis=0)
    with np.errstate(over="ignore"):
        mmm = np.where(some, top, np.nan).astype(np.float32)
    return mean, mmm, np.where(some, first + 1, 0).astype(np.uint8)


def _engine(device):
    from .detect import get_engine

    return get_engine(0 if device is None else device)


def _climatology_pass(p, eng, sst_w, lab):
    """``(sum float64, cnt uint32) [12, C]`` of the labelled steps: the result of ``HotPath.group_mean``."""
    T, C = p["T"], p["C"]
    used = np.flatnonzero(lab >= 0)
    lo, hi = int(used[0]), int(used[-1]) + 1
    per_step = sst_w.upload_bytes_per_step
    B = _stream._window_steps(eng, "monthly_maximum_climatology", hi - lo, C, per_step, 12 * 12 * C + 4 * T, p["block_steps"],
                              f"12 x {C} cells of 12 bytes (sum, count) and the field of {hi - lo} timesteps, 4 bytes per cell, as "
                              "far as it is not on the device already", ["Narrow the baseline"])
    acc = r = None
    for a in range(lo, hi, B):
        b = min(hi, a + B)
        r = eng.group_mean(sst_w.get(a, b), lab, 12, t0=a, acc=acc, finish=b >= hi)
        acc = r["acc"]
    return r["sum"], r["cnt"]


def _climatology(p, sst, lab, device, eng=None, sst_w=None):
    T, C = p["T"], p["C"]
    if T == 0 or C == 0:
        return (*climatology_of(np.zeros((12, C)), np.zeros((12, C), np.uint32)), np.zeros((12, C), np.uint32), eng, sst_w)
    eng = eng or _engine(device)
    sst_w = sst_w or _Windows(eng, sst, T, C, np.float32, False)
    total, cnt = _climatology_pass(p, eng, sst_w, lab)
    return (*climatology_of(total, cnt), cnt, eng, sst_w)


def _monthly_maximum_climatology(sst, baseline, months, block_steps, device):
    from .xr_compat import Dataset

    what = "monthly_maximum_climatology"
    p = {"block_steps": _check_block_steps(block_steps), **_stream.plan_float_field(sst, what)}
    lab = month_labels(p, baseline, months, what)
    mean, mmm, month, cnt, _, _ = _climatology(p, sst, lab, device)
    mc = {"month": ("month", np.arange(1, 13, dtype=np.int64))}
    return Dataset({"monthly_mean": _stream.space(p, mean, ("month",), mc), "monthly_count": _stream.space(p, cnt, ("month",), mc),
                    "mmm": _stream.space(p, mmm), "mmm_month": _stream.space(p, month)},
                   attrs={"baseline_steps": int((lab >= 0).sum())})


def monthly_maximum_climatology(sst, baseline=None, months=None, block_steps=None, device=None):
    """The maximum of the monthly mean climatology (MMM) of every cell: the threshold of the HotSpot and the Degree Heating
    Week of NOAA Coral Reef Watch, from one pass over the baseline's steps on the device.

    ``sst``: a float field ``(time, y, x)`` or ``(time, cells)``, a DataArray, an array or a device tensor, on the host or
    device resident (then it is read in place); it is read as float32.  The month of every step comes from the datetime64
    time coordinate, or from ``months``, an integer ``[time]`` of 1 .. 12 for a field without a calendar; with neither:
    :class:`ConfigurationError`.  ``baseline``: None (every step), ``(first_year, last_year)`` inclusive (needs the
    calendar) or one bool per step.  ``block_steps``: as in :func:`marex_amd.event_intensity`; the results do not depend
    on it, not even in the last bit.

    Returns ``monthly_count`` (uint32 ``[month, space]``: the finite samples), ``monthly_mean`` (float64: the float64 sum of
    the finite float32 samples in ascending time, one addition per sample, divided once by the count; NaN where the count
    is 0), ``mmm`` (float32 ``[space]``: the largest monthly mean over the months that have a sample; NaN where none has)
    and ``mmm_month`` (uint8: the first month 1 .. 12 that attains it; 0 where none)."""
    return _monthly_maximum_climatology(sst, baseline, months, block_steps, device)


def _mmm_vector(mmm, p):
    """The given climatology as float32 ``[C]``."""
    if _stream._kind(mmm) != "f":
        raise create_data_validation_error("mmm must be a floating-point map over the cells of a timestep",
                                           details=f"Found dtype {_stream._dtype_name(mmm)}")
    with np.errstate(over="ignore"):
        return _stream.spatial(mmm, p, "mmm").astype(np.float32)


def _plan(sst, mmm, baseline, months, window, steps_per_week, hotspot_min, levels, by, block_steps):
    """Everything that can be refused or derived without a device."""
    p = {"block_steps": _check_block_steps(block_steps), **_check_args(window, steps_per_week, hotspot_min, levels),
         **_stream.plan_float_field(sst, "heat_stress")}
    if mmm is not None:
        p["m"], p["lab"] = _mmm_vector(mmm, p), None
    else:
        p["m"], p["lab"] = None, month_labels(p, baseline, months, "heat_stress without mmm")
    p["grp"] = None if by is None else mo.group_labels(by, p["tv"], p["T"])
    return p


def _device_pass(p, sst, return_dhw, return_alert, device):
    """The device passes: the result of ``HotPath.heat_stress`` on the host, ``m``, ``dhw`` and ``alert``."""
    T, C, W, lev = p["T"], p["C"], p["window"], p["levels"]
    L = int(lev.size)
    G = 1 if p["grp"] is None else p["grp"][1]
    m = p["m"]
    if T == 0 or C == 0:
        if m is None:
            m = np.full(C, np.nan, np.float32)
        return {"m": m, "dhw_max": np.full((G, C), np.nan, np.float32), "tmax": np.full((G, C), -1, np.int32),
                "hotspot_max": np.full((G, C), np.nan, np.float32), "invalid": np.zeros((G, C), np.uint32),
                "alert_steps": np.zeros((G, 3 + L, C), np.uint32), "onset": np.full((G, L, C), -1, np.int32),
                "dhw": np.zeros((T, C), np.float32) if return_dhw else None, "alert": np.zeros((T, C), np.uint8) if return_alert else None}
    import torch

    eng = _engine(device)
    sst_w = _Windows(eng, sst, T, C, np.float32, False)
    if m is None:
        m = _climatology(p, sst, p["lab"], device, eng, sst_w)[1]
    per_step = sst_w.upload_bytes_per_step
    fixed = 12 * C + accumulator_bytes(G, C, L) + (4 * T * C if return_dhw else 0) + (T * C if return_alert else 0) + W * per_step
    B = _stream._window_steps(
        eng, "heat_stress", T, C, per_step, fixed, p["block_steps"],
        f"{C} cells of 12 bytes (carried sum, mmm), {G} x {C} cells of accumulators, {accumulator_bytes(1, 1, L)} bytes each, "
        f"{'the dhw output of ' + str(T) + ' x ' + str(C) + ' x 4 bytes, ' if return_dhw else ''}"
        f"{'the alert output of ' + str(T) + ' x ' + str(C) + ' bytes, ' if return_alert else ''}"
        f"and the field of {T} timesteps and {W} of history, 4 bytes per cell, as far as it is not on the device already",
        ["Group by fewer labels"] + (["Pass return_dhw=False"] if return_dhw else []) + (["Pass return_alert=False"] if return_alert else []))
    dhw = torch.empty((T, C), dtype=torch.float32, device=eng.device) if return_dhw else None
    alert = torch.empty((T, C), dtype=torch.uint8, device=eng.device) if return_alert else None
    kw = dict(window=W, hotspot_min=p["hmin"], steps_per_week=p["spw"], levels=lev, dhw=dhw, alert=alert)
    if p["grp"] is not None:
        kw.update(grp=p["grp"][0], G=G)

    def step(a, b, acc, finish):
        lead = min(W, a)
        return eng.heat_stress(sst_w.get(a - lead, b), m, t0=a, lead=lead, acc=acc, finish=finish, **kw)

    r = _stream.walk_windows(T, B, step)
    r.update(m=m, dhw=dhw, alert=alert)
    return r


def _heat_stress(sst, mmm, baseline, months, window, steps_per_week, hotspot_min, levels, by, return_dhw, return_alert, block_steps,
                 device):
    from .xr_compat import DataArray, Dataset

    p = _plan(sst, mmm, baseline, months, window, steps_per_week, hotspot_min, levels, by, block_steps)
    r = _device_pass(p, sst, bool(return_dhw), bool(return_alert), device)
    lev = p["levels"]
    grouped = p["grp"] is not None
    gname, gvals = (p["grp"][2], p["grp"][3]) if grouped else (None, None)
    gc = {gname: (gname, gvals)} if grouped else {}

    def space(v, mid=(), extra=None):
        """``v [G, *mid, C]`` over (group,) + mid + the spatial dims; the group axis is dropped without ``by``."""
        return _stream.space(p, v if grouped else v[0], ((gname,) if grouped else ()) + tuple(mid), {**gc, **(extra or {})})

    data = {"dhw_max": space(r["dhw_max"]), "time_of_dhw_max": space(r["tmax"]), "hotspot_max": space(r["hotspot_max"]),
            "alert_steps": space(r["alert_steps"], ("alert_class",), {"alert_class": ("alert_class", np.arange(3 + lev.size, dtype=np.int64))}),
            "invalid_steps": space(r["invalid"]), "level_onset": space(r["onset"], ("level",), {"level": ("level", lev.copy())}),
            "mmm": _stream.space(p, r["m"])}
    tc = {} if p["tv"] is None else {p["tname"]: (p["tname"], p["tv"])}
    resident = _tensor_of(sst) is not None
    for name, key in (("dhw", "dhw"), ("alert_level", "alert")):
        f = r[key]
        if f is None:
            continue
        on_device = type(f).__module__.startswith("torch")  # an empty field has a NumPy one
        f = f.reshape(p["shape"]) if on_device and resident else (f.cpu().numpy() if on_device else f).reshape(p["shape"])
        data[name] = DataArray(f, dims=(p["tname"],) + tuple(p["sdims"]), coords={**p["scoords"], **tc})
    return Dataset(data, attrs={"warmup_steps": p["window"] - 1, "window": p["window"], "steps_per_week": p["spw"],
                                "hotspot_min": p["hmin"]})


def heat_stress(sst, mmm=None, baseline=None, months=None, window=84, steps_per_week=7, hotspot_min=1.0, levels=(4.0, 8.0), by=None,
                return_dhw=False, return_alert=False, block_steps=None, device=None):
    """Accumulated heat stress of every cell: the HotSpot, the Degree Heating Week (DHW) and the bleaching alert level of
    NOAA Coral Reef Watch (Liu et al. 2014, Skirving et al. 2020), from one pass over the raw SST on the device.

    ``sst``: as in :func:`monthly_maximum_climatology`.  ``mmm``: the threshold of every cell, a float map over the cells of
    a timestep -- any climatology, e.g. Coral Reef Watch's own; None takes ``mmm`` of
    ``monthly_maximum_climatology(sst, baseline, months)``.  ``block_steps``: the results do not depend on it in any bit.

    Per step, with the float32 difference ``d = sst[t] - mmm``: the step is *valid* when both are finite and ``|d| < 1024``;
    the HotSpot ``h[t]`` is ``d`` where the step is valid and ``d >= hotspot_min``, else 0; ``dhw[t]`` is the sum of ``h``
    over the last ``window`` steps (fewer in the first ``window - 1`` steps: the attribute ``warmup_steps``), divided by
    ``steps_per_week`` in float64 and rounded to float32 -- K-weeks; NaN where ``mmm`` is not finite.  An invalid step adds
    nothing and is counted; no gap is filled.  ``window`` is an integer in 1 .. 366, ``hotspot_min`` lies in
    ``[2^-10, 1024)``: within these bounds the float64 running sum is the exact sum, in any order and under any windows.
    The alert class of a step: 255 not valid, 0 for ``d <= 0``, 1 for ``0 < d < hotspot_min``, else 2 plus the number of
    ``levels`` (0 .. 6 values, strictly increasing) that ``dhw[t]`` reaches.  With the defaults -- daily steps, twelve weeks,
    1 K, 4 and 8 K-weeks -- the classes 0 .. 4 are Coral Reef Watch's No Stress, Bleaching Watch, Bleaching Warning, Alert
    Level 1 and Alert Level 2; a step below ``hotspot_min`` is never an alert, whatever the DHW, as there.

    Returned over the spatial dimensions, with a leading group dimension under ``by`` (``"year"``, ``"season"``,
    ``"month"``, ``"dayofyear"`` or integer labels, as in :func:`marex_amd.local_intensity`): ``dhw_max`` (float32, NaN for
    a cell without ``mmm`` or a group without steps), ``time_of_dhw_max`` (int32: the first step that attains it, -1 where
    none), ``hotspot_max`` (float32: the largest ``d`` over the valid steps, negative where the cell stayed below ``mmm``;
    NaN where none), ``alert_steps`` (uint32 ``[alert_class]``: the steps per class), ``invalid_steps`` (uint32),
    ``level_onset`` (int32 ``[level]``: the first step of the group with ``dhw >= level``, -1 where none) and ``mmm``.
    ``return_dhw=True`` adds ``dhw`` (float32) and ``return_alert=True`` adds ``alert_level`` (uint8) over the field's own
    dimensions -- resident tensors when ``sst`` was resident, NumPy arrays otherwise.  ``alert_level >= 3``, as a torch or
    NumPy comparison, is a mask that :func:`marex_amd.event_occurrence`, :func:`marex_amd.regional_series`,
    :func:`marex_amd.compound_events` and the tracker take (mind that 255, not valid, passes it: use
    ``(alert_level >= 3) & (alert_level != 255)``); the annual ``dhw_max`` maps of ``by="year"`` go into
    :func:`marex_amd.cell_trends`.

    Everything is an exact integer, a float32 maximum or the rounding of an exact sum."""
    return _heat_stress(sst, mmm, baseline, months, window, steps_per_week, hotspot_min, levels, by, return_dhw, return_alert,
                        block_steps, device)
