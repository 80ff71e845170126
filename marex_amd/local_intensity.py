"""Per-cell intensity of extremes and their severity categories: how hot, for how many degree-days and when a grid cell
was while it was in an extreme.

The reference leaves this to notebook code -- ``dat_anomaly.where(extreme_events)`` with ``.groupby("time.year")`` and
``sum`` / ``mean`` / ``max`` / ``idxmax``; its docs list "statistical summaries (event frequency, duration, intensity)" as
the third step of the workflow -- and the severity categories of Hobday et al. (2018), Moderate / Strong / Severe /
Extreme as multiples of the threshold, need the anomalies, the thresholds and the mask side by side, which
``preprocess_data`` leaves in device memory.  Here all of it comes from one streaming pass on the device
(``marex_local_intensity_u8`` / ``marex_local_intensity_i32``): per (time group, cell) the days, the
sequential float64 sum, the maximum and its step and the days per category, and per (time group, latitude class,
category) the classified cells.  The time labels, the day of year of every step and the latitude classes are derived on the
host.
"""
from __future__ import annotations

import numpy as np

from . import _stream, calendar, occurrence as mo
from ._stream import _I32_MAX, _Windows, _check_block_steps, _dtype_name, _kind
from .exceptions import create_data_validation_error
from .track import _tensor_of

CATEGORIES = ("below", "moderate", "strong", "severe", "extreme", "undefined")


def accumulator_bytes(G: int, C: int, categories: bool) -> int:
    """The per-cell accumulators of the device pass: days, invalid, maximum and its step (4 bytes each), the float64 sum,
    and six uint32 category counts with thresholds."""
    return int(G) * int(C) * (24 + (24 if categories else 0))


def _threshold_layout(thresholds, sp, sdims):
    """``(kind, n_doy)``, kind one of ``"doy_last"``, ``"doy_first"``, ``"none"``: by the dimension names where the
    thresholds carry them, by the shape otherwise."""
    shape = tuple(int(k) for k in thresholds.shape)
    dims = tuple(getattr(thresholds, "dims", ()) or ())
    if _kind(thresholds) != "f":
        raise create_data_validation_error("thresholds must be a floating-point field",
                                           details=f"Found dtype {_dtype_name(thresholds)}",
                                           data_info={"actual_dtype": _dtype_name(thresholds)})
    kind = None
    if dims:
        rest = tuple(d for d in dims if d != "dayofyear")
        if sdims is not None and rest != tuple(sdims):
            raise create_data_validation_error("field and thresholds differ in their dimensions",
                                               details=f"a timestep of the field {tuple(sdims)}, thresholds {dims}; the order "
                                                       "must agree too")
        if "dayofyear" not in dims:
            kind = "none"
        elif dims[-1] == "dayofyear":
            kind = "doy_last"
        elif dims[0] == "dayofyear":
            kind = "doy_first"
    elif shape == sp:
        kind = "none"
    elif shape[:-1] == sp and shape[-1] == calendar.N_DOY:
        kind = "doy_last"
    elif shape[1:] == sp and shape[0] == calendar.N_DOY:
        kind = "doy_first"
    want = {"none": sp, "doy_last": sp + (calendar.N_DOY,), "doy_first": (calendar.N_DOY,) + sp}.get(kind)
    if want is None or shape != want:
        raise create_data_validation_error("thresholds do not match the spatial shape of the field",
                                           details=f"thresholds {shape}, a timestep {sp}: expected (*space, dayofyear), "
                                                   f"(dayofyear, *space) with {calendar.N_DOY} days of the year, or (*space)")
    return kind


def _plan(field, dat_anomaly, thresholds, by, zonal, zonal_by, lat, lat_bins, event_id, block_steps):
    """Everything that can be refused or derived without a device."""
    p = {"block_steps": _check_block_steps(block_steps), **_stream.plan_field(field, "local_intensity", dat_anomaly)}
    shape, T, tv = p["shape"], p["T"], p["tv"]
    p["match"] = 0
    if event_id is not None:
        if p["bool"]:
            raise create_data_validation_error("event_id needs an ID field, not a boolean mask")
        k = event_id.item() if isinstance(event_id, np.generic) else event_id
        if isinstance(k, bool) or not isinstance(k, int) or k <= 0 or k > _I32_MAX:
            raise create_data_validation_error("event_id must be a positive int32 ID", details=f"got {event_id!r}")
        p["match"] = int(k)
    p["thr"] = None
    if thresholds is not None:
        kind = _threshold_layout(thresholds, shape[1:], p["sdims"] if p["labelled"] else None)
        doy = np.zeros(T, np.int32)
        if kind != "none":
            mo._calendar(tv, "thresholds by dayofyear")
            doy = (calendar._to_year_doy(tv)[1].astype(np.int32) - 1) if T else doy  # the row preprocess_data compares with
        p["thr"] = (kind, doy, 1 if kind == "none" else calendar.N_DOY)
    elif zonal:
        raise create_data_validation_error("zonal category counts need thresholds",
                                           details="zonal=True counts the cells of every category per latitude class")
    p["grp"] = None if by is None else mo.group_labels(by, tv, T)
    p["sec"] = None
    if zonal:
        p["sec"] = _stream.plan_sections(p, zonal_by, lat, lat_bins)
    return p


def _device_thresholds(eng, thresholds, kind: str, n_doy: int, C: int):
    """The thresholds as a contiguous float32 ``[n_doy, C]`` tensor on the engine's device (a float64 ``global_extreme``
    threshold is rounded to float32 here)."""
    import torch

    t = _tensor_of(thresholds)
    if t is None:
        t = torch.from_numpy(np.ascontiguousarray(thresholds.values if hasattr(thresholds, "values") else thresholds))
    t = t.to(eng.device)
    if kind == "doy_last":
        t = t.reshape(C, n_doy).t()
    return t.reshape(n_doy, C).to(torch.float32).contiguous()


def _thresholds_copied(eng, thresholds, kind: str) -> bool:
    """Whether :func:`_device_thresholds` makes a copy: not of a contiguous float32 tensor on the engine's device whose
    layout needs no transpose, which is resident as it is."""
    t = _tensor_of(thresholds)
    return not (t is not None and t.device == eng.device and kind != "doy_last" and "float32" in str(t.dtype)
                and t.is_contiguous())


def _device_pass(p, field, dat_anomaly, thresholds, device):
    """The device pass: the result of ``HotPath.local_intensity`` on the host."""
    T, C = p["T"], p["C"]
    G = 1 if p["grp"] is None else p["grp"][1]
    cats, sec = p["thr"] is not None, p["sec"]
    if T == 0 or C == 0:
        return {"days": np.zeros((G, C), np.uint32), "invalid": np.zeros((G, C), np.uint32), "sum": np.zeros((G, C)),
                "vmax": np.full((G, C), np.nan, np.float32), "tmax": np.full((G, C), -1, np.int32),
                "cat_days": np.zeros((G, 6, C), np.uint32) if cats else None,
                "sec_cnt": None if sec is None else np.zeros((sec[0][1], sec[2], 6), np.uint64)}
    from .detect import get_engine

    eng = get_engine(0 if device is None else device)
    x_w = _Windows(eng, field, T, C, np.uint8 if p["kind"] == "m" else np.int32, p["kind"] == "i")
    a_w = _Windows(eng, dat_anomaly, T, C, np.float32, False)
    n_doy = p["thr"][2] if cats else 0
    thr_copy = cats and _thresholds_copied(eng, thresholds, p["thr"][0])
    fixed = accumulator_bytes(G, C, cats) + (4 * n_doy * C if thr_copy else 0) + \
        (48 * sec[0][1] * sec[2] if sec is not None else 0)
    per_step = x_w.upload_bytes_per_step + a_w.upload_bytes_per_step
    B = _stream._window_steps(
        eng, "local_intensity", T, C, per_step, fixed, p["block_steps"],
        f"{G} x {C} cells of accumulators, {24 + (24 if cats else 0)} bytes each, {n_doy} x {C} float32 thresholds, "
        f"and the field and the anomalies of {T} timesteps, {x_w.item} + 4 bytes per cell, as far as they are not "
        "on the device already", ["Group by fewer labels"])
    kw = {"match": p["match"]}
    if p["grp"] is not None:
        kw.update(grp=p["grp"][0], G=G)
    if cats:
        kw.update(thr=_device_thresholds(eng, thresholds, p["thr"][0], n_doy, C), doy=p["thr"][1])
    if sec is not None:
        kw.update(sgrp=sec[0][0], G2=sec[0][1], cls=sec[1], R=sec[2])

    def step(a, b, acc, finish):
        return eng.local_intensity(x_w.get(a, b), a_w.get(a, b), t0=a, acc=acc, finish=finish, **kw)

    return _stream.walk_windows(T, B, step)


def _time_of_max(tv, T: int, tmax, has):
    """The time coordinate's value at ``tmax``; NaT (dates) or -1 where there is no maximum."""
    tv = np.arange(T) if tv is None else np.asarray(tv)
    dates = tv.dtype.kind in "mM"
    none = np.array("NaT", dtype=tv.dtype) if dates else np.array(-1, dtype=tv.dtype if tv.dtype.kind in "if" else np.int64)
    if T == 0:
        return np.full(tmax.shape, none)
    return np.where(has, tv[np.where(has, tmax, 0)], none)


def _local_intensity(field, dat_anomaly, thresholds, by, zonal, zonal_by, lat, lat_bins, event_id, block_steps, device):
    from .xr_compat import DataArray, Dataset

    p = _plan(field, dat_anomaly, thresholds, by, zonal, zonal_by, lat, lat_bins, event_id, block_steps)
    r = _device_pass(p, field, dat_anomaly, thresholds, device)
    T, _ratio = p["T"], mo._ratio
    grouped = p["grp"] is not None
    gname, gvals = (p["grp"][2], p["grp"][3]) if grouped else (None, None)
    gc = {gname: (gname, gvals)} if grouped else {}

    def space(v, mid=(), extra=None):
        """``v [G, *mid, C]`` over (group,) + mid + the spatial dims; the group axis is dropped without ``by``."""
        return _stream.space(p, v if grouped else v[0], ((gname,) if grouped else ()) + tuple(mid), {**gc, **(extra or {})})

    days = r["days"]
    has = ~np.isnan(r["vmax"])
    data = {"days": space(days), "invalid_steps": space(r["invalid"]), "intensity_cumulative": space(r["sum"]),
            "intensity_mean": space(_ratio(r["sum"], days)), "intensity_max": space(r["vmax"]),
            "time_of_max": space(_time_of_max(p["tv"], T, r["tmax"], has))}
    if grouped:
        data["steps_by"] = DataArray(np.bincount(p["grp"][0], minlength=p["grp"][1]).astype(np.int64), dims=(gname,), coords=gc)
    else:
        data["steps_by"] = DataArray(np.asarray(np.int64(T)), dims=())
    if p["thr"] is not None:
        cat = r["cat_days"]
        cc = {"category": ("category", np.array(CATEGORIES))}
        data["category_days"] = space(cat, ("category",), cc)
        peak = np.zeros(days.shape, np.uint8)
        for k in (1, 2, 3, 4):
            peak[cat[:, k] > 0] = k
        data["category_peak"] = space(peak)
    if p["sec"] is not None:
        zname, cname, zc, class_cells = _stream.section_coords(p["sec"], {"category": ("category", np.array(CATEGORIES))})
        sec = r["sec_cnt"]
        per_cat = sec.sum(axis=1, dtype=np.uint64)
        data["category_cells"] = DataArray(sec, dims=(zname, cname, "category"), coords=zc)
        data["category_share"] = DataArray(_ratio(per_cat, per_cat.sum(axis=1, dtype=np.uint64)[:, None]), dims=(zname, "category"),
                                           coords={k: zc[k] for k in (zname, "category")})
        data["class_cells"] = class_cells
    return Dataset(data)


def local_intensity(field, dat_anomaly, thresholds=None, by=None, zonal=None, zonal_by="month", lat=None, lat_bins=None,
                    event_id=None, block_steps=None, device=None):
    """How intense the extremes of every cell were: days, cumulative, mean and maximum intensity, the date of the peak and
    the days per severity category, from one pass over the presence field, the anomalies and the thresholds on the device.

    ``field``: ``extreme_events`` (bool or uint8; nonzero is present) or an integer ``ID_field`` (present where ``> 0``, or
    where it equals ``event_id``; a negative value is refused, as by the trackers), ``(time, y, x)`` or ``(time, cells)``.
    ``dat_anomaly``: the anomalies, float32 (other float types are cast), same shape, dimension order and time coordinate.
    Either may be a DataArray, an array or a device tensor, on the host or device resident (then it is read in place).
    ``block_steps``: as in :func:`marex_amd.event_intensity`; the results do not depend on it, not even in the last bit.

    Always returned, over the spatial dimensions of the field: ``days`` (uint32, present steps with a finite anomaly),
    ``invalid_steps`` (uint32, present steps whose anomaly is NaN or infinite: they count for nothing else),
    ``intensity_cumulative`` (float64: anomaly x timesteps, degree-days on a daily axis -- the float64 sum of the float32
    anomalies one step after the other in ascending time, the bits of a row-by-row NumPy loop), ``intensity_mean`` (float64
    ``cumulative / days``, NaN where ``days == 0``), ``intensity_max`` (float32, NaN where none), ``time_of_max`` (the time
    coordinate's value at the earliest step that attains the maximum; NaT, or -1 on a non-datetime axis, where none) and
    ``steps_by`` (int64, the timesteps).

    ``by``: ``"season"``, ``"month"``, ``"year"``, ``"dayofyear"`` or an integer label per timestep, as in
    :func:`marex_amd.event_occurrence`: every variable above gets a leading dimension named after the grouping
    (``by="year"``: annual maps), ``steps_by`` the steps of every group.

    ``thresholds``: the ``thresholds`` of ``preprocess_data`` in any of its layouts -- ``(*space, dayofyear)``,
    ``(dayofyear, *space)`` (both need a datetime64 time coordinate: a step is compared with the threshold of its day of
    the year, as ``preprocess_data`` does) or ``(*space)`` alone (``global_extreme``; float64 is rounded to float32) --
    recognised by its dimension names when it has them, by its shape otherwise.  Adds ``category_days`` (uint32
    ``[group, category, space]`` over ``category`` = below, moderate, strong, severe, extreme, undefined) and
    ``category_peak`` (uint8: the highest of 1..4 with a day, else 0).  With the threshold ``h`` of the step and the
    float32 products ``2 h``, ``3 h``, ``4 h`` a day counted in ``days`` is *below* for ``a < h`` (present under the
    threshold: a gap-filled day of a tracked event), *moderate* for ``h <= a < 2 h``, *strong* up to ``3 h``, *severe* up to
    ``4 h``, *extreme* from ``4 h``, and *undefined* where ``h`` is NaN, infinite or not positive.

    ``zonal`` (needs thresholds): classes and ``zonal_by`` as in :func:`marex_amd.event_occurrence` (grid rows, or
    ``lat`` / ``lat_bins`` on a mesh).  Adds ``category_cells`` (uint64 ``[zonal group, class, category]``, the classified
    cells), ``category_share`` (float64 ``[zonal group, category]``: the counts summed over the classes, divided by the
    classified cells of the zonal group, NaN for none) and ``class_cells`` (int64 ``[class]``).

    Everything is an exact integer, a float32 maximum or a float64 sum in one fixed order."""
    return _local_intensity(field, dat_anomaly, thresholds, by, zonal, zonal_by, lat, lat_bins, event_id, block_steps, device)
