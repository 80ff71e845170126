"""Regional series: per timestep and region, how much area is in an extreme state, how intense it is there and in which
severity category -- the time series every marine-heatwave study and every operational monitor leads with (Hobday et al.
2018, Fig. 3; the basin series of Oliver et al. 2018).

The reference leaves this to notebook code -- ``(extreme_events * cell_area).where(basin).sum(("lat", "lon"))`` per basin.
Here it is one streaming pass on the device (``marex_regional_series_u8`` / ``marex_regional_series_i32``, DESIGN.md
section 4) over the presence field, the anomalies under its present cells and the thresholds and areas under those with a
finite anomaly: per (timestep, region) the cells, the area as an exact integer sum of fixed-point cell areas, the float64 sums of
weight and weight x anomaly, the maximum and the cells and area of every severity category.  Regions are any integer map
over space -- ocean basins, large marine ecosystems, EEZs, reef polygons -- not latitude rows; the host ranks them,
derives the area table and the per-region denominators, and finishes the ``by=`` groups.
"""
from __future__ import annotations

import numpy as np

from . import _stream, calendar, occurrence as mo
from ._stream import _I32_MAX, _Windows, _check_block_steps, area_weight_table, spatial, tracker_time, weighted_mean  # noqa: F401
from .exceptions import create_data_validation_error
from .local_intensity import CATEGORIES, _device_thresholds, _threshold_layout, _thresholds_copied

MAX_REGIONS = 32767


def region_ranks(regions, mask, p: dict):
    """``(rvals, rank)`` of a region map over the spatial shape of the planned field ``p``: the distinct values ``>= 0``,
    ascending -- the ``region`` coordinate -- and the rank int32 ``[C]`` of every cell among them, -1 for a cell of no region
    (a value below 0, or a cell that ``mask`` removes).  ``regions`` None: one region 0 that holds every cell."""
    C = p["C"]
    if regions is None:
        rvals, rank = np.zeros(1, np.int64), np.zeros(C, np.int32)
    else:
        r = spatial(regions, p, "regions")
        if r.dtype.kind not in "iu":
            raise create_data_validation_error("regions must be an integer map", details=f"Found dtype {r.dtype}")
        r = r.astype(np.int64)
        rvals, inv = np.unique(r[r >= 0], return_inverse=True)
        if rvals.size > MAX_REGIONS:
            raise create_data_validation_error(f"regions holds {rvals.size} distinct regions, at most {MAX_REGIONS} are taken",
                                               details="values below 0 mean no region")
        rank = np.full(C, -1, np.int32)
        rank[r >= 0] = inv.reshape(-1).astype(np.int32)
    if mask is not None:
        m = spatial(mask, p, "mask")
        if m.dtype.kind not in "biu":
            raise create_data_validation_error("mask must be boolean or integer", details=f"Found dtype {m.dtype}")
        rank = np.where(m != 0, rank, np.int32(-1)).astype(np.int32)
    return rvals, rank


def _plan(field, regions, cell_areas, dat_anomaly, thresholds, mask, by, event_id, block_steps, time=None):
    """Everything that can be refused or derived without a device.  ``time``: the tracker's ``(time dimension, time
    coordinate, values)``; its values stand in where the fields carry no time coordinate."""
    p = {"block_steps": _check_block_steps(block_steps), **_stream.plan_field(field, "regional_series", dat_anomaly)}
    tracker_time(p, time, names=False)
    T, tv = p["T"], p["tv"]
    p["match"] = 0
    if event_id is not None:
        if p["kind"] == "m":
            raise create_data_validation_error("event_id needs an ID field, not a mask")
        k = event_id.item() if isinstance(event_id, np.generic) else event_id
        if isinstance(k, bool) or not isinstance(k, int) or k <= 0 or k > _I32_MAX:
            raise create_data_validation_error("event_id must be a positive int32 ID", details=f"got {event_id!r}")
        p["match"] = int(k)
    rvals, rank = region_ranks(regions, mask, p)  # the kernel gets the ranks, -1 for none
    R = max(int(rvals.size), 1)  # a map without a region: one that holds no cell
    if rvals.size == 0:
        rvals = np.zeros(1, np.int64)
    p.update(rvals=rvals, rank=rank, R=R)
    p["e"], p["q"], p["wf"] = _stream.area_tables(cell_areas, p)
    p["thr"] = None
    if thresholds is not None:
        if dat_anomaly is None:
            raise create_data_validation_error("thresholds need dat_anomaly",
                                               details="the categories compare the anomaly of a cell with its threshold")
        kind = _threshold_layout(thresholds, p["shape"][1:], p["sdims"] if p["labelled"] else None)
        doy = np.zeros(T, np.int32)
        if kind != "none":
            mo._calendar(tv, "thresholds by dayofyear")
            doy = (calendar._to_year_doy(tv)[1].astype(np.int32) - 1) if T else doy
        p["thr"] = (kind, doy, 1 if kind == "none" else calendar.N_DOY)
    p["grp"] = None if by is None else mo.group_labels(by, tv, T)
    p["region_cells"], p["region_q"] = _stream.region_denominators(rank, p["q"], R)
    return p


def _device_pass(p, field, dat_anomaly, thresholds, device):
    """The device pass: the result of ``HotPath.regional_series`` on the host."""
    T, C, R = p["T"], p["C"], p["R"]
    an, cats = dat_anomaly is not None, p["thr"] is not None
    if T == 0 or C == 0:
        return {"area": np.zeros((T, R), np.int64), "cnt": np.zeros((T, R, 2), np.int64),
                "sums": np.zeros((T, R, 2)) if an else None, "vmax": np.full((T, R), np.nan, np.float32) if an else None,
                "cat_cnt": np.zeros((T, R, 6), np.int64) if cats else None,
                "cat_area": np.zeros((T, R, 6), np.int64) if cats and p["q"] is not None else None}
    from .detect import get_engine

    eng = get_engine(0 if device is None else device)
    x_w = _Windows(eng, field, T, C, np.uint8 if p["kind"] == "m" else np.int32, p["kind"] == "i")
    a_w = _Windows(eng, dat_anomaly, T, C, np.float32, False) if an else None
    n_doy = p["thr"][2] if cats else 0
    thr_copy = cats and _thresholds_copied(eng, thresholds, p["thr"][0])
    tables = 4 * C + (12 * C if p["q"] is not None else 0) + (4 * T if cats else 0)
    fixed = eng.regional_slot_bytes(T, R, an, cats, p["q"] is not None) + tables + (4 * n_doy * C if thr_copy else 0)
    per_step = x_w.upload_bytes_per_step + (a_w.upload_bytes_per_step if an else 0)
    B = _stream._window_steps(
        eng, "regional_series", T, C, per_step, fixed, p["block_steps"],
        f"{T} x {R} (timestep, region) slots, the region{', area and weight' if p['q'] is not None else ''} of {C} cells, "
        f"{n_doy} x {C} float32 thresholds, and the field{' and the anomalies' if an else ''} of {T} timesteps, "
        f"{x_w.item}{' + 4' if an else ''} bytes per cell, as far as they are not on the device already", ["Take fewer regions"])
    kw = dict(reg=p["rank"], R=R, T=T, q=p["q"], wf=p["wf"] if an else None, match=p["match"])
    if cats:
        kw.update(thr=_device_thresholds(eng, thresholds, p["thr"][0], n_doy, C), doy=p["thr"][1])

    def step(a, b, acc, finish):
        return eng.regional_series(x_w.get(a, b), t0=a, anom=a_w.get(a, b) if an else None, acc=acc, finish=finish, **kw)

    return _stream.walk_windows(T, B, step)


def _regional_series(field, regions, cell_areas, dat_anomaly, thresholds, mask, by, event_id, block_steps, device, time=None):
    from .xr_compat import DataArray, Dataset

    p = _plan(field, regions, cell_areas, dat_anomaly, thresholds, mask, by, event_id, block_steps, time)
    r = _device_pass(p, field, dat_anomaly, thresholds, device)
    T, R, e, _ratio = p["T"], p["R"], p["e"], mo._ratio
    tracker_time(p, time, fitting=True)
    tname, tcoord = p["tname"], p["tcoord"] or p["tname"]
    tv = np.arange(T) if p["tv"] is None else np.asarray(p["tv"])
    an, cats, areas = r["sums"] is not None, r["cat_cnt"] is not None, p["q"] is not None
    rc = {"region": ("region", p["rvals"])}
    tc = {tcoord: (tname, tv), **rc}
    cc = {"category": ("category", np.array(CATEGORIES))}

    def to_area(S):  # exact: an integer below 2^62 scaled by a power of two (rounded once where it exceeds 2^53)
        return np.ldexp(S.astype(np.float64), -e) if areas else S.astype(np.float64)

    def series(v, extra=(), c=None):
        return DataArray(v, dims=(tname, "region") + tuple(extra), coords={**tc, **(c or {})})

    cells, S = r["cnt"][..., 0].astype(np.int64), r["area"]
    region_area = to_area(p["region_q"])
    data = {"cells": series(cells), "area": series(to_area(S)),
            "area_share": series(_ratio(to_area(S), region_area[None, :])),
            "cells_share": series(_ratio(cells, p["region_cells"][None, :])),
            "region_cells": DataArray(p["region_cells"], dims=("region",), coords=rc),
            "region_area": DataArray(region_area, dims=("region",), coords=rc)}
    if an:
        W, SA = r["sums"][..., 0], r["sums"][..., 1]
        some = cells > 0
        data["intensity_mean"] = series(weighted_mean(some, W, SA))
        data["intensity_max"] = series(r["vmax"].astype(np.float32))
        data["intensity_integral"] = series(np.where(some, SA, np.nan))
        data["invalid_cells"] = series(r["cnt"][..., 1].astype(np.int64))
    if cats:
        ccnt = r["cat_cnt"].astype(np.int64)
        carea = r["cat_area"] if areas else ccnt
        data["category_cells"] = series(ccnt, ("category",), cc)
        data["category_area"] = series(to_area(carea), ("category",), cc)
        data["category_share"] = series(_ratio(to_area(carea), region_area[None, :, None]), ("category",), cc)
    if p["grp"] is not None:
        lab, G, gname, gvals = p["grp"]
        gc = {gname: (gname, gvals), **rc}

        def grouped(v, extra=(), c=None):
            return DataArray(v, dims=(gname, "region") + tuple(extra), coords={**gc, **(c or {})})

        def add_by(v, dt):  # one element after the other in ascending time: deterministic given the slots
            o = np.zeros((G,) + v.shape[1:], dt)
            np.add.at(o, lab, v.astype(dt))
            return o

        steps = np.bincount(lab, minlength=G).astype(np.int64)
        area_steps = add_by(to_area(S), np.float64)
        data["steps_by"] = DataArray(steps, dims=(gname,), coords={gname: (gname, gvals)})
        data["cell_steps_by"] = grouped(add_by(cells, np.int64))
        data["area_steps_by"] = grouped(area_steps)
        data["share_by"] = grouped(_ratio(area_steps, steps[:, None] * region_area[None, :]))
        if an:
            vm = np.full((G, R), -np.inf, np.float64)
            has = np.zeros((G, R), bool)
            ok = ~np.isnan(r["vmax"])
            np.maximum.at(vm, lab, np.where(ok, r["vmax"].astype(np.float64), -np.inf))
            np.logical_or.at(has, lab, ok)
            data["intensity_max_by"] = grouped(np.where(has, vm, np.nan).astype(np.float32))
        if cats:
            data["category_cell_steps_by"] = grouped(add_by(ccnt, np.int64), ("category",), cc)
            data["category_area_steps_by"] = grouped(add_by(to_area(carea), np.float64), ("category",), cc)
    return Dataset(data)


def regional_series(field, regions=None, cell_areas=None, dat_anomaly=None, thresholds=None, mask=None, by=None, event_id=None,
                    block_steps=None, device=None):
    """Per timestep and region: the area in an extreme state, its share of the region, the intensity there and the severity
    categories, from one pass over the field (and the anomalies and thresholds under it) on the device.

    ``field``: ``extreme_events``, ``hobday_events`` or ``compound_events`` (bool or uint8; nonzero is present) or an integer
    ``ID_field`` (present where ``> 0``, or where it equals ``event_id``; a negative value is refused, as by the trackers),
    ``(time, y, x)`` or ``(time, cells)``, a DataArray, an array or a device tensor (then it is read in place).
    ``regions``: an integer map over the spatial shape -- ocean basins, large marine ecosystems, EEZs, reef polygons; a
    value below 0 means no region.  Its distinct values ``>= 0``, ascending, are the ``region`` coordinate (at most 32 767);
    None: one region 0 that holds every cell.  Every cell belongs to at most one region: overlapping regions are out of
    scope, and the series of a union of regions is the exact integer sum of its parts (add ``cells``, add ``area``), which
    the host can form.  ``mask``: the valid cells (the ``mask`` of the ``preprocess_data`` Dataset); a cell outside it
    belongs to no region, so it defines the denominators ``region_cells`` and ``region_area`` too.  ``cell_areas``: None
    (every cell has area 1), or finite, non-negative areas in the spatial shape or, on a grid, a ``[y]`` vector broadcast
    along x.  ``block_steps``: as in :func:`marex_amd.event_intensity`; the integer results do not depend on it at all, the
    float64 sums within the bound below.

    Returned over ``(time, region)``: ``cells`` (int64), ``area`` (float64: ``ldexp(S, -e)`` of the exact integer sum ``S``
    of the fixed-point areas ``rint(a * 2^e)`` of :func:`area_weight_table`; the cells without ``cell_areas``),
    ``area_share`` and ``cells_share`` (float64: one division by ``region_area`` / ``region_cells``, NaN for a region
    without a valid cell), and per region ``region_cells`` (int64) and ``region_area`` (float64).

    ``dat_anomaly`` (float, same shape, dimension order and time coordinate) adds ``intensity_mean`` (float64
    ``sum(w a) / sum(w)``, ``w`` the float32 ``cell_areas``; NaN where no cell counts), ``intensity_max`` (float32, NaN
    where none), ``intensity_integral`` (float64 ``sum(w a)``: anomaly x area) and ``invalid_cells`` (int64).  NaN rule:
    ``cells`` and ``area`` count the same cells -- with anomalies the present cells whose anomaly is finite, without
    anomalies all present cells.  A present cell whose anomaly is NaN or infinite is counted in ``invalid_cells`` and in
    nothing else.

    ``thresholds`` (needs ``dat_anomaly``): the ``thresholds`` of ``preprocess_data`` in any of its three layouts, as in
    :func:`marex_amd.local_intensity`, whose class rule applies.  Adds, over ``(time, region, category)`` with ``category``
    = below, moderate, strong, severe, extreme, undefined: ``category_cells`` (int64), ``category_area`` and
    ``category_share`` (float64: the area of the category over ``region_area``).

    ``by``: ``"season"``, ``"month"``, ``"year"``, ``"dayofyear"`` or an integer label per timestep, as in
    :func:`marex_amd.event_occurrence`.  Adds per ``(group, region)``: ``steps_by`` (per group), ``cell_steps_by`` (int64),
    ``area_steps_by`` (float64: the areas added in ascending time), ``share_by`` (``area_steps_by`` over steps x
    ``region_area``), ``intensity_max_by`` and ``category_cell_steps_by`` / ``category_area_steps_by``.

    Every count and every area is an exact integer on the device: equal from run to run, whatever the windows.  The two
    float64 sums behind the intensities are sums of exact products in no fixed order: bit for bit
    reproducible where the partial sums are representable, otherwise within ``2 n u sum|w a|`` of the exact sum, ``n``
    the cells of the slot and ``u = 2^-53``."""
    return _regional_series(field, regions, cell_areas, dat_anomaly, thresholds, mask, by, event_id, block_steps, device)
