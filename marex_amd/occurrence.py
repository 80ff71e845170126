"""Occurrence statistics of an event mask or a tracked ID field: how often, for how long at a stretch and at which
latitudes events are present.

The reference computes these in notebook code -- ``(ID_field > 0).mean("time")`` and ``.groupby("time.season").mean("time")``
(``03_visualise_events``; the same over ``extreme_events`` in ``01_preprocess_extremes``), ``(ID_field == id).sum("time")``
for the longest events, ``(ID_field > 0).mean("lon").resample(time="ME").mean()`` / ``.groupby("time.dayofyear").mean()``
and, on a mesh, ``groupby_bins(lat, bins).mean("ncells")``; its docs list "statistical summaries (event frequency,
duration, intensity)" as the third step of the workflow.  Here all of them come from one streaming pass over the field on
the device (``marex_occurrence_u8`` / ``marex_occurrence_i32``): integer counts per (time group, cell)
and per (time group, latitude class) and the per-cell run statistics, which the host divides in float64.  The time labels
are derived on the host from the time coordinate.
"""
from __future__ import annotations

from functools import partial

import numpy as np

from . import _stream
from ._stream import _I32_MAX, _Windows, _check_block_steps, _plan_windows
from .exceptions import ConfigurationError, create_data_validation_error
from .track import _host

SEASONS = ("DJF", "JJA", "MAM", "SON")  # xarray's (alphabetical) order of the groups of "time.season"
_SEASON_OF_MONTH = np.array([0, 0, 2, 2, 2, 1, 1, 1, 3, 3, 3, 0], np.int32)  # January .. December
_BY = ("season", "month", "year", "dayofyear")
_ZONAL_BY = ("month", "dayofyear", "year", "step")


def _calendar(tv, what: str):
    """``(year, month 1..12, dayofyear 1..366)`` of datetime64 time values."""
    tv = None if tv is None else np.asarray(tv)
    if tv is None or tv.dtype.kind != "M":
        raise create_data_validation_error(f"{what} needs a datetime time coordinate",
                                           details="pass a DataArray whose leading dimension has datetime64 values, or an "
                                                   "integer label per timestep",
                                           data_info={"time_dtype": None if tv is None else str(tv.dtype)})
    if np.isnat(tv).any():
        raise create_data_validation_error(f"{what}: the time coordinate holds NaT")
    y = tv.astype("datetime64[Y]")
    m = tv.astype("datetime64[M]")
    d = tv.astype("datetime64[D]")
    return y.astype(np.int64) + 1970, (m.astype(np.int64) % 12 + 1), (d - y.astype("datetime64[D]")).astype(np.int64) + 1


def _labels_of_array(v, T: int, what: str):
    a = np.asarray(_host(v))
    if a.ndim != 1 or a.shape[0] != T or a.dtype.kind not in "iu":
        raise create_data_validation_error(f"{what} labels must be one integer per timestep",
                                           details=f"got {a.dtype} {a.shape} for {T} timesteps")
    if a.size and int(a.min()) < 0:
        raise create_data_validation_error(f"{what} labels must not be negative", details=f"smallest label {int(a.min())}")
    n = int(a.max()) + 1 if a.size else 1
    if n > _I32_MAX:
        raise create_data_validation_error(f"{what} labels must fit int32", details=f"largest label {n - 1}")
    return a.astype(np.int32), n


def group_labels(by, tv, T: int):
    """``(labels int32 [T], G, coordinate name, coordinate values)`` of a per-cell grouping.  ``"season"``: the four groups
    DJF, JJA, MAM, SON (xarray's order; December belongs to DJF) and ``"month"``: 1..12, whether or not every group has a
    step; ``"year"`` and ``"dayofyear"``: the values present, ascending; an integer array ``[T]``: groups
    ``0 .. max``."""
    if isinstance(by, str):
        if by not in _BY:
            raise ConfigurationError(f"by must be one of {_BY} or an integer label per timestep", details=f"by={by!r}")
        year, month, doy = _calendar(tv, f"by={by!r}")
        if by == "season":
            return _SEASON_OF_MONTH[month - 1].astype(np.int32), 4, "season", np.array(SEASONS)
        if by == "month":
            return (month - 1).astype(np.int32), 12, "month", np.arange(1, 13, dtype=np.int64)
        vals, lab = np.unique(year if by == "year" else doy, return_inverse=True)
        return lab.reshape(-1).astype(np.int32), max(int(vals.size), 1), by, vals.astype(np.int64)
    lab, n = _labels_of_array(by, T, "by")
    return lab, n, "group", np.arange(n, dtype=np.int64)


def zonal_labels(zonal_by, tv, T: int):
    """The same for the section counts.  ``"month"``: one group per calendar month from the first to the last month of the
    series (what ``resample(time="ME")`` gives; the coordinate is the first day of the month); ``"step"``: one group per
    timestep; ``"year"``, ``"dayofyear"``: the values present; an integer array ``[T]``: groups ``0 .. max``."""
    if isinstance(zonal_by, str):
        if zonal_by not in _ZONAL_BY:
            raise ConfigurationError(f"zonal_by must be one of {_ZONAL_BY} or an integer label per timestep",
                                     details=f"zonal_by={zonal_by!r}")
        if zonal_by == "step":
            return np.arange(T, dtype=np.int32), max(T, 1), "zonal_step", (np.arange(T) if tv is None else np.asarray(tv))
        year, month, doy = _calendar(tv, f"zonal_by={zonal_by!r}")
        if zonal_by == "month":
            mi = (year - 1970) * 12 + (month - 1)
            lo = int(mi.min()) if mi.size else 0
            n = int(mi.max()) - lo + 1 if mi.size else 1
            if n > _I32_MAX:
                raise create_data_validation_error("zonal_by='month': the series spans too many months", details=f"{n} months")
            return (mi - lo).astype(np.int32), n, "zonal_month", (lo + np.arange(n)).astype("datetime64[M]").astype("datetime64[D]")
        vals, lab = np.unique(year if zonal_by == "year" else doy, return_inverse=True)
        return lab.reshape(-1).astype(np.int32), max(int(vals.size), 1), "zonal_" + zonal_by, vals.astype(np.int64)
    lab, n = _labels_of_array(zonal_by, T, "zonal_by")
    return lab, n, "zonal_group", np.arange(n, dtype=np.int64)


def lat_classes(lat, lat_bins, C: int):
    """``(cls int32 [C], R, edges)``: the bin of every mesh cell under the right-closed intervals of ``groupby_bins`` -- bin
    r holds ``edges[r] < lat <= edges[r + 1]``; a cell outside every bin or with a non-finite latitude gets -1."""
    if lat is None or lat_bins is None:
        raise create_data_validation_error("zonal presence on a mesh needs lat [cells] and lat_bins (ascending edges)")
    la = np.asarray(_host(lat), dtype=np.float64).reshape(-1)
    e = np.asarray(_host(lat_bins), dtype=np.float64)
    if la.shape != (C,):
        raise create_data_validation_error("lat does not match the cells of the field", details=f"lat {la.shape}, {C} cells")
    if e.ndim != 1 or e.size < 2 or not np.isfinite(e).all() or not (np.diff(e) > 0).all():
        raise create_data_validation_error("lat_bins must be at least two finite, strictly ascending edges",
                                           details=f"got {e.shape}: {e[:8].tolist()}")
    R = int(e.size) - 1
    r = np.searchsorted(e, la, side="left").astype(np.int64) - 1  # first edge >= lat, minus one; NaN sorts past the end
    r[(r < 0) | (r >= R) | ~np.isfinite(la)] = -1
    return r.astype(np.int32), R, e


def _plan(field, by, zonal, zonal_by, lat, lat_bins, event_ids, block_steps):
    """Everything that can be refused or derived without a device."""
    p = {"block_steps": _check_block_steps(block_steps), **_stream.plan_field(field, "event_occurrence")}
    T, tv = p["T"], p["tv"]
    ids = []
    if event_ids is not None:
        ids = [k for k in np.asarray(event_ids).reshape(-1).tolist()]
        if p["bool"]:
            raise create_data_validation_error("event_ids need an ID field, not a boolean mask")
        if any(isinstance(k, bool) or not isinstance(k, int) or k <= 0 or k > _I32_MAX for k in ids):
            raise create_data_validation_error("event_ids must be positive int32 IDs", details=f"got {ids[:8]}")
    p["ids"] = ids
    p["grp"] = None if by is None else group_labels(by, tv, T)
    p["sec"] = None
    if zonal:
        p["sec"] = _stream.plan_sections(p, zonal_by, lat, lat_bins)
    return p


def _counts(p, field, device):
    """The device pass: ``(cell_cnt [G, C], runs [3, C], sec_cnt or None, dur [K, C])`` on the host."""
    T, C = p["T"], p["C"]
    G = 1 if p["grp"] is None else p["grp"][1]
    K = len(p["ids"])
    if T == 0 or C == 0:
        sec = None if p["sec"] is None else np.zeros((p["sec"][0][1], p["sec"][2]), np.uint64)
        return np.zeros((G, C), np.uint32), np.zeros((3, C), np.uint32), sec, np.zeros((K, C), np.uint32)
    from .detect import get_engine

    eng = get_engine(0 if device is None else device)
    wins = _Windows(eng, field, T, C, np.uint8 if p["kind"] == "m" else np.int32, p["kind"] == "i")
    B = _plan_windows(eng, T, C, wins.upload_bytes_per_step, p["block_steps"], "event_occurrence",
                      f"the field of {T} timesteps of {C} cells, {wins.item} bytes per cell, as far as it is not on the device "
                      "already")
    kw = {}
    if p["grp"] is not None:
        kw.update(grp=p["grp"][0], G=G)
    if p["sec"] is not None:
        kw.update(sgrp=p["sec"][0][0], G2=p["sec"][0][1], cls=p["sec"][1], R=p["sec"][2])

    def step(a, b, acc, finish):
        return eng.occurrence(wins.get(a, b), t0=a, event_ids=p["ids"], acc=acc, finish=finish, **kw)

    r = _stream.walk_windows(T, B, step)
    return r["cell_cnt"], r["runs"], r["sec_cnt"], r["dur"]


def _ratio(num, den):
    with np.errstate(invalid="ignore", divide="ignore"):
        return np.where(den != 0, np.asarray(num, np.float64) / np.where(den != 0, den, 1).astype(np.float64), np.nan)


def _event_occurrence(field, by, zonal, zonal_by, lat, lat_bins, event_ids, block_steps, device):
    from .xr_compat import DataArray, Dataset

    p = _plan(field, by, zonal, zonal_by, lat, lat_bins, event_ids, block_steps)
    cell_cnt, runs, sec_cnt, dur = _counts(p, field, device)
    T, space = p["T"], partial(_stream.space, p)
    occ = cell_cnt.sum(axis=0, dtype=np.uint32) if cell_cnt.shape[0] != 1 else cell_cnt[0]
    data = {"occurrence": space(occ), "frequency": space(_ratio(occ, np.int64(T))), "n_runs": space(runs[1]),
            "longest_run": space(runs[2]), "mean_run": space(_ratio(occ, runs[1]))}
    if p["grp"] is not None:
        lab, G, gname, gvals = p["grp"]
        steps = np.bincount(lab, minlength=G).astype(np.int64)
        gc = {gname: (gname, gvals)}
        data["occurrence_by"] = space(cell_cnt, (gname,), gc)
        data["steps_by"] = DataArray(steps, dims=(gname,), coords=gc)
        data["frequency_by"] = space(_ratio(cell_cnt, steps[:, None]), (gname,), gc)
    if p["sec"] is not None:
        (lab, G2, *_), *_, ccells = p["sec"]
        steps = np.bincount(lab, minlength=G2).astype(np.int64)
        zname, cname, zc, class_cells = _stream.section_coords(p["sec"])
        data["presence_cells"] = DataArray(sec_cnt, dims=(zname, cname), coords=zc)
        data["presence"] = DataArray(_ratio(sec_cnt, steps[:, None] * ccells[None, :]), dims=(zname, cname), coords=zc)
        data["class_cells"] = class_cells
    if event_ids is not None:
        ec = {"event": ("event", np.asarray(p["ids"], np.int32))}
        data["local_duration"] = space(dur, ("event",), ec)
    return Dataset(data)


def event_occurrence(field, by=None, zonal=None, zonal_by="month", lat=None, lat_bins=None, event_ids=None, block_steps=None,
                     device=None):
    """Where and when events occur: frequency maps, run lengths, local durations and zonal presence, from one pass over
    the field on the device.

    ``field``: ``extreme_events`` (bool or uint8; nonzero is present) or an integer ``ID_field`` (present where ``> 0``; a
    negative value is refused, as by the trackers), ``(time, y, x)`` or ``(time, cells)``; a DataArray, an array or a
    device tensor, on the host or device resident (then it is read in place).  ``block_steps``: as in
    :func:`marex_amd.event_intensity` -- None takes the field whole, a number walks it in windows of that many timesteps,
    ``"auto"`` takes the largest window the free memory allows; the results do not depend on it.

    Always returned, over the spatial dimensions of the field: ``occurrence`` (uint32, timesteps present), ``frequency``
    (float64 ``occurrence / T``: ``(field > 0).mean("time")``), ``n_runs`` and ``longest_run`` (uint32: the runs of
    consecutive present timesteps and the longest of them) and ``mean_run`` (float64 ``occurrence / n_runs``, NaN where
    there is no run).

    ``by``: ``"season"`` (DJF, JJA, MAM, SON -- xarray's order; December belongs to DJF), ``"month"`` (1..12), ``"year"``,
    ``"dayofyear"`` (the values present) or an integer label per timestep (groups ``0 .. max``, dimension ``group``).  Adds
    ``occurrence_by`` (uint32 ``[G, space]``), ``steps_by`` (int64 ``[G]``) and ``frequency_by`` (float64, NaN for a group
    without steps: ``.groupby("time.season").mean("time")``) over a coordinate named after the grouping.  A grouping by
    name needs a datetime64 time coordinate (:class:`DataValidationError` otherwise).

    ``zonal``: on a grid the classes are the y rows and all ``nx`` cells of a row count, land included
    (``.mean("lon")``); on a mesh ``lat`` ``[cells]`` and ``lat_bins`` (ascending edges) give right-closed bins,
    ``edges[r] < lat <= edges[r + 1]`` (``groupby_bins``), other cells and non-finite latitudes are in no bin.
    ``zonal_by``: ``"month"`` (one group per calendar month of the series: ``resample(time="ME")``), ``"dayofyear"``,
    ``"year"``, ``"step"`` or labels.  Adds ``presence_cells`` (uint64 ``[G2, R]``), ``presence`` (float64
    ``presence_cells / (steps x cells of the class)``, NaN where that is 0) and ``class_cells`` (int64 ``[R]``).

    ``event_ids``: positive IDs; adds ``local_duration`` (uint32 ``[K, space]``, ``(field == id).sum("time")``) over
    ``event``.  One more pass over each resident window per ID; refused for a boolean field.

    Everything is an exact integer count or a single float64 division of two of them."""
    return _event_occurrence(field, by, zonal, zonal_by, lat, lat_bins, event_ids, block_steps, device)
