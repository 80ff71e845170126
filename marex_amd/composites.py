"""Lagged composites of a field around event onsets and ends (superposed-epoch analysis), on the device.

What did another variable -- air-sea heat flux, wind stress, sea-level pressure, mixed-layer depth, or the SST anomaly
itself -- do before, during and after the events of a cell?  The driver studies that follow Hobday et al. (2016, 2018)
all compute it; the reference leaves it to host loops over cells.  Here one sparse pass (``marex_event_composites_u8``,
DESIGN.md section 4) streams the presence field once, finds every cell's anchors and, per anchor, adds the ``2 L + 1``
values around it into float64 accumulators per (time group, cell, lag): count, sum and sum of squares, in ascending anchor
step.  The host derives mean, standard deviation and t statistic from them in float64.
"""
from __future__ import annotations

from functools import partial

import numpy as np

from . import _stream
from ._stream import _Windows, _check_block_steps
from .compound import MAX_LAG, _events_of, _Presence, _steps
from .exceptions import ConfigurationError
from .occurrence import group_labels

ANCHORS = ("onset", "end")


def accumulator_bytes(G: int, C: int, L: int) -> int:
    return int(G) * int(C) * (4 + 20 * (2 * int(L) + 1))


def _plan(field, values, max_lag, anchor, by, block_steps):
    """Everything that can be refused or derived without a device."""
    p = {"block_steps": _check_block_steps(block_steps), "L": _steps("max_lag", max_lag)}
    if not isinstance(anchor, str) or anchor not in ANCHORS:
        raise ConfigurationError(f"anchor must be one of {ANCHORS}", details=f"anchor={anchor!r}")
    p["anchor"] = anchor
    p.update(_stream.plan_field(field, "event_composites", partner=values, names=("field", "values")))
    p["grp"] = None if by is None else group_labels(by, p["tv"], p["T"])
    return p


def _device_pass(p, field, values, device):
    """The device pass: ``anchors`` uint32 ``[G, C]``, ``count`` uint32, ``sum`` and ``sumsq`` float64 ``[G, 2 L + 1, C]``."""
    T, C, L = p["T"], p["C"], p["L"]
    G = 1 if p["grp"] is None else p["grp"][1]
    W = 2 * L + 1
    if T == 0 or C == 0:
        return {"anchors": np.zeros((G, C), np.uint32), "count": np.zeros((G, W, C), np.uint32),
                "sum": np.zeros((G, W, C), np.float64), "sumsq": np.zeros((G, W, C), np.float64)}
    from .detect import get_engine

    eng = get_engine(0 if device is None else device)
    wx = _Presence(eng, field, T, C, p["kind"])
    wv = _Windows(eng, values, T, C, np.float32, False)
    per_step = wx.upload_bytes_per_step + wv.upload_bytes_per_step
    fixed = accumulator_bytes(G, C, L)
    details = (f"{G} x {C} cells of 4 + 20 x {W} bytes of accumulators (anchors; count, sum and sum of squares of {W} lags), and "
               f"both fields of {T} timesteps, {wx.w.item} and {wv.item} bytes per cell, as far as they are not on the device "
               "already")
    B = _stream._window_steps(eng, "event_composites", T, C, per_step, fixed, p["block_steps"], details,
                              ["Pass a smaller max_lag", "Pass by=None"] if G > 1 else ["Pass a smaller max_lag"])
    H = max(L, 1)
    kw = dict(max_lag=L, anchor=p["anchor"])
    if p["grp"] is not None:
        kw.update(grp=p["grp"][0], G=G)

    def step(a, b, acc, finish):
        lo, hi = max(0, a - H), min(T, b + H)  # the halo stands in the place of a carried state
        return eng.event_composites(wx.get(lo, hi), wv.get(lo, hi), lo, a, b, T, acc=acc, finish=finish, **kw)

    return _stream.walk_windows(T, B, step)


def derived(count, total, sumsq):
    """``(mean, std, t)`` of the accumulators, float64 expressions of NumPy on the host (the docstring of
    :func:`event_composites` spells them out)."""
    n = count.astype(np.float64)
    with np.errstate(divide="ignore", invalid="ignore"):
        mean = np.where(count > 0, total / n, np.nan)
        std = np.where(count >= 2, np.sqrt(np.maximum(0.0, (sumsq - total * total / n) / (n - 1.0))), np.nan)
        t = np.where((count >= 2) & (std != 0), mean / (std / np.sqrt(n)), np.nan)
    return mean, std, t


def _event_composites(field, values, max_lag, anchor, by, block_steps, device):
    from .xr_compat import DataArray, Dataset

    field = _events_of(field)
    p = _plan(field, values, max_lag, anchor, by, block_steps)
    r = _device_pass(p, field, values, device)
    L, space = p["L"], partial(_stream.space, p)
    lc = {"lag": ("lag", np.arange(-L, L + 1, dtype=np.int64))}
    anchors, count, total, sumsq = r["anchors"], r["count"], r["sum"], r["sumsq"]
    if p["grp"] is None:
        mean, std, t = derived(count[0], total[0], sumsq[0])
        lag = lambda v: space(v, ("lag",), lc)  # noqa: E731
        return Dataset({"anchors": space(anchors[0]), "composite_count": lag(count[0]), "composite_sum": lag(total[0]),
                        "composite_sumsq": lag(sumsq[0]), "composite_mean": lag(mean), "composite_std": lag(std),
                        "composite_t": lag(t)})
    lab, G, gname, gvals = p["grp"]
    gc = {gname: (gname, gvals)}
    mean, std, t = derived(count, total, sumsq)
    lag = lambda v: space(v, (gname, "lag"), {**gc, **lc})  # noqa: E731
    return Dataset({"anchors": space(anchors.sum(axis=0, dtype=np.uint32)), "anchors_by": space(anchors, (gname,), gc),
                    "composite_count_by": lag(count), "composite_sum_by": lag(total), "composite_sumsq_by": lag(sumsq),
                    "composite_mean_by": lag(mean), "composite_std_by": lag(std), "composite_t_by": lag(t),
                    "steps_by": DataArray(np.bincount(lab, minlength=G).astype(np.int64), dims=(gname,), coords=gc)})


def event_composites(field, values, max_lag=10, anchor="onset", by=None, block_steps=None, device=None):
    """Lagged composites (superposed-epoch analysis) of ``values`` around the onsets or the ends of the events of every
    cell: what another variable did before, during and after the events, from one sparse pass on the device.

    ``field``: a presence field as :func:`marex_amd.compound_events` takes it -- ``extreme_events``, ``hobday_events`` or
    ``compound_events`` (bool or uint8; nonzero is present) or an integer ``ID_field`` (present where ``> 0``; a negative
    value is refused, as by the trackers), ``(time, y, x)`` or ``(time, cells)``; a DataArray, an array or a device tensor,
    on the host or device resident; a Dataset of ``preprocess_data`` is taken by its ``extreme_events``.  An event of a cell
    is a maximal run of consecutive present steps.  The Hobday duration and gap rule is not re-implemented here: pass
    ``cell_events(..., return_mask=True)["hobday_events"]`` for events of a minimum duration with short gaps joined.  In an
    ID field two different IDs on adjacent steps of a cell form one run.

    ``values``: a floating-point field of the same shape, dimension names with their order, and time coordinate
    (:class:`DataValidationError` otherwise, before any device work), on the host or resident; it is read as float32 on
    the device.  A value that is NaN or +-inf is missing.

    ``anchor``: ``"onset"`` -- the steps ``s > 0`` with ``x[s]`` and not ``x[s - 1]`` -- or ``"end"`` -- the steps
    ``e < T - 1`` with ``x[e]`` and not ``x[e + 1]``.  A run that touches step 0 has no onset anchor and a run that touches
    step ``T - 1`` no end anchor: its true date is unknown, so it is censored, not guessed.  ``max_lag = L``: an integer in
    ``0 .. 30``; with ``L = 0`` only the anchor step is used.  Anything else for either raises
    :class:`ConfigurationError`.  ``block_steps`` and ``device`` as in :func:`marex_amd.event_occurrence`; no result
    depends on ``block_steps`` or on which field was resident (:class:`TrackingError` with the figures when the call does
    not fit: the accumulators take ``G x cells x (4 + 20 (2 L + 1))`` bytes).

    Returned over the spatial dimensions of the field, with the coordinate ``lag`` (int64 ``-L .. L``; a negative lag is
    before the anchor): ``anchors`` (uint32 ``[space]``: the anchors used); ``composite_count`` (uint32 ``[lag, space]``:
    the anchors ``t`` whose step ``t + lag`` lies inside ``0 .. T - 1`` and whose value there is finite),
    ``composite_sum`` and ``composite_sumsq`` (float64 ``[lag, space]``: the sum of those values and of their squares, each
    value converted to float64 and the terms added in ascending anchor step, so that the bits are those of the plain loop);
    and three float64 expressions of NumPy on them, with ``n = composite_count`` as float64:
    ``composite_mean = composite_sum / n``, NaN where ``n == 0``;
    ``composite_std = sqrt(max(0, (composite_sumsq - composite_sum * composite_sum / n) / (n - 1)))``, NaN where ``n < 2``;
    ``composite_t = composite_mean / (composite_std / sqrt(n))``, NaN where ``n < 2`` or ``composite_std == 0``.
    Count, sum and sum of squares are returned so that cells can be pooled into regions exactly.

    ``by`` as in ``event_occurrence`` (an anchor belongs to the group of its own step, whatever the steps of its lags):
    the result then holds ``anchors_by`` (uint32 ``[G, space]``), the six composite variables with the suffix ``_by`` over
    ``(group, lag, space)``, ``steps_by`` (int64 ``[G]``) and the plain ``anchors`` as the integer sum over the groups;
    the plain float variables are not returned, because summing the groups would change their bits.

    Out of scope: regional pooling inside the call (pool ``composite_count``, ``composite_sum`` and ``composite_sumsq``
    on the host), an anchor at the event's peak, and the unconditional mean of ``values`` -- pass anomalies."""
    return _event_composites(field, values, max_lag, anchor, by, block_steps, device)
