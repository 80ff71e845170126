"""Compound events: two presence fields joined in one pass on the device.

The reference's guide lists compound events as its one advanced feature (``docs/user_guide.rst:821-833``): two masks from
``preprocess_data`` on two variables and ``sst_extremes.extreme_events & salinity_extremes.extreme_events``; what follows --
how often the two coincide in a cell, whether that is more than chance, whether one leads the other, what share of the runs
of one came with the other -- is left to host loops.  Here one streaming pass over both fields
(``marex_compound_u8``) gives the integer counts behind all of them: per cell the steps with A, with B
and with both by time group, the run statistics of the joint mask, the pairs at every lag ``-L .. L`` and the runs of each
field that the other meets within a tolerance; per (time group, latitude class) the three counts; and the joint mask itself
when asked for.  The host divides in float64.
"""
from __future__ import annotations

from functools import partial

import numpy as np

from . import _stream
from ._stream import _Windows, _check_block_steps
from .exceptions import ConfigurationError
from .occurrence import _ratio, group_labels
from .track import _tensor_of

MAX_LAG = 30     # a field's history is one 32-bit word for the tolerance, two for the lags of a block of 32 steps
STATE_ROWS = 13  # uint32 rows a cell carries between windows (include/marex_hip.h)


def _steps(name: str, v) -> int:
    k = v.item() if isinstance(v, np.generic) else v
    if isinstance(k, bool) or not isinstance(k, int) or k < 0 or k > MAX_LAG:
        raise ConfigurationError(f"{name} must be an integer in 0 .. {MAX_LAG}", details=f"{name}={v!r}")
    return int(k)


def _events_of(f):
    """A Dataset as ``preprocess_data`` returns it is taken by its ``extreme_events``."""
    return f["extreme_events"] if hasattr(f, "data_vars") and "extreme_events" in f.data_vars else f


def accumulator_bytes(G: int, C: int, L: int) -> int:
    return 4 * (3 * int(G) + (2 * int(L) + 1 if L else 0) + STATE_ROWS) * int(C)


def _plan(field_a, field_b, max_lag, tolerance, by, zonal, zonal_by, lat, lat_bins, block_steps):
    """Everything that can be refused or derived without a device."""
    p = {"block_steps": _check_block_steps(block_steps), "L": _steps("max_lag", max_lag), "K": _steps("tolerance", tolerance),
         **_stream.plan_field(field_a, "compound_events", field_b, names=("field_a", "field_b"), presence_partner=True)}
    p["grp"] = None if by is None else group_labels(by, p["tv"], p["T"])
    p["sec"] = _stream.plan_sections(p, zonal_by, lat, lat_bins) if zonal else None
    return p


class _Presence:
    """The rows ``a .. b`` of a presence field as uint8 on the device: a mask through ``_Windows`` as it is, an ID field
    through its int32 window, the check for negative IDs and one comparison."""

    def __init__(self, eng, field, T: int, C: int, kind: str):
        self.ids = kind == "i"
        self.w = _Windows(eng, field, T, C, np.int32 if self.ids else np.uint8, self.ids)

    @property
    def upload_bytes_per_step(self) -> int:
        return self.w.upload_bytes_per_step

    def get(self, a: int, b: int):
        import torch

        x = self.w.get(a, b)
        if self.ids:
            if x.numel():
                lo = int(x.min().item())
                if lo < 0:
                    from .track import tracker

                    raise tracker._id_range_error(lo, int(x.max().item()))
            x = (x > 0).to(torch.uint8)
        return x


def _device_pass(p, field_a, field_b, return_mask, device):
    """The device pass: the result of ``HotPath.compound`` on the host, and ``mask``."""
    T, C, L, K = p["T"], p["C"], p["L"], p["K"]
    G = 1 if p["grp"] is None else p["grp"][1]
    sec = p["sec"]
    if T == 0 or C == 0:
        z = lambda *s: np.zeros(s + (C,), np.uint32)  # noqa: E731
        return {"days": z(3, G), "runs": z(3), "co": z(4), "lag_days": z(2 * L + 1) if L else None,
                "sec_cnt": None if sec is None else np.zeros((3, sec[0][1], sec[2]), np.uint64),
                "mask": np.zeros((T, C), np.uint8) if return_mask else None}
    import torch

    from .detect import get_engine

    eng = get_engine(0 if device is None else device)
    wa = _Presence(eng, field_a, T, C, p["kind"])
    wb = _Presence(eng, field_b, T, C, p["kind_b"])
    per_step = wa.upload_bytes_per_step + wb.upload_bytes_per_step
    sec_bytes = 0 if sec is None else 24 * sec[0][1] * sec[2]
    fixed = accumulator_bytes(G, C, L) + sec_bytes + (T * C if return_mask else 0)
    details = (f"{3 * G + (2 * L + 1 if L else 0) + STATE_ROWS} x {C} uint32 of counts and carried state, {sec_bytes} bytes of "
               f"section counts, {'the joint mask of ' + str(T) + ' x ' + str(C) + ' bytes, ' if return_mask else ''}and both "
               f"fields of {T} timesteps, {wa.w.item} and {wb.w.item} bytes per cell, as far as they are not on the device already")
    B = _stream._window_steps(eng, "compound_events", T, C, per_step, fixed, p["block_steps"], details,
                              ["Pass return_mask=False"] if return_mask else [])
    kw = dict(max_lag=L, tolerance=K)
    if p["grp"] is not None:
        kw.update(grp=p["grp"][0], G=G)
    if sec is not None:
        kw.update(sgrp=sec[0][0], G2=sec[0][1], cls=sec[1], R=sec[2])
    mask = torch.empty((T, C), dtype=torch.uint8, device=eng.device) if return_mask else None

    def step(a, b, acc, finish):
        return eng.compound(wa.get(a, b), wb.get(a, b), t0=a, mask=mask, acc=acc, finish=finish, **kw)

    r = _stream.walk_windows(T, B, step)
    r["mask"] = mask
    return r


def _lmf(both, n_a, n_b, steps):
    """``(both * steps) / (n_a * n_b)``: both products in int64, one float64 division, NaN where the denominator is 0."""
    return _ratio(both.astype(np.int64) * np.asarray(steps, np.int64), n_a.astype(np.int64) * n_b.astype(np.int64))


def _compound_events(field_a, field_b, max_lag, tolerance, by, zonal, zonal_by, lat, lat_bins, return_mask, block_steps, device):
    from .xr_compat import DataArray, Dataset

    field_a, field_b = _events_of(field_a), _events_of(field_b)
    p = _plan(field_a, field_b, max_lag, tolerance, by, zonal, zonal_by, lat, lat_bins, block_steps)
    r = _device_pass(p, field_a, field_b, bool(return_mask), device)
    T, L, space = p["T"], p["L"], partial(_stream.space, p)
    days = r["days"]
    n_a, n_b, both = (days[k].sum(axis=0, dtype=np.uint32) if days.shape[1] != 1 else days[k][0] for k in range(3))
    runs, co = r["runs"], r["co"]
    i64 = lambda v: v.astype(np.int64)  # noqa: E731
    data = {"days_a": space(n_a), "days_b": space(n_b), "days_both": space(both), "n_runs": space(runs[1]),
            "longest_run": space(runs[2]), "mean_run": space(_ratio(both, runs[1])), "lmf": space(_lmf(both, n_a, n_b, T)),
            "jaccard": space(_ratio(both, i64(n_a) + i64(n_b) - i64(both))),
            "runs_a": space(co[0]), "runs_a_coincident": space(co[1]), "runs_b": space(co[2]), "runs_b_coincident": space(co[3]),
            "coincidence_a": space(_ratio(co[1], co[0])), "coincidence_b": space(_ratio(co[3], co[2]))}
    if L:
        data["lag_days"] = space(r["lag_days"], ("lag",), {"lag": ("lag", np.arange(-L, L + 1, dtype=np.int64))})
    if p["grp"] is not None:
        lab, G, gname, gvals = p["grp"]
        steps = np.bincount(lab, minlength=G).astype(np.int64)
        gc = {gname: (gname, gvals)}
        data.update(days_a_by=space(days[0], (gname,), gc), days_b_by=space(days[1], (gname,), gc),
                    days_both_by=space(days[2], (gname,), gc), steps_by=DataArray(steps, dims=(gname,), coords=gc),
                    lmf_by=space(_lmf(days[2], days[0], days[1], steps[:, None]), (gname,), gc))
    if p["sec"] is not None:
        (lab, G2, *_), *_, ccells = p["sec"]
        steps = np.bincount(lab, minlength=G2).astype(np.int64)
        zname, cname, zc, class_cells = _stream.section_coords(p["sec"])
        sc = r["sec_cnt"]
        zda = lambda v: DataArray(v, dims=(zname, cname), coords=zc)  # noqa: E731
        data.update(cells_a=zda(sc[0]), cells_b=zda(sc[1]), cells_both=zda(sc[2]),
                    share_both=zda(_ratio(sc[2], steps[:, None] * ccells[None, :])), class_cells=class_cells)
    if return_mask:
        m = r["mask"]
        on_device = type(m).__module__.startswith("torch")  # an empty field has a NumPy one
        as_bool = p["bool"] and p["bool_b"]
        if on_device and _tensor_of(field_a) is not None:
            import torch

            m = (m.view(torch.bool) if as_bool else m).reshape(p["shape"])
        else:
            m = (m.cpu().numpy() if on_device else m).astype(bool if as_bool else np.uint8).reshape(p["shape"])
        tc = {} if p["tv"] is None else {p["tname"]: (p["tname"], p["tv"])}
        data["compound_events"] = DataArray(m, dims=(p["tname"],) + tuple(p["sdims"]), coords={**p["scoords"], **tc})
    return Dataset(data)


def compound_events(field_a, field_b, max_lag=0, tolerance=0, by=None, zonal=None, zonal_by="month", lat=None, lat_bins=None,
                    return_mask=False, block_steps=None, device=None):
    """Where and when two kinds of extremes occur together: joint, lagged and run-level coincidence per cell, by time
    group and by latitude class, from one pass over both fields on the device.

    ``field_a``, ``field_b``: presence fields as :func:`marex_amd.event_occurrence` takes them -- ``extreme_events`` or
    ``hobday_events`` (bool or uint8; nonzero is present) or an integer ``ID_field`` (present where ``> 0``; a negative value
    is refused, as by the trackers), ``(time, y, x)`` or ``(time, cells)``; a DataArray, an array or a device tensor, on the
    host or device resident, in any mix; a Dataset of ``preprocess_data`` is taken by its ``extreme_events``.  The two must
    agree in shape, dimension names with their order, and time coordinate (:class:`DataValidationError` otherwise, before
    any device work).  An ID field is reduced to presence bytes per window on the device, which costs one more pass over
    that window (the check for negative IDs and the comparison).  ``block_steps`` and ``device`` as in
    :func:`marex_amd.event_occurrence`; no result depends on ``block_steps`` or on which field was resident.

    A low-tail extreme (the guide's low salinity) is not ``threshold_percentile=5``: the approximate method refuses that,
    and the ``>=`` mask would not make it a low extreme.  Run ``preprocess_data`` on the negated variable at the high
    percentile and pass its ``extreme_events``.

    With ``A[t]``, ``B[t]`` the presence of a cell at step ``t = 0 .. T - 1``, always returned over the spatial dimensions
    of the fields: ``days_a``, ``days_b``, ``days_both`` (uint32: steps with A, with B, with both); ``n_runs``,
    ``longest_run`` (uint32) and ``mean_run`` (float64 ``days_both / n_runs``, NaN without a run): the run statistics of
    the joint mask as ``event_occurrence`` defines them; ``lmf`` (float64), the likelihood multiplication factor
    ``(days_both * T) / (days_a * days_b)`` -- both products in int64, one division, NaN where the denominator is 0;
    ``jaccard`` (float64 ``days_both / (days_a + days_b - days_both)``, NaN where that is 0); ``runs_a``,
    ``runs_a_coincident``, ``runs_b``, ``runs_b_coincident`` (uint32) and ``coincidence_a``, ``coincidence_b`` (float64
    ratios, NaN without a run): a run ``[s, e]`` of A (maximal, consecutive present steps) is coincident when B is present
    at some step of ``[max(0, s - tolerance), min(T - 1, e + tolerance)]``, and the same for B with the roles swapped; a run
    open at the record's end is a run, judged on what is there.

    ``max_lag = L`` in ``1 .. 30`` adds ``lag_days`` (uint32 ``[lag, space]``, ``lag = -L .. L``):
    ``lag_days[l] = #{t : A[t] and B[t + l]}`` with both steps inside the record -- a positive lag means B follows A, and
    ``lag_days[0]`` equals ``days_both``.  ``tolerance``: ``0 .. 30``.  Anything else for either raises
    :class:`ConfigurationError`.

    ``by`` as in ``event_occurrence``: adds ``days_a_by``, ``days_b_by``, ``days_both_by`` (uint32 ``[G, space]``),
    ``steps_by`` (int64 ``[G]``) and ``lmf_by`` (``steps_by`` in the place of ``T``).  Lags and run coincidence are not
    grouped.  ``zonal=True`` with ``zonal_by``, ``lat``, ``lat_bins`` as in ``event_occurrence`` (the same classes and
    periods; on a grid land cells count in the denominator): adds ``cells_a``, ``cells_b``, ``cells_both`` (uint64
    ``[G2, R]``), ``share_both`` (float64 ``cells_both / (steps x cells of the class)``, NaN where that is 0) and
    ``class_cells`` (int64 ``[R]``).

    ``return_mask=True`` adds ``compound_events`` over the fields' own dimensions: the joint mask ``A and B`` (the
    simultaneous one, whatever ``max_lag`` and ``tolerance``), bool where both inputs were bool and uint8 otherwise, a
    device tensor when ``field_a`` was resident and a NumPy array otherwise; ``tracker``, ``cell_events``,
    ``event_occurrence`` and ``local_intensity`` take it as their field.  It takes one byte per cell of the whole record on
    the device (:class:`TrackingError` with the figures when the call does not fit).

    Everything is an exact integer count or a single float64 division of two exact integers."""
    return _compound_events(field_a, field_b, max_lag, tolerance, by, zonal, zonal_by, lat, lat_bins, return_mask, block_steps,
                            device)
