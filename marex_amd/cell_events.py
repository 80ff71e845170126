"""Per-cell marine-heatwave events under the definition the literature counts with (Hobday et al. 2016): at a cell an event
is a run of at least ``min_duration`` consecutive extreme days, and two such runs at most ``max_gap`` days apart are one
event, gap days included.

The reference's mask is that of the single extreme days; neither it nor ``event_occurrence`` / ``local_intensity`` applies
the duration and gap rule per cell.  Here one streaming pass over the mask (and the anomalies) on the device
(``marex_cell_events_u8``) walks every cell through a small state machine and gives the per-cell event
statistics, the filtered mask -- which, fed to ``local_intensity``, ``event_occurrence`` or ``tracker``, gives all their
outputs under this definition -- and, from a second pass, one record per event.  Labels, offsets and the rates of onset and
decline are derived around it.
"""
from __future__ import annotations

import numpy as np

from . import _stream, occurrence as mo
from ._stream import _I32_MAX, _Windows, _check_block_steps
from .exceptions import ConfigurationError, create_data_validation_error
from .track import _tensor_of


def state_bytes(C: int, anomalies: bool) -> int:
    """The carried state of the device pass: four int32 planes, with anomalies ten and two float64 planes."""
    return int(C) * (56 if anomalies else 16)


def accumulator_bytes(G: int, C: int, anomalies: bool) -> int:
    """The per-cell accumulators: events, event days, longest duration (4 bytes each), with anomalies the float64 sum, the
    maximum and the invalid steps."""
    return int(G) * int(C) * (28 if anomalies else 12)


def _small_int(name: str, v, lo: int) -> int:
    k = v.item() if isinstance(v, np.generic) else v
    if isinstance(k, bool) or not isinstance(k, int) or k < lo or k > _I32_MAX:
        raise ConfigurationError(f"{name} must be an integer of at least {lo} that fits int32", details=f"{name}={v!r}")
    return int(k)


def _plan(field, dat_anomaly, min_duration, max_gap, by, block_steps):
    """Everything that can be refused or derived without a device."""
    p = {"block_steps": _check_block_steps(block_steps), "D": _small_int("min_duration", min_duration, 1),
         "gap": _small_int("max_gap", max_gap, 0), **_stream.plan_field(field, "cell_events", dat_anomaly)}
    if p["kind"] != "m":
        name = _stream._dtype_name(field)
        raise create_data_validation_error("field must be an extreme_events mask (bool or uint8)", details=f"Found dtype {name}",
                                           data_info={"actual_dtype": name})
    p["grp"] = None if by is None else mo.group_labels(by, p["tv"], p["T"])
    return p


def _empty(p, G, anomalies, return_mask, records):
    C = p["C"]
    z = lambda dt: np.zeros((G, C), dt)  # noqa: E731
    r = {"events": z(np.uint32), "event_days": z(np.uint32), "duration_max": z(np.uint32), "mask": None, "rec": None}
    if anomalies:
        r.update(sum=z(np.float64), vmax=np.full((G, C), np.nan, np.float32), invalid=z(np.uint32))
    if return_mask:
        r["mask"] = np.zeros((p["T"], C), bool)
    if records:
        e = lambda dt: np.zeros(0, dt)  # noqa: E731
        r["rec"] = {"off": np.zeros(C + 1, np.int64), "start": e(np.int32), "end": e(np.int32)}
        if anomalies:
            r["rec"].update(vmax=e(np.float32), tmax=e(np.int32), sum=e(np.float64), invalid=e(np.uint32), edge=[e(np.float32)] * 4)
    return r


def _gather(w: _Windows, t, c):
    """The float32 anomalies at the steps ``t`` of the cells ``c``: torch on a resident field, NumPy on a host one."""
    if w.dev is not None:
        import torch

        C = int(w.dev.shape[1])
        idx = torch.from_numpy(t.astype(np.int64) * C + c).to(w.dev.device)
        return w.dev.reshape(-1)[idx].to(torch.float32).cpu().numpy()
    return np.asarray(w.host[t, c]).astype(np.float32)


def _device_pass(p, field, dat_anomaly, return_mask, records, device):
    """Both device passes: the result of ``HotPath.cell_events`` on the host, ``mask`` and ``rec``."""
    T, C, D, gap = p["T"], p["C"], p["D"], p["gap"]
    G = 1 if p["grp"] is None else p["grp"][1]
    anomalies = dat_anomaly is not None
    if T == 0 or C == 0:
        return _empty(p, G, anomalies, return_mask, records)
    import torch

    from .detect import get_engine

    eng = get_engine(0 if device is None else device)
    x_w = _Windows(eng, field, T, C, np.uint8, False)
    a_w = _Windows(eng, dat_anomaly, T, C, np.float32, False) if anomalies else None
    per_step = x_w.upload_bytes_per_step + (a_w.upload_bytes_per_step if anomalies else 0)
    fixed = state_bytes(C, anomalies) + accumulator_bytes(G, C, anomalies) + (T * C if return_mask else 0)
    details = (f"{C} cells of state and {G} x {C} cells of accumulators, {state_bytes(1, anomalies)} and "
               f"{accumulator_bytes(1, 1, anomalies)} bytes each, {'the mask of ' + str(T) + ' x ' + str(C) + ' bytes, ' if return_mask else ''}"
               f"and the field{' and the anomalies' if anomalies else ''} of {T} timesteps, 1{' + 4' if anomalies else ''} bytes "
               "per cell, as far as they are not on the device already")
    B = _stream._window_steps(eng, "cell_events", T, C, per_step, fixed, p["block_steps"], details,
                              ["Group by fewer labels"] + (["Pass return_mask=False"] if return_mask else []))
    kw = dict(min_duration=D, max_gap=gap)
    if p["grp"] is not None:
        kw.update(grp=p["grp"][0], G=G)
    mask = torch.empty((T, C), dtype=torch.uint8, device=eng.device) if return_mask else None

    def window(a, b):
        return (x_w.get(a, b), a_w.get(a, b) if anomalies else None)

    def step(a, b, acc, finish):
        return eng.cell_events(*window(a, b), t0=a, mask=mask, acc=acc, finish=finish, **kw)

    r = _stream.walk_windows(T, B, step)
    r["mask"], r["rec"] = mask, None
    if records:
        rec = eng.cell_event_records(r["acc"])  # the offsets from the counts of the first pass; checks the record memory

        def step2(a, b, acc, finish):
            return eng.cell_events(*window(a, b), t0=a, records=rec, acc=acc, finish=finish, **kw)

        r["rec"] = _stream.walk_windows(T, B, step2)["rec"]
        if anomalies:  # the operands of the rates: gathers at the records' indices
            s, e = r["rec"]["start"].astype(np.int64), r["rec"]["end"].astype(np.int64)
            cell = np.repeat(np.arange(C, dtype=np.int64), np.diff(r["rec"]["off"]))
            r["rec"]["edge"] = [_gather(a_w, t, cell) for t in (np.maximum(s - 1, 0), s, e, np.minimum(e + 1, T - 1))]
    return r


def _rates(rec, T: int):
    """``(rate_onset, rate_decline)`` in float64 from the float32 operands; NaN where an operand is not finite."""
    before, first, last, after = (v.astype(np.float64) for v in rec["edge"])
    peak, s, e, tm = rec["vmax"].astype(np.float64), rec["start"].astype(np.int64), rec["end"].astype(np.int64), rec["tmax"].astype(np.int64)
    p, q = (tm - s).astype(np.float64), (e - tm).astype(np.float64)
    with np.errstate(invalid="ignore", divide="ignore", over="ignore"):
        on = np.where(s > 0, (peak - 0.5 * (before + first)) / (p + 0.5), (peak - first) / np.maximum(p, 1.0))
        off = np.where(e < T - 1, (peak - 0.5 * (last + after)) / (q + 0.5), (peak - last) / np.maximum(q, 1.0))
    ok = np.isfinite(peak)
    on = np.where(ok & np.isfinite(first) & ((s == 0) | np.isfinite(before)), on, np.nan)
    off = np.where(ok & np.isfinite(last) & ((e == T - 1) | np.isfinite(after)), off, np.nan)
    return on, off


def _cell_events(field, dat_anomaly, min_duration, max_gap, by, return_mask, records, block_steps, device):
    from .xr_compat import DataArray, Dataset

    p = _plan(field, dat_anomaly, min_duration, max_gap, by, block_steps)
    r = _device_pass(p, field, dat_anomaly, bool(return_mask), bool(records), device)
    T, C, _ratio = p["T"], p["C"], mo._ratio
    anomalies = dat_anomaly is not None
    grouped = p["grp"] is not None
    gname, gvals = (p["grp"][2], p["grp"][3]) if grouped else (None, None)
    gc = {gname: (gname, gvals)} if grouped else {}

    def space(v):
        return _stream.space(p, v if grouped else v[0], (gname,) if grouped else (), gc)

    data = {"events": space(r["events"]), "event_days": space(r["event_days"]), "duration_max": space(r["duration_max"]),
            "duration_mean": space(_ratio(r["event_days"], r["events"]))}
    if anomalies:
        valid = r["event_days"].astype(np.int64) - r["invalid"].astype(np.int64)
        data.update(intensity_max=space(r["vmax"]), intensity_cumulative=space(r["sum"]),
                    intensity_mean=space(_ratio(r["sum"], valid)), invalid_steps=space(r["invalid"]))
    if return_mask:
        m = r["mask"]
        on_device = type(m).__module__.startswith("torch")  # an empty field has a NumPy one
        if on_device and _tensor_of(field) is not None:
            import torch

            m = (m.view(torch.bool) if p["bool"] else m).reshape(p["shape"])
        else:
            m = (m.cpu().numpy() if on_device else m).astype(bool).reshape(p["shape"])
        tc = {} if p["tv"] is None else {p["tname"]: (p["tname"], p["tv"])}
        data["hobday_events"] = DataArray(m, dims=(p["tname"],) + tuple(p["sdims"]), coords={**p["scoords"], **tc})
    if records:
        rec = r["rec"]
        s, e = rec["start"], rec["end"]
        dur = (e.astype(np.int64) - s + 1).astype(np.int32)
        ev = lambda v: DataArray(v, dims=("event",))  # noqa: E731
        data.update(record_offsets=DataArray(rec["off"].astype(np.int64), dims=("cell_edge",)),
                    cell=ev(np.repeat(np.arange(C, dtype=np.int64), np.diff(rec["off"]))), start=ev(s), end=ev(e), duration=ev(dur))
        if anomalies:
            on, off = _rates(rec, T)
            data.update(record_intensity_max=ev(rec["vmax"]), time_of_max=ev(rec["tmax"]), record_intensity_cumulative=ev(rec["sum"]),
                        record_intensity_mean=ev(_ratio(rec["sum"], dur.astype(np.int64) - rec["invalid"].astype(np.int64))),
                        record_invalid_steps=ev(rec["invalid"]), rate_onset=ev(on), rate_decline=ev(off))
    return Dataset(data)


def cell_events(field, dat_anomaly=None, min_duration=5, max_gap=2, by=None, return_mask=False, records=False, block_steps=None,
                device=None):
    """The marine-heatwave events of every cell under the duration and gap rule of Hobday et al. (2016), from a streaming
    pass over the mask and the anomalies on the device.

    ``field``: ``extreme_events``, bool or uint8 (nonzero is present), ``(time, y, x)`` or ``(time, cells)``; any other type
    is refused.  ``dat_anomaly`` (optional): the anomalies, float32 (other float types are cast), same shape, dimension
    order and time coordinate.  Either may be a DataArray, an array or a device tensor, on the host or device resident
    (then it is read in place).  ``block_steps``: as in :func:`marex_amd.event_intensity`; no result depends on it, not
    even in the last bit.

    Per cell, in timesteps: a run of at least ``min_duration`` present steps qualifies; shorter runs are ignored and bridge
    nothing.  A qualifying run that starts at most ``max_gap`` steps after the end of the current event extends it (this
    chains), any other starts a new event.  An event spans ``start .. end`` inclusive, ``duration = end - start + 1``, gaps
    included.  A run that touches the first or the last step of the record counts by its observed length.

    Always returned, over the spatial dimensions of the field: ``events`` (uint32), ``event_days`` (uint32, the sum of the
    durations), ``duration_max`` (uint32) and ``duration_mean`` (float64 ``event_days / events``, NaN for none).  With
    ``dat_anomaly``, taken over all steps of the events, gap steps included: ``intensity_max`` (float32, the largest
    peak; NaN for none), ``intensity_cumulative`` (float64: the events' sums added in time order; each event's sum has one
    fixed order), ``intensity_mean`` (cumulative by the steps with a finite anomaly) and
    ``invalid_steps`` (uint32: steps of events whose anomaly is NaN or infinite; they count for nothing else).

    ``by``: ``"year"``, ``"season"``, ``"month"``, ``"dayofyear"`` or an integer label per timestep, as in
    :func:`marex_amd.event_occurrence`: every variable above gets a leading dimension named after the grouping.  An event
    belongs to the group of its START step, whole.

    ``return_mask=True`` adds ``hobday_events`` over the field's own dimensions: 1 exactly on the steps inside an event,
    gaps included -- a resident tensor of the field's type when the field was resident, a NumPy bool array otherwise.  It
    takes one byte per cell of the whole record on the device (:class:`TrackingError` with the figures when that does not
    fit).  :func:`marex_amd.local_intensity`, :func:`marex_amd.event_occurrence` and :class:`marex_amd.tracker` take it as
    their field.

    ``records=True`` adds the flat list of events over ``event``, ordered by cell, then by start: ``record_offsets`` (int64
    ``[cells + 1]``: the events of cell c are ``record_offsets[c] .. record_offsets[c + 1] - 1``), ``cell`` (int64, the
    flat cell index), ``start``, ``end``, ``duration`` (int32 steps) and with ``dat_anomaly`` ``record_intensity_max``
    (float32), ``time_of_max`` (int32, the earliest step that attains it; -1 for none), ``record_intensity_cumulative``,
    ``record_intensity_mean``, ``record_invalid_steps``, ``rate_onset`` and ``rate_decline`` (float64, anomaly per step:
    with ``p = time_of_max - start``, ``(peak - (a[start - 1] + a[start]) / 2) / (p + 0.5)``, at the record's first step
    ``(peak - a[start]) / max(p, 1)``, and the mirror image towards ``end``; NaN where an operand is not finite).  The
    records take a second pass of the same kernel over the field, with the offsets from the counts of the first: a host
    field walked in windows is uploaded a second time.

    Counts, durations and maxima are exact integers or float32 values; a sum is float64 in one fixed order."""
    return _cell_events(field, dat_anomaly, min_duration, max_gap, by, return_mask, records, block_steps, device)
