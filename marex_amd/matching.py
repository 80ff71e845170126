"""Event matching: which event of one tracking is which event of another -- a model against observations, the surface
against the subsurface, ``allow_merging=True`` against ``False``, two thresholds or two ensemble members -- over what area, for
how long, with which lag, and the hit rates that follow.  The join of two ``ID_field`` of the same shape: where
:func:`marex_amd.event_exposure` pairs events with a region map fixed in time, this pairs them with the events of a second
field.

The device part is the keyed accumulation of the exposure with a second streamed field (``marex_event_matching_count_i32`` /
``marex_event_matching_i32``): one pass per window over both fields into an open-addressing table keyed by
(step, event of A, event of B), the key one 64-bit word whose widths follow the IDs of the window.  The host sorts the
step-level records by (A, B, time) and derives everything per pair, per event and per step from them: exact integers, and
float64 values that are each one division of two exact integer sums.
"""
from __future__ import annotations

import numpy as np

from . import _stream, occurrence as mo
from ._stream import (_I32_MAX, _Windows, _check_block_steps, _first_where, _halves_f64, _halves_norm, _int_sum_halves, _starts,
                      pad_events, tracker_time)
from .exceptions import ConfigurationError, ProcessingError, create_data_validation_error

_FIELDS = ("t", "a", "b", "cells", "area")


def _plan(ID_field_a, ID_field_b, cell_areas, min_share, block_steps, time=None):
    """Everything that can be refused or derived without a device."""
    if ID_field_b is None:
        raise create_data_validation_error("event_matching needs two ID fields", details="ID_field_b is None")
    p = {"block_steps": _check_block_steps(block_steps),
         **_stream.plan_field(ID_field_a, "event_matching", ID_field_b, names=("ID_field_a", "ID_field_b"), presence_partner=True)}
    for kind, name in ((p["kind"], "ID_field_a"), (p["kind_b"], "ID_field_b")):
        if kind == "m":
            raise create_data_validation_error("event_matching needs ID fields, not masks",
                                               details=f"{name} is a mask; events are matched by their IDs: track the mask first")
    if isinstance(min_share, (bool, str)) or not isinstance(min_share, (int, float, np.integer, np.floating)) or \
            not 0.0 <= float(min_share) <= 1.0:
        raise ConfigurationError("min_share must be a number in 0 .. 1", details=f"min_share={min_share!r}")
    p["min_share"] = float(min_share)
    tracker_time(p, time, names=False)
    p["e"], p["q"], _ = _stream.area_tables(cell_areas, p)
    return p


def _no_records() -> dict:
    return {"t": np.zeros(0, np.int64), "a": np.zeros(0, np.int32), "b": np.zeros(0, np.int32), "cells": np.zeros(0, np.int64),
            "area": np.zeros(0, np.int64)}


def _host_values(field):
    return np.asarray(field.values if hasattr(field, "values") else field)


def _device_pass(p, ID_field_a, ID_field_b, device):
    """The step-level records of every window (``HotPath.event_matching``), sorted by (a, b, t)."""
    T, C = p["T"], p["C"]
    if T == 0 or C == 0:
        return _no_records()
    if _stream._tensor_of(ID_field_a) is None and _stream._tensor_of(ID_field_b) is None:
        ha, hb = _host_values(ID_field_a), _host_values(ID_field_b)
        if min(ha.min(), hb.min()) >= 0 and max(ha.max(), hb.max()) <= 0:  # host fields without an event need no device
            return _no_records()
    from .detect import get_engine

    eng = get_engine(0 if device is None else device)
    a_w = _Windows(eng, ID_field_a, T, C, np.int32, True)
    b_w = _Windows(eng, ID_field_b, T, C, np.int32, True)
    per = eng.matching_entry_bytes(p["q"] is not None)
    pieces = -(-C // 64)
    # a window's table is sized after its count pass; the plan allows one run per 64-cell piece and step, table and compacted
    # copy (5 entries per run at most) -- HotPath.event_matching checks the real figure
    per_step = a_w.upload_bytes_per_step + b_w.upload_bytes_per_step + 5 * per * pieces
    fixed = 8 * C if p["q"] is not None else 0
    B = _stream._window_steps(
        eng, "event_matching", T, C, per_step, fixed, p["block_steps"],
        f"{'the area of ' + str(C) + ' cells, ' if p['q'] is not None else ''}per timestep a table of {5 * pieces} entries of {per} "
        f"bytes, and the two ID fields of {T} timesteps, 4 bytes per cell each, as far as they are not on the device already")
    import torch

    q_d = None if p["q"] is None else torch.from_numpy(np.ascontiguousarray(p["q"])).to(eng.device)
    parts = []
    for a in range(0, T, B):
        b = min(T, a + B)
        parts.append(eng.event_matching(a_w.get(a, b), b_w.get(a, b), t0=a, q=q_d))
    rec = {k: np.concatenate([r[k] for r in parts]) for k in _FIELDS}
    if len(parts) > 1:  # the windows are in ascending time: a stable sort by (a, b) leaves every pair in time order
        order = np.lexsort((rec["b"], rec["a"]))
        rec = {k: v[order] for k, v in rec.items()}
    return rec


def _per_id(ids, t, cells, S, N: int) -> dict:
    """Per ID ``0 .. N`` of the records sorted by ``ids``: the exact area-steps in halves, the cell-steps, the first and the
    last step (``-1`` without a cell) and the number of distinct steps."""
    st = _starts(ids)
    who = ids[st].astype(np.int64)
    o = {k: np.zeros(N + 1, np.int64) for k in ("hi", "lo", "cell_steps", "steps")}
    o["first"], o["last"] = np.full(N + 1, -1, np.int64), np.full(N + 1, -1, np.int64)
    if st.size:
        o["hi"][who], o["lo"][who] = _int_sum_halves(S, st)
        o["cell_steps"][who] = np.add.reduceat(cells, st)
        o["first"][who], o["last"][who] = np.minimum.reduceat(t, st), np.maximum.reduceat(t, st)
        order = np.lexsort((t, ids))
        i2, t2 = ids[order], t[order]
        o["steps"] = np.bincount(i2[_starts(i2, t2)].astype(np.int64), minlength=N + 1).astype(np.int64)
    return o


def _side(d, name, tot, only, pid, partner, O_f, P, N, min_share):
    """The variables over one field's ``ID`` axis, from its totals ``tot``, its uncovered part ``only`` (halves per ID) and
    its pairs ``pid`` (sorted by this ID, then the partner's) with their overlap ``O_f``.  Returns the matched events."""
    dim = ("ID_" + name,)
    A_f = _halves_f64(tot["hi"], tot["lo"])
    seen = tot["cell_steps"] > 0
    pe = _starts(pid)
    pe_id = pid[pe]
    n_par, best, best_O = np.zeros(N + 1, np.int64), np.zeros(N + 1, np.int64), np.zeros(N + 1, np.float64)
    if P:
        width = np.diff(np.concatenate([pe, [P]]))
        n_par[pe_id] = width
        top = np.maximum.reduceat(O_f, pe)
        at = _first_where(O_f == top[np.repeat(np.arange(pe.size), width)], pe, P)  # ascending partner: the smaller wins a tie
        best[pe_id], best_O[pe_id] = partner[at], top
    m_f = _halves_f64(*_halves_norm(tot["hi"] - only[0], tot["lo"] - only[1]))  # the covered part, an exact integer
    share = np.where(seen, mo._ratio(m_f, A_f), np.nan)
    d.update({f"{name}_steps": (dim, tot["steps"][1:]), f"{name}_cell_steps": (dim, tot["cell_steps"][1:]),
              f"{name}_area_steps": (dim, A_f[1:]), f"{name}_matches": (dim, n_par[1:]), f"{name}_best_match": (dim, best[1:]),
              f"{name}_best_share": (dim, np.where(seen, mo._ratio(best_O, A_f), np.nan)[1:]),
              f"{name}_matched_share": (dim, share[1:])})
    with np.errstate(invalid="ignore"):
        return int(seen[1:].sum()), int((seen & (share > 0) & (share >= min_share))[1:].sum())


def _derive(rec, p, Na: int, Nb: int, tv, per_timestep: bool) -> dict:
    """``{name: (dims, values)}`` of everything per pair, event of either field, step and (``per_timestep``) record."""
    e, areas, T = p["e"], p["q"] is not None, p["T"]

    def to_area(f):  # exact: a power of two
        return np.ldexp(f, -e) if areas else f

    def times(idx):
        return tv[idx] if tv.size else tv[:0]

    a, b, t, cells, S = rec["a"], rec["b"], rec["t"], rec["cells"], rec["area"]
    # the whole events, the cells that the other field leaves uncovered included
    ia, ib = a > 0, b > 0
    tot_a = _per_id(a[ia], t[ia], cells[ia], S[ia], Na)
    ob = np.argsort(b, kind="stable")  # (b, a, t)
    ob = ob[b[ob] > 0]
    tot_b = _per_id(b[ob], t[ob], cells[ob], S[ob], Nb)
    la, lb = ia & ~ib, np.flatnonzero(~ia[ob])
    only_a = _per_id(a[la], t[la], cells[la], S[la], Na)
    only_b = _per_id(b[ob][lb], t[ob][lb], cells[ob][lb], S[ob][lb], Nb)
    # the records of the pairs
    keep = ia & ib
    r = {k: v[keep] for k, v in rec.items()}
    n = int(r["t"].size)
    st = _starts(r["a"], r["b"])
    P = int(st.size)
    off = np.concatenate([st, [n]]).astype(np.int64)
    steps = np.diff(off)
    seg = np.repeat(np.arange(P), steps)
    pa, pb = r["a"][st].astype(np.int64), r["b"][st].astype(np.int64)
    Sp = r["area"]
    o_hi, o_lo = _int_sum_halves(Sp, st)
    O_f = _halves_f64(o_hi, o_lo)
    s_max = np.maximum.reduceat(Sp, st) if P else np.zeros(0, np.int64)
    t_amax = r["t"][np.minimum(_first_where(Sp == s_max[seg], st, n), max(n - 1, 0))] if P else np.zeros(0, np.int64)
    A_f, B_f = _halves_f64(tot_a["hi"], tot_a["lo"]), _halves_f64(tot_b["hi"], tot_b["lo"])
    union = _halves_f64(*_halves_norm(tot_a["hi"][pa] + tot_b["hi"][pb] - o_hi, tot_a["lo"][pa] + tot_b["lo"][pb] - o_lo))
    d = {"pair_ID_a": (("pair",), pa), "pair_ID_b": (("pair",), pb), "pair_steps": (("pair",), steps.astype(np.int64)),
         "pair_time_start": (("pair",), times(r["t"][st])), "pair_time_end": (("pair",), times(r["t"][off[1:] - 1] if P else st)),
         "pair_cell_steps": (("pair",), np.add.reduceat(r["cells"], st) if P else np.zeros(0, np.int64)),
         "pair_area_steps": (("pair",), to_area(O_f)),
         "pair_cells_max": (("pair",), np.maximum.reduceat(r["cells"], st) if P else np.zeros(0, np.int64)),
         "pair_area_max": (("pair",), to_area(s_max.astype(np.float64))), "pair_time_of_max_area": (("pair",), times(t_amax)),
         "pair_share_of_a": (("pair",), mo._ratio(O_f, A_f[pa])), "pair_share_of_b": (("pair",), mo._ratio(O_f, B_f[pb])),
         "pair_iou": (("pair",), mo._ratio(O_f, union)),
         "pair_onset_lag": (("pair",), tot_b["first"][pb] - tot_a["first"][pa]),
         "pair_end_lag": (("pair",), tot_b["last"][pb] - tot_a["last"][pa])}
    # per event: the pairs of an event of A are consecutive and in ascending partner; those of B after a stable sort
    n_a, m_a = _side(d, "a", tot_a, (only_a["hi"], only_a["lo"]), pa, pb, O_f, P, Na, p["min_share"])
    ord_b = np.lexsort((pa, pb))
    n_b, m_b = _side(d, "b", tot_b, (only_b["hi"], only_b["lo"]), pb[ord_b], pa[ord_b], O_f[ord_b], P, Nb, p["min_share"])
    d["a_area_steps"] = (d["a_area_steps"][0], to_area(d["a_area_steps"][1]))
    d["b_area_steps"] = (d["b_area_steps"][0], to_area(d["b_area_steps"][1]))
    f64, i64 = np.float64, np.int64

    def rate(num, den):
        return f64(num / den) if den else f64(np.nan)

    d.update({"n_a": ((), i64(n_a)), "n_b": ((), i64(n_b)), "matched_a": ((), i64(m_a)), "matched_b": ((), i64(m_b)),
              "pod": ((), rate(m_a, n_a)), "far": ((), f64(1.0) - rate(m_b, n_b)), "csi": ((), rate(m_a, n_a + n_b - m_b))})
    whole = np.zeros(1, np.int64)
    for name, sel in (("both", keep), ("only_a", la), ("only_b", ~ia)):
        d["cell_steps_" + name] = ((), i64(cells[sel].sum()))
        hl = _int_sum_halves(S[sel], whole) if sel.any() else (whole, whole)
        d["area_steps_" + name] = ((), f64(to_area(_halves_f64(*hl))[0]))
        per_step = np.zeros(T, np.int64)
        np.add.at(per_step, t[sel], cells[sel])
        d["step_cells_" + name] = (("time",), per_step)
    if per_timestep:
        d.update({"pair_record_offsets": (("pair_edge",), off), "record_time": (("record",), times(r["t"])),
                  "record_cells": (("record",), r["cells"]), "record_area": (("record",), to_area(Sp.astype(np.float64)))})
    return d


def _event_matching(ID_field_a, ID_field_b, cell_areas, min_share, per_timestep, block_steps, device, n_events_a=None,
                    n_events_b=None, time=None):
    from .xr_compat import DataArray, Dataset

    p = _plan(ID_field_a, ID_field_b, cell_areas, min_share, block_steps, time)
    rec = _device_pass(p, ID_field_a, ID_field_b, device)
    tracker_time(p, time, fitting=True)
    tv = np.arange(p["T"]) if p["tv"] is None else np.asarray(p["tv"])
    N = []
    for key, n_events, name in (("a", n_events_a, "ID_field_a"), ("b", n_events_b, "ID_field_b")):
        n = pad_events(f"event_matching ({name})", int(rec[key].max()) if rec[key].size else 0, n_events)[0]
        if n == _I32_MAX:
            raise ProcessingError(f"event_matching: the per-event variables of {name} run over ID = 1 .. N, and N is 2^31 - 1",
                                  details="renumber sparse IDs densely")
        N.append(n)
    d = _derive(rec, p, N[0], N[1], tv, bool(per_timestep))
    tname = p["tname"]
    coords = {"ID_a": ("ID_a", np.arange(1, N[0] + 1, dtype=np.int64)), "ID_b": ("ID_b", np.arange(1, N[1] + 1, dtype=np.int64)),
              tname: (tname, tv)}
    data = {}
    for name, (dims, v) in d.items():
        dims = tuple(tname if k == "time" else k for k in dims)
        data[name] = DataArray(v, dims=dims, coords={k: coords[k] for k in dims if k in coords})
    return Dataset(data)


def event_matching(ID_field_a, ID_field_b, cell_areas=None, min_share=0.0, per_timestep=False, block_steps=None, device=None):
    """Which events of ``ID_field_a`` are which events of ``ID_field_b``: the join of two tracked fields, from one keyed
    pass over both on the device.

    ``ID_field_a``, ``ID_field_b``: two integer ``(time, y, x)`` or ``(time, cells)`` fields of the basic or the merge
    tracker, of the same shape, dimension order and time coordinate (an event is the cells of one ID ``> 0``; a negative
    value is refused, as by the trackers, naming the field; a mask is refused: matching needs IDs), each a DataArray, an
    array or a device tensor (then it is read in place), in any mix.  ``cell_areas``: None (every cell has area 1), or
    finite, non-negative areas in the spatial shape or, on a grid, a ``[y]`` vector broadcast along x; areas are exact
    integer sums of the fixed-point table of :func:`marex_amd.regional.area_weight_table`.  ``block_steps``: as in
    :func:`marex_amd.event_intensity`; the results do not depend on it.

    Over ``pair`` (an event of A and one of B that share at least one cell at one step), sorted by (ID_a, ID_b):
    ``pair_ID_a``, ``pair_ID_b``, ``pair_steps`` (the timesteps with a shared cell), ``pair_time_start``, ``pair_time_end``,
    ``pair_cell_steps`` (int64), ``pair_area_steps`` (float64, area x timesteps of the overlap: the exact integer sum,
    converted once), ``pair_cells_max``, ``pair_area_max`` and ``pair_time_of_max_area`` (the first step that reaches it),
    ``pair_share_of_a`` and ``pair_share_of_b`` (the overlap over the area-steps of the whole event, the cells that the
    other field leaves uncovered included), ``pair_iou`` (overlap / (A + B - overlap) in area-steps, the denominator formed
    as an exact integer) and ``pair_onset_lag`` / ``pair_end_lag`` (int64 steps: the first / last step of the event of B
    minus that of the event of A, of the whole events and not only of their overlap).

    Over ``ID_a = 1 .. Na`` (``Na`` the largest ID found in A), and the same with ``b_`` over ``ID_b = 1 .. Nb``:
    ``a_steps`` (the timesteps with a cell of the event: its duration), ``a_cell_steps``, ``a_area_steps``, ``a_matches``
    (its partners), ``a_best_match`` (the partner with the largest ``pair_area_steps``, the smaller ID on a tie, 0 for
    none), ``a_best_share`` (that pair's share of the event) and ``a_matched_share`` (the share of the event's area-steps
    that any event of the other field covers -- exact, because a cell holds one ID per field); the two shares are NaN for an
    ID without a cell.

    Scalars: ``n_a``, ``n_b`` (the events with a cell), ``matched_a``, ``matched_b`` (an event is matched when its matched
    share is ``> 0`` and ``>= min_share``), ``pod = matched_a / n_a``, ``far = 1 - matched_b / n_b`` and the critical
    success index ``csi = matched_a / (n_a + n_b - matched_b)`` -- hits over hits, misses and false alarms, with the hits
    counted among the events of A and the false alarms among those of B (NaN where a denominator is 0); the cell-level
    contingency ``cell_steps_both``, ``cell_steps_only_a``, ``cell_steps_only_b`` (int64) and ``area_steps_both``,
    ``area_steps_only_a``, ``area_steps_only_b`` (float64).  Over time: ``step_cells_both``, ``step_cells_only_a``,
    ``step_cells_only_b``.

    ``per_timestep=True`` adds the step-level records over ``record``, sorted by (ID_a, ID_b, time):
    ``pair_record_offsets`` (int64 ``[pairs + 1]`` over ``pair_edge``: the records of pair k are ``pair_record_offsets[k] ..
    pair_record_offsets[k + 1] - 1``), ``record_time``, ``record_cells`` and ``record_area``.

    Empty fields, ``T == 0`` and fields without events give empty Datasets of the same variables and types without
    device work.  Every count, area, step and time is exact, and every share is one float64 division of two exact
    integer sums, each converted once: equal from run to run, whatever the windows, the residency and the layout."""
    return _event_matching(ID_field_a, ID_field_b, cell_areas, min_share, per_timestep, block_steps, device)
