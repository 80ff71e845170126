"""Event exposure: which tracked events touched which region, when, over what area and how intensely -- the join of the
events with the regions that follows the basin series of :func:`marex_amd.regional_series` in a study or an operational
monitor (which events entered this EEZ, basin, reef polygon or protected area; which region an event mainly belongs to; how
many events a region saw).

The result is sparse -- an event touches one or two regions, a region sees a small share of the events -- so the device part
is a keyed accumulation, not a dense slot array (``marex_event_exposure_count_i32`` / ``marex_event_exposure_i32``,
DESIGN.md section 4): one streaming pass per window over the ID field, the region rank, the area and the anomaly under its
event cells, into an open-addressing table keyed by (step, region, event).  The host sorts the step-level records by
(event, region, time) and derives everything per pair, per event and per region from them, in float64 and in ascending time.
"""
from __future__ import annotations

import numpy as np

from . import _stream, occurrence as mo
from ._keys import float_key, key_float
from ._stream import (_I32_MAX, _Windows, _check_block_steps, _first_where, _int_sum_f64, _seq_sum, _starts, pad_events, tracker_time,
                      weighted_mean)
from .exceptions import ProcessingError, create_data_validation_error
from .intensity import _time_of_max_values
from .regional import region_ranks


def _plan(ID_field, regions, cell_areas, dat_anomaly, mask, block_steps, time=None):
    """Everything that can be refused or derived without a device."""
    p = {"block_steps": _check_block_steps(block_steps),
         **_stream.plan_field(ID_field, "event_exposure", dat_anomaly, names=("ID_field", "dat_anomaly"))}
    if p["kind"] == "m":
        raise create_data_validation_error("event_exposure needs an ID field, not a mask",
                                           details="the exposure of an event is keyed by its ID; track the mask first")
    if regions is None:
        raise create_data_validation_error("event_exposure needs regions", details="an integer map over the spatial shape")
    tracker_time(p, time, names=False)
    rvals, rank = region_ranks(regions, mask, p)
    R = int(rvals.size)
    p.update(rvals=rvals, rank=rank, R=R)
    p["e"], p["q"], p["wf"] = _stream.area_tables(cell_areas, p)
    p["region_cells"], p["region_q"] = _stream.region_denominators(rank, p["q"], R)
    return p


_FIELDS = ("t", "rank", "id", "cells", "finite", "area", "sums", "vmax")


def _no_records(an: bool) -> dict:
    return {"t": np.zeros(0, np.int64), "rank": np.zeros(0, np.int32), "id": np.zeros(0, np.int32), "cells": np.zeros(0, np.int64),
            "finite": np.zeros(0, np.int64), "area": np.zeros(0, np.int64), "sums": np.zeros((0, 2)) if an else None,
            "vmax": np.zeros(0, np.float32) if an else None}


def _device_pass(p, ID_field, dat_anomaly, device):
    """The step-level records of every window (``HotPath.event_exposure``), sorted by (id, rank, t)."""
    T, C, R = p["T"], p["C"], p["R"]
    an = dat_anomaly is not None
    if T == 0 or C == 0 or R == 0:
        return _no_records(an)
    t_f = _stream._tensor_of(ID_field)
    if t_f is None:  # a host field without an event needs no device
        h = np.asarray(ID_field.values if hasattr(ID_field, "values") else ID_field)
        if h.min() >= 0 and h.max() <= 0:
            return _no_records(an)
    from .detect import get_engine

    eng = get_engine(0 if device is None else device)
    x_w = _Windows(eng, ID_field, T, C, np.int32, True)
    a_w = _Windows(eng, dat_anomaly, T, C, np.float32, False) if an else None
    per = eng.exposure_entry_bytes(p["q"] is not None, an)
    pieces = -(-C // 64)
    # a window's table is sized after its count pass; the plan allows one run per 64-cell piece and step, table and compacted
    # copy (5 entries per run at most) -- HotPath.event_exposure checks the real figure
    per_step = x_w.upload_bytes_per_step + (a_w.upload_bytes_per_step if an else 0) + 5 * per * pieces
    fixed = 4 * C + (12 * C if p["q"] is not None else 0)
    B = _stream._window_steps(
        eng, "event_exposure", T, C, per_step, fixed, p["block_steps"],
        f"the region{', area and weight' if p['q'] is not None else ''} of {C} cells, per timestep a table of {5 * pieces} "
        f"entries of {per} bytes, and the ID field{' and the anomalies' if an else ''} of {T} timesteps, 4{' + 4' if an else ''} "
        "bytes per cell, as far as they are not on the device already")
    B = min(B, 1 << eng.exposure_layout()["step_bits"])  # the step of the key
    import torch

    def up(v):
        return None if v is None else torch.from_numpy(np.ascontiguousarray(v)).to(eng.device)

    rank_d, q_d, w_d = up(p["rank"]), up(p["q"]), up(p["wf"] if an else None)
    parts = []
    for a in range(0, T, B):
        b = min(T, a + B)
        parts.append(eng.event_exposure(x_w.get(a, b), rank_d, R, t0=a, q=q_d, wf=w_d, anom=a_w.get(a, b) if an else None))
    rec = {k: (None if parts[0][k] is None else np.concatenate([r[k] for r in parts])) for k in _FIELDS}
    if len(parts) > 1:  # the windows are in ascending time: a stable sort by (id, rank) leaves every pair in time order
        order = np.lexsort((rec["rank"], rec["id"]))
        rec = {k: (None if v is None else v[order]) for k, v in rec.items()}
    return rec


def _derive(rec, p, N: int, tv, per_timestep: bool) -> dict:
    """``{name: (dims, values)}`` of everything per pair, event, region and (``per_timestep``) record."""
    R, e, areas = p["R"], p["e"], p["q"] is not None
    an = rec["sums"] is not None

    def to_area(f):  # exact: a power of two
        return np.ldexp(f, -e) if areas else f

    # per event, cells outside every region included
    ev_start = _starts(rec["id"])
    ev_id = rec["id"][ev_start].astype(np.int64)
    ev_area = np.zeros(N + 1, np.float64)
    ev_area[ev_id] = _int_sum_f64(rec["area"], ev_start)
    out_start = _starts(rec["id"][rec["rank"] == R])
    out_area = np.zeros(N + 1, np.float64)
    out_area[rec["id"][rec["rank"] == R][out_start].astype(np.int64)] = _int_sum_f64(rec["area"][rec["rank"] == R], out_start)
    # the records of the pairs
    keep = rec["rank"] < R
    r = {k: (None if v is None else v[keep]) for k, v in rec.items()}
    n = int(r["t"].size)
    st = _starts(r["id"], r["rank"])
    P = int(st.size)
    off = np.concatenate([st, [n]]).astype(np.int64)
    steps = np.diff(off)
    seg = np.repeat(np.arange(P), steps)
    pid, prank = r["id"][st].astype(np.int64), r["rank"][st].astype(np.int64)
    S = r["area"]
    a_steps = _int_sum_f64(S, st)
    s_max = np.maximum.reduceat(S, st) if P else np.zeros(0, np.int64)
    t_amax = r["t"][np.minimum(_first_where(S == s_max[seg], st, n), max(n - 1, 0))] if P else np.zeros(0, np.int64)
    region_area = to_area(p["region_q"].astype(np.float64))
    area_max = to_area(s_max.astype(np.float64))

    def times(idx):
        return tv[idx] if tv.size else tv[:0]

    d = {"pair_ID": (("pair",), pid), "pair_region": (("pair",), p["rvals"][prank] if P else np.zeros(0, np.int64)),
         "pair_steps": (("pair",), steps.astype(np.int64)),
         "pair_time_start": (("pair",), times(r["t"][st])), "pair_time_end": (("pair",), times(r["t"][off[1:] - 1] if P else st)),
         "pair_cell_steps": (("pair",), np.add.reduceat(r["cells"], st) if P else np.zeros(0, np.int64)),
         "pair_area_steps": (("pair",), to_area(a_steps)),
         "pair_cells_max": (("pair",), np.maximum.reduceat(r["cells"], st) if P else np.zeros(0, np.int64)),
         "pair_area_max": (("pair",), area_max), "pair_time_of_max_area": (("pair",), times(t_amax)),
         "pair_share_of_event": (("pair",), mo._ratio(a_steps, ev_area[pid])),
         "pair_region_share_max": (("pair",), mo._ratio(area_max, region_area[prank]))}
    if an:
        W, SA = r["sums"][:, 0], r["sums"][:, 1]
        key = np.where(np.isnan(r["vmax"]), np.uint32(0), float_key(r["vmax"])).astype(np.uint32)
        kmax = np.maximum.reduceat(key, st) if P else np.zeros(0, np.uint32)
        has = kmax != 0
        first = np.minimum(_first_where(key == kmax[seg], st, n), max(n - 1, 0)) if P else np.zeros(0, np.int64)
        pw, psa = _seq_sum(W, seg, P), _seq_sum(SA, seg, P)
        pfin = np.add.reduceat(r["finite"], st) if P else np.zeros(0, np.int64)
        d.update({"pair_intensity_max": (("pair",), np.where(has, key_float(kmax), np.float32(np.nan)).astype(np.float32)),
                  "pair_time_of_intensity_max": (("pair",), _time_of_max_values(tv, r["t"][first] if P else first, has)),
                  "pair_intensity_integral": (("pair",), psa),
                  "pair_intensity_mean": (("pair",), weighted_mean(pfin > 0, pw, psa)),
                  "pair_invalid_cells": (("pair",), (np.add.reduceat(r["cells"] - r["finite"], st) if P
                                                     else np.zeros(0, np.int64)))})
    # per event: the pairs of an event are consecutive and in ascending region
    pe = _starts(pid)
    pe_id = pid[pe]
    n_reg = np.zeros(N + 1, np.int64)
    n_reg[pe_id] = np.diff(np.concatenate([pe, [P]]))
    main = np.full(N + 1, -1, np.int64)
    if P:
        best = np.maximum.reduceat(a_steps, pe)
        eseg = np.repeat(np.arange(pe.size), np.diff(np.concatenate([pe, [P]])))
        main[pe_id] = p["rvals"][prank[_first_where(a_steps == best[eseg], pe, P)]]
    seen = np.zeros(N + 1, bool)
    seen[ev_id] = True
    d.update({"event_regions": (("ID",), n_reg[1:]), "event_main_region": (("ID",), main[1:]),
              "event_outside_share": (("ID",), np.where(seen, mo._ratio(out_area, ev_area), np.nan)[1:])})
    d.update({"region_events": (("region",), np.bincount(prank, minlength=R).astype(np.int64)),
              "region_event_steps": (("region",), np.bincount(prank, weights=steps, minlength=R).astype(np.int64)),
              "region_cells": (("region",), p["region_cells"]), "region_area": (("region",), region_area)})
    if per_timestep:
        d.update({"pair_record_offsets": (("pair_edge",), off), "record_time": (("record",), times(r["t"])),
                  "record_cells": (("record",), r["cells"]), "record_area": (("record",), to_area(S.astype(np.float64)))})
        if an:
            d.update({"record_intensity_max": (("record",), r["vmax"].astype(np.float32)),
                      "record_intensity_integral": (("record",), SA.astype(np.float64)),
                      "record_intensity_mean": (("record",), weighted_mean(r["finite"] > 0, W, SA)),
                      "record_invalid_cells": (("record",), r["cells"] - r["finite"])})
    return d


def _event_exposure(ID_field, regions, cell_areas, dat_anomaly, mask, per_timestep, block_steps, device, n_events=None, time=None):
    from .xr_compat import DataArray, Dataset

    p = _plan(ID_field, regions, cell_areas, dat_anomaly, mask, block_steps, time)
    rec = _device_pass(p, ID_field, dat_anomaly, device)
    tracker_time(p, time, fitting=True)
    tv = np.arange(p["T"]) if p["tv"] is None else np.asarray(p["tv"])
    N = pad_events("event_exposure", int(rec["id"].max()) if rec["id"].size else 0, n_events)[0]
    if N == _I32_MAX:
        raise ProcessingError("event_exposure: the per-event variables run over ID = 1 .. N, and N is 2^31 - 1",
                              details="renumber sparse IDs densely")
    d = _derive(rec, p, N, tv, bool(per_timestep))
    coords = {"ID": ("ID", np.arange(1, N + 1, dtype=np.int64)), "region": ("region", p["rvals"])}
    data = {}
    for name, (dims, v) in d.items():
        data[name] = DataArray(v, dims=dims, coords={k: coords[k] for k in dims if k in coords})
    return Dataset(data)


def event_exposure(ID_field, regions, cell_areas=None, dat_anomaly=None, mask=None, per_timestep=False, block_steps=None, device=None):
    """Which tracked events touched which region, when and how: the join of an ``ID_field`` with a region map, from one
    keyed pass over the field (and the anomalies under its event cells) on the device.

    ``ID_field``: the integer ``(time, y, x)`` or ``(time, cells)`` field of the basic or the merge tracker (an event is the
    cells of one ID ``> 0``; a negative value is refused, as by the trackers; a mask is refused: exposure needs IDs), a
    DataArray, an array or a device tensor (then it is read in place).  ``regions``: an integer map over the spatial shape --
    EEZs, ocean basins, reef polygons, protected areas; its distinct values ``>= 0``, ascending, are the ``region`` coordinate
    (at most 32 767), a value below 0 means no region.  ``mask`` removes cells from every region (and from the denominators
    ``region_cells`` / ``region_area``).  The cells of an event that lie in no region never appear as a pair but are counted,
    so that the totals of an event and the shares of them are exact.  ``cell_areas``: None (every cell has area 1), or
    finite, non-negative areas in the spatial shape or, on a grid, a ``[y]`` vector broadcast along x; areas are exact
    integer sums of the fixed-point table of :func:`marex_amd.regional.area_weight_table`.  ``block_steps``: as in
    :func:`marex_amd.event_intensity`; the results do not depend on it, the float64 sums within the bound below.

    Over ``pair``, sorted by (ID, region value): ``pair_ID``, ``pair_region``, ``pair_steps`` (the timesteps with at least
    one cell of the event in the region), ``pair_time_start``, ``pair_time_end``, ``pair_cell_steps`` (int64),
    ``pair_area_steps`` (float64, area x timesteps: the exact integer sum over the steps, converted once), ``pair_cells_max``,
    ``pair_area_max`` and ``pair_time_of_max_area`` (the first step that reaches it), ``pair_share_of_event``
    (``pair_area_steps`` over the area-steps of the whole event, the cells outside every region included) and
    ``pair_region_share_max`` (``pair_area_max`` over ``region_area``).

    ``dat_anomaly`` (float, same shape, dimension order and time coordinate) adds ``pair_intensity_max`` (float32, NaN where
    no cell has a finite anomaly), ``pair_time_of_intensity_max`` (the first step reaching it; NaT / NaN where none),
    ``pair_intensity_integral`` (float64: the sum of ``w a`` over the cell-steps with a finite anomaly, ``w`` the float32
    ``cell_areas``), ``pair_intensity_mean`` (integral over the sum of ``w``; NaN where no cell counts) and
    ``pair_invalid_cells`` (int64).  NaN rule: an event cell whose anomaly is NaN or infinite is a cell of the event -- it
    counts in the steps, the cells and the areas, which do not depend on whether anomalies are passed -- and is counted in
    ``pair_invalid_cells``; it reaches neither the sums nor the maximum.

    Over ``ID = 1 .. N`` (``N`` the largest ID found): ``event_regions`` (the regions the event touched),
    ``event_main_region`` (the region value with the largest ``pair_area_steps``, the smallest on a tie; -1 for an event
    that touched none) and ``event_outside_share`` (the share of the event's area-steps outside every region; NaN for an ID
    without a cell).  Over ``region``: ``region_events`` (the distinct events that touched it), ``region_event_steps`` (the
    sum of their ``pair_steps``), ``region_cells`` and ``region_area`` as :func:`marex_amd.regional_series` gives them.

    ``per_timestep=True`` adds the step-level records over ``record``, sorted by (ID, region, time):
    ``pair_record_offsets`` (int64 ``[pairs + 1]`` over ``pair_edge``: the records of pair k are ``pair_record_offsets[k] ..
    pair_record_offsets[k + 1] - 1``), ``record_time``, ``record_cells``, ``record_area`` and, with anomalies,
    ``record_intensity_max``, ``record_intensity_integral``, ``record_intensity_mean`` and ``record_invalid_cells``.

    An empty field, ``T == 0``, a field without events and a map without regions give empty Datasets of the same
    variables and types without device work.  Every count, area, maximum, step and time is exact: equal from run to run,
    whatever the windows, the residency and the layout.  The two float64 sums behind the intensities are sums of exact
    products in no fixed order: bit for bit reproducible where the partial sums are representable,
    otherwise within ``2 n u sum|w a|`` of the exact sum, ``n`` the cells of the record and ``u = 2^-53``; the host adds the
    records of a pair one after the other in ascending time."""
    return _event_exposure(ID_field, regions, cell_areas, dat_anomaly, mask, per_timestep, block_steps, device)
