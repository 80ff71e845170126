"""What the streaming statistics (``intensity``, ``event_categories``, ``shapes``, ``regional``, ``exposure``, ``occurrence``,
``local_intensity``, ``cell_events``, ``heat_stress``, ``resample``, ``compound``, ``composites``; ``trends`` for the free memory) share in front of the
engine: what a ``[time, space]`` field says without a device, the windows it is walked in -- with or without a part that
stays for the whole call -- and the way back to its spatial dimensions.  For the first five also the parser of a map or of
``cell_areas`` over space, the area table, the regions' denominators and the tracker's ``time`` triple; for the statistics over
(timestep, event) slots (the first three, ``track`` and ``exposure`` in part) the two-pass walk, the slot index and the padding;
for the keyed joins (``exposure``, ``matching``) the segment helpers of their sorted records."""
from __future__ import annotations

from typing import Optional

import numpy as np

from .exceptions import ConfigurationError, ProcessingError, TrackingError, create_data_validation_error
from .track import _BLOCK_CELLS, PINNED_ID_FIELD_BYTES, _host, _tensor_of
from .xr_compat import DataArray

_I32_MAX = 2**31 - 1


def _check_block_steps(block_steps):
    b = block_steps
    if b is not None and b != "auto" and (isinstance(b, (bool, str)) or not isinstance(b, (int, np.integer)) or b <= 0):
        raise ConfigurationError("block_steps must be a positive number of timesteps, 'auto' or None", details=f"block_steps={b!r}")
    return b if b is None or isinstance(b, str) else int(b)


def _dtype_name(x) -> str:
    t = _tensor_of(x)
    if t is not None:
        return str(t.dtype).replace("torch.", "")
    return str(x.dtype if hasattr(x, "dtype") else np.asarray(x).dtype)


def _kind(x) -> str:
    """'i' for an integer field, 'f' for a float one, '?' for anything else (bool, complex, objects)."""
    t = _tensor_of(x)
    if t is not None:
        if t.dtype.is_floating_point:
            return "f"
        return "?" if t.dtype.is_complex or "bool" in str(t.dtype) else "i"
    k = np.dtype(_dtype_name(x)).kind
    return "i" if k in "iu" else "f" if k == "f" else "?"


def _field_kind(field) -> str:
    """'m' for a mask (bool or uint8), 'i' for another integer field."""
    t = _tensor_of(field)
    name = _dtype_name(field) if t is None else str(t.dtype).replace("torch.", "")
    if name in ("bool", "uint8"):
        return "m"
    try:
        kind = np.dtype(name).kind
    except TypeError:
        kind = "?"
    if kind not in "iu":
        raise create_data_validation_error("field must be a mask (bool or uint8) or an integer ID field",
                                           details=f"Found dtype {name}", data_info={"actual_dtype": name})
    return "i"


def _time_of(field, T: int):
    """``(name, values or None)`` of the leading (time) dimension of a field."""
    dims = tuple(getattr(field, "dims", ()) or ())
    name = dims[0] if dims else "time"
    coords = getattr(field, "coords", None)
    if coords is None or not dims:
        return name, None
    c = coords[name] if name in coords else next((coords[k] for k in coords if tuple(getattr(coords[k], "dims", ())) == (name,)), None)
    if c is None:
        return name, None
    v = np.asarray(_host(c))
    return name, (v if v.shape == (T,) else None)


def _float_kind(field, name: str) -> str:
    """'f' for a floating-point field; anything else is refused under ``name``."""
    if _kind(field) != "f":
        raise create_data_validation_error(f"{name} must be a floating-point field", details=f"Found dtype {_dtype_name(field)}",
                                           data_info={"actual_dtype": _dtype_name(field)})
    return "f"


def plan_float_field(field, what: str, name: str = "sst") -> dict:
    """:func:`plan_field` of a float field that stands alone (``kind`` 'f'), called ``name`` in the refusals."""
    return plan_field(field, what, names=(name, None), floats=True)


def plan_field(field, what: str, partner=None, names=("field", "dat_anomaly"), presence_partner: bool = False,
               floats: bool = False) -> dict:
    """What a presence field says without a device: ``shape``, ``T``, ``C``, ``kind`` ('m' mask, 'i' IDs), ``bool``, the
    time axis (``tname``, ``tv``), the spatial dimensions ``sdims`` and their coordinates ``scoords``.  ``partner``: the
    anomaly field, which must agree in shape, dimensions and time; its names and coordinates fill in what the field lacks.
    ``presence_partner``: the partner is a second presence field, not a float one (adds ``kind_b`` and ``bool_b``);
    ``names``: what the errors call the two.  ``floats``: the field is a float one itself (:func:`plan_float_field`)."""
    fname, pname = names
    shape = tuple(int(k) for k in field.shape)
    if len(shape) not in (2, 3):
        raise create_data_validation_error("field must be (time, y, x) or (time, cells)", details=f"got shape {shape}")
    dims = tuple(getattr(field, "dims", ()) or ())
    d_a = ()
    if partner is not None:
        ashape = tuple(int(k) for k in partner.shape)
        if ashape != shape:
            raise create_data_validation_error(f"{fname} and {pname} differ in shape", details=f"{fname} {shape}, {pname} {ashape}")
        d_a = tuple(getattr(partner, "dims", ()) or ())
        if dims and d_a and dims != d_a:
            raise create_data_validation_error(f"{fname} and {pname} differ in their dimensions",
                                               details=f"{fname} {dims}, {pname} {d_a}; the order must agree too")
    kind = _float_kind(field, fname) if floats else _field_kind(field)
    kind_b = _field_kind(partner) if presence_partner and partner is not None else None
    if partner is not None and not presence_partner and _kind(partner) != "f":
        raise create_data_validation_error(f"{pname} must be a floating-point field",
                                           details=f"Found dtype {_dtype_name(partner)}",
                                           data_info={"actual_dtype": _dtype_name(partner)})
    T, C = shape[0], int(np.prod(shape[1:]))
    if C >= _I32_MAX or T >= _I32_MAX:
        raise TrackingError(f"{what}: a timestep of {C} cells or a record of {T} steps reaches 2^31 - 1",
                            details="the field may hold any number of cells, a single timestep and the time axis may not")
    tname, tv = _time_of(field, T)
    if partner is not None:
        _, tv_a = _time_of(partner, T)
        if tv is not None and tv_a is not None and not np.array_equal(tv, tv_a):
            raise create_data_validation_error(f"{fname} and {pname} differ in their time coordinate",
                                               details=f"the first difference is at step {int(np.argmax(tv != tv_a))}")
        tv = tv if tv is not None else tv_a
    labelled = dims or d_a
    sdims = labelled[1:] if labelled else (("y", "x") if len(shape) == 3 else ("cells",))
    coords = {}
    for src in (partner, field):  # the field's coordinates win
        for k, c in (getattr(src, "coords", None) or {}).items():
            cd = tuple(getattr(c, "dims", ()) or ())
            if cd and all(d in sdims for d in cd):
                coords[k] = (cd, np.asarray(_host(c)))
    p = dict(kind=kind, bool=_dtype_name(field) == "bool", shape=shape, T=T, C=C, tname=tname, tv=tv, labelled=bool(labelled),
             sdims=sdims, scoords=coords)
    if kind_b is not None:
        p.update(kind_b=kind_b, bool_b=_dtype_name(partner) == "bool")
    return p


def plan_sections(p: dict, zonal_by, lat, lat_bins):
    """``p["sec"]`` of a zonal call: ``(step labels of zonal_labels, cls int32 [C], R, class dimension, class coordinate
    or None, cells per class)`` -- the y rows of a grid, the latitude bins of a mesh."""
    from .occurrence import lat_classes, zonal_labels  # occurrence imports this module

    shape, sdims = p["shape"], p["sdims"]
    lab = zonal_labels(zonal_by, p["tv"], p["T"])
    if len(shape) == 3:
        if lat is not None or lat_bins is not None:
            raise create_data_validation_error("lat and lat_bins belong to a mesh: on a grid the classes are the y rows")
        ny, nx = shape[1], shape[2]
        cls = np.repeat(np.arange(ny, dtype=np.int32), nx)
        yc = p["scoords"].get(sdims[0])
        return (lab, cls, ny, sdims[0], None if yc is None else yc[1], np.full(ny, nx, np.int64))
    cls, R, e = lat_classes(lat, lat_bins, p["C"])
    return (lab, cls, R, "lat_bins", 0.5 * (e[:-1] + e[1:]), np.bincount(cls[cls >= 0], minlength=R).astype(np.int64))


def space(p: dict, v, lead=(), extra=None):
    """``v [*lead, C]`` over ``lead`` + the spatial dimensions of the field, with their coordinates and ``extra``."""
    c = dict(p["scoords"])
    c.update(extra or {})
    return DataArray(v.reshape(v.shape[:len(lead)] + p["shape"][1:]), dims=tuple(lead) + tuple(p["sdims"]), coords=c)


def section_coords(sec, extra=None):
    """``(zonal dimension, class dimension, coordinates of both and of extra, class_cells DataArray)`` of ``p["sec"]``."""
    (_, _, zname, zvals), _, _, cname, cvals, ccells = sec
    zc = {zname: (zname, zvals), **(extra or {})}
    if cvals is not None:
        zc[cname] = (cname, cvals)
    return zname, cname, zc, DataArray(ccells, dims=(cname,), coords={cname: zc[cname]} if cvals is not None else None)


def _free_bytes(eng) -> int:
    import torch

    free, _ = torch.cuda.mem_get_info(eng.device)
    return int(free + torch.cuda.memory_reserved(eng.device) - torch.cuda.memory_allocated(eng.device))


class _Windows:
    """The rows ``a .. b`` of a ``[T, C]`` field as a device tensor of one dtype: a view of a resident field (converted per
    window when its type differs), an upload of a host one -- through the engine's pinned pipe where the window is large."""

    def __init__(self, eng, field, T: int, C: int, np_dtype, is_ids: bool):
        import torch

        self.eng, self.np_dtype, self.is_ids = eng, np.dtype(np_dtype), is_ids
        self.item = self.np_dtype.itemsize
        self.tdt = torch.uint8 if self.np_dtype == np.uint8 else torch.int32 if is_ids else torch.float32
        t = _tensor_of(field)
        self.dev = self.host = None
        if t is not None:
            if t.dtype == torch.bool and self.tdt == torch.uint8:
                t = t.view(torch.uint8)  # the bytes of a bool tensor are 0 / 1: read in place
            if t.device != eng.device:
                t = t.to(eng.device)
            self.dev = t.reshape(T, C) if t.is_contiguous() else t.contiguous().reshape(T, C)
        else:
            self.host = np.asarray(field.values if hasattr(field, "values") else field).reshape(T, C)

    @property
    def upload_bytes_per_step(self) -> int:
        if self.host is not None:
            return self.item * self.host.shape[1]
        return 0 if self.dev.dtype == self.tdt else self.item * self.dev.shape[1]

    def _range_check(self, lo: int, hi: int) -> None:
        if lo < 0 or hi > _I32_MAX:
            from .track import tracker

            raise tracker._id_range_error(lo, hi)

    def get(self, a: int, b: int):
        import torch

        if self.dev is not None:
            x = self.dev[a:b]
            if x.dtype != self.tdt:
                if self.is_ids and x.numel():
                    self._range_check(int(x.min().item()), int(x.max().item()))
                x = x.to(self.tdt)
            return x
        h = self.host[a:b]
        if self.is_ids and h.dtype != np.int32 and h.size:
            self._range_check(int(h.min()), int(h.max()))
        if h.shape[0] * h.shape[1] * self.item >= PINNED_ID_FIELD_BYTES:
            from .detect import _pipe

            return _pipe(self.eng).upload(h, self.np_dtype)
        return torch.from_numpy(np.ascontiguousarray(h, dtype=self.np_dtype)).to(self.eng.device)


def _plan_windows(eng, T: int, C: int, per_step: int, block_steps, what: str = "event_intensity", details: Optional[str] = None):
    """Steps per window.  ``per_step``: bytes a window takes per timestep beyond what is resident already.  ``what`` /
    ``details`` word the error of a field that does not fit whole."""
    cap = max(1, _BLOCK_CELLS // C)  # the span kernels take blocks below 2^31 - 1 cells
    if block_steps is None:
        free = _free_bytes(eng)
        if T * per_step > free:
            raise TrackingError(f"{what}: needs {T * per_step / 1e9:.3f} GB of device memory, {free / 1e9:.3f} GB are free",
                                details=details or
                                f"the ID field and the anomalies of {T} timesteps of {C} cells, 4 bytes per cell each, "
                                "as far as they are not on the device already",
                                suggestions=["Pass block_steps='auto'", "Pass block_steps=<timesteps per window>"])
        return min(T, cap)
    if block_steps == "auto":
        free = _free_bytes(eng)
        free -= free // 16  # the slots, the small tables and the allocator's rounding
        return max(1, min(T, cap, free // per_step if per_step else T))
    return min(int(block_steps), T, cap)


def _window_steps(eng, what: str, T: int, C: int, per_step: int, fixed: int, block_steps, details: str, suggestions=()) -> int:
    """Steps per window of a call that keeps ``fixed`` bytes for its whole length (accumulators, carried state, thresholds,
    a whole output) beside the ``per_step`` bytes of :func:`_plan_windows`.  ``suggestions``: what the caller can offer
    beyond windows when the call does not fit."""
    free = _free_bytes(eng)
    need = fixed + per_step * (T if block_steps is None else 1)
    if need > free:
        raise TrackingError(f"{what}: needs {need / 1e9:.3f} GB of device memory, {free / 1e9:.3f} GB are free", details=details,
                            suggestions=["Pass block_steps='auto'", "Pass block_steps=<timesteps per window>", *suggestions])
    B = _plan_windows(eng, T, C, per_step, block_steps, what, details)
    if block_steps == "auto" and per_step:
        B = max(1, min(B, (free - free // 16 - fixed) // per_step))
    return B


def walk_windows(T: int, B: int, step):
    """The last result of ``step(a, b, acc, finish)`` over the windows of ``B`` steps, each given the ``"acc"`` before it."""
    acc = r = None
    for a in range(0, T, B):
        r = step(a, min(T, a + B), acc, a + B >= T)
        acc = r["acc"]
    return r


def spatial(v, p: dict, name: str, row_vector: bool = False, mismatch: Optional[str] = None, numbers: bool = False):
    """``v`` flat over the cells of a timestep of the planned field ``p`` (``shape``, ``labelled``, ``sdims``): given in the
    spatial shape, flat, transposed under the field's own dimension names, or -- ``row_vector`` -- as a ``[y]`` vector
    broadcast along x.  ``mismatch``: the caller's wording of the refusal; ``numbers``: anything but numbers is refused too."""
    a = np.asarray(_host(v))
    if numbers and a.dtype.kind not in "fiu":
        raise create_data_validation_error(f"{name} must be numbers", details=f"Found dtype {a.dtype}")
    sp = tuple(p["shape"][1:])
    d = tuple(getattr(v, "dims", ()) or ())
    if len(sp) == 2 and a.ndim == 2 and d and p["labelled"] and d == (p["sdims"][1], p["sdims"][0]):
        a = a.T
    if a.shape == sp or a.shape == (int(np.prod(sp)),):
        return np.ascontiguousarray(a).reshape(-1)
    if row_vector and len(sp) == 2 and a.shape == (sp[0],):
        return np.ascontiguousarray(np.broadcast_to(a[:, None], sp)).reshape(-1)
    raise create_data_validation_error(mismatch or f"{name} does not match the spatial shape of the field",
                                       details=f"{name} {a.shape}, a timestep {sp}")


def area_weight_table(cell_areas):
    """``(e, q)``: the fixed-point areas of the cells, ``q = rint(a * 2^e)`` int64 in the shape of ``cell_areas`` with
    ``a = float64(cell_areas)`` and ``e = 61 - ceil(log2(sum(a)))`` -- the rule, and the bits, of row 0 of
    ``track_mesh.mesh_weight_tables``: the sum of ``q`` over any set of cells stays below 2^62, so 64-bit integer sums
    cannot overflow, and an area is ``ldexp(float64(S), -e)`` of its integer sum ``S``.  :class:`DataValidationError` for
    an area that is negative or not finite, or areas that sum to zero.  Needs no GPU."""
    a = np.ascontiguousarray(np.asarray(_host(cell_areas), dtype=np.float64))
    flat = a.reshape(-1)
    if flat.size == 0 or not np.isfinite(flat).all() or (flat < 0).any():
        raise create_data_validation_error("cell_areas must be finite and non-negative",
                                           details=f"{int((~np.isfinite(flat)).sum())} non-finite and {int((flat < 0).sum())} "
                                                   f"negative of {flat.size} values")
    total = float(flat.sum())
    if not (total > 0 and np.isfinite(total)):
        raise create_data_validation_error("cell_areas must have a positive, finite sum", details=f"sum {total}")
    e = 61 - int(np.ceil(np.log2(total)))
    return e, np.rint(np.ldexp(flat, e)).astype(np.int64).reshape(a.shape)


def area_tables(cell_areas, p: dict):
    """``(e, q, wf)`` of the ``cell_areas`` of a region statistic: the exponent and the int64 ``[C]`` areas of
    :func:`area_weight_table`, and the float32 weights of the anomaly sums; ``(0, None, None)`` without areas or cells."""
    a = None if cell_areas is None else spatial(cell_areas, p, "cell_areas", row_vector=True, numbers=True)
    if a is None or not p["C"]:
        return 0, None, None
    return (*area_weight_table(a), np.ascontiguousarray(a, dtype=np.float32))


def region_denominators(rank, q, R: int):
    """``(region_cells, region_q)`` int64 ``[R]``: the cells of every region and their fixed-point area (the cells again
    without ``q``), exact host integers, over the cells with ``rank >= 0``."""
    ok = rank >= 0
    cells = np.bincount(rank[ok], minlength=R).astype(np.int64)
    if q is None:
        return cells, cells
    ra = np.zeros(R, np.int64)
    np.add.at(ra, rank[ok], q[ok])
    return cells, ra


def tracker_time(p: dict, time, names: bool = True, fitting: bool = False) -> None:
    """Applies a tracker's ``time`` triple ``(time dimension, time coordinate, values)`` to the plan ``p`` (``T``, ``tname``,
    ``tv``; adds ``tcoord``, None without a tracker): its names and values replace the field's -- with ``fitting`` the values
    only if they have the field's length.  Without ``names`` only its values, where they fit and the field has no time coordinate."""
    p.setdefault("tcoord", None)
    if time is None:
        return
    if names:
        p["tname"], p["tcoord"] = time[0], time[1]
    fits = len(time[2]) == p["T"]
    if (names and not fitting) or (fits and (names or p["tv"] is None)):
        p["tv"] = np.asarray(time[2])


def weighted_mean(some, W, SA):
    """``SA / W`` where ``some`` holds and ``W`` is not 0, NaN elsewhere."""
    with np.errstate(invalid="ignore", divide="ignore"):
        return np.where(some & (W != 0), SA / np.where(W != 0, W, 1.0), np.nan)


def _starts(*keys):
    """The first index of every run of equal key tuples in sorted vectors."""
    n = keys[0].size
    if n == 0:
        return np.zeros(0, np.int64)
    new = np.zeros(n, bool)
    new[0] = True
    for k in keys:
        new[1:] |= k[1:] != k[:-1]
    return np.flatnonzero(new).astype(np.int64)


def _int_sum_f64(S, starts):
    """The float64 of the exact sum of the non-negative int64 ``S`` over the segments that begin at ``starts``: the sum is
    carried in two halves of 32 bits, so that any number of terms below 2^62 cannot overflow, and converted once."""
    return _halves_f64(*_int_sum_halves(S, starts))


def _int_sum_halves(S, starts):
    """``(hi, lo)`` int64 with ``hi * 2^32 + lo`` the exact sum of the non-negative int64 ``S`` over the segments that begin
    at ``starts`` and ``0 <= lo < 2^32``.  Sums and differences of such pairs stay exact: add or subtract the halves and
    pass them through :func:`_halves_norm`."""
    if starts.size == 0:
        return np.zeros(0, np.int64), np.zeros(0, np.int64)
    return _halves_norm(np.add.reduceat(S >> 32, starts), np.add.reduceat(S & 0xFFFFFFFF, starts))


def _halves_norm(hi, lo):
    """The same integer ``hi * 2^32 + lo`` with ``0 <= lo < 2^32`` (``lo`` may come in negative: the shift floors)."""
    return hi + (lo >> 32), lo & 0xFFFFFFFF


def _halves_f64(hi, lo):
    """The float64 of the non-negative integer ``hi * 2^32 + lo`` (normalised halves), rounded once."""
    if hi.size == 0:
        return np.zeros(0, np.float64)
    small = hi < 2**30  # the whole sum fits int64: its conversion rounds once
    out = ((np.where(small, hi, 0) << 32) + lo).astype(np.float64)
    for k in np.flatnonzero(~small):  # rare: a Python integer, rounded once by float()
        out[k] = float((int(hi[k]) << 32) + int(lo[k]))
    return out


def _first_where(hit, starts, n):
    """Per segment the first index at which ``hit`` holds (``n`` where none does)."""
    return np.minimum.reduceat(np.where(hit, np.arange(n), n), starts) if starts.size else np.zeros(0, np.int64)


def _seq_sum(v, seg, n_seg):
    """Per segment the float64 sum of ``v``, one element after the other in the order given (ascending time)."""
    out = np.zeros(n_seg, np.float64)
    np.add.at(out, seg, v)
    return out


def event_spans(eng, ids_w, T: int, B: int):
    """The first pass of a slot statistic over an ID field in windows of ``B`` steps: ``(N, tmin, tmax, wins, kept)`` -- the
    largest event number, the first and last step of the events 0..N (int64, entry 0 unused), the windows ``(a, b)`` and the
    window itself where the field is taken whole."""
    wins = [(a, min(T, a + B)) for a in range(0, T, B)]
    kept = None
    tmin, tmax = np.full(1, _I32_MAX, np.int64), np.full(1, -1, np.int64)
    for a, b in wins:
        x = ids_w.get(a, b)
        sp = eng.id_spans(x)
        if len(wins) == 1:
            kept = x
        if sp is None:
            continue
        lo, hi = sp[0].astype(np.int64), sp[1].astype(np.int64)
        if lo.size > tmin.size:
            grow = lo.size - tmin.size
            tmin = np.concatenate([tmin, np.full(grow, _I32_MAX, np.int64)])
            tmax = np.concatenate([tmax, np.full(grow, -1, np.int64)])
        seen = hi >= 0
        n = lo.size
        tmin[:n] = np.where(seen, np.minimum(tmin[:n], lo + a), tmin[:n])
        tmax[:n] = np.where(seen, np.maximum(tmax[:n], hi + a), tmax[:n])
        del x
    tmin[0], tmax[0] = _I32_MAX, -1
    return int(tmin.size) - 1, tmin, tmax, wins, kept


def walk_event_slots(ids_w, wins, kept, step):
    """The second pass: the last result of ``step(x, a, b, acc, finish)`` over the windows of :func:`event_spans`, each given
    its rows ``x`` (``kept``, or fetched again), the ``"acc"`` of the result before it, and ``finish`` on the last."""
    acc = r = None
    for i, (a, b) in enumerate(wins):
        r = step(kept if kept is not None else ids_w.get(a, b), a, b, acc, i == len(wins) - 1)
        acc = r["acc"]
    return r


def slot_index(off, tmin, N: int):
    """``(e_of, t_of)``: the event and the timestep of every (timestep, event) slot -- event ``e`` of 1..N owns the slots
    ``off[e] .. off[e + 1] - 1``, one per step from ``tmin[e]`` on."""
    e_of = np.repeat(np.arange(N + 1), np.diff(off)[:N + 1])
    return e_of, np.arange(e_of.size) - off[e_of] + tmin[e_of]


def pad_events(what: str, N: int, n_events: Optional[int], tmin=None, off=None):
    """``(N, tmin, off)`` stretched to the ``n_events`` of the events Dataset (None: as they are): trailing events without
    a cell get no slot.  :class:`ProcessingError` where the field holds an event beyond them."""
    if n_events is None:
        return N, tmin, off
    if N > n_events:
        raise ProcessingError(f"{what}: the ID field holds event {N}, the events Dataset ends at {n_events}")
    if N < n_events and tmin is not None:
        tmin = np.concatenate([tmin, np.full(n_events - N, _I32_MAX, np.int64)])
        off = np.concatenate([off[:N + 2], np.full(n_events - N, off[N + 1], np.int64)])
    return int(n_events), tmin, off
