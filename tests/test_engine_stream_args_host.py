"""What the streaming statistics of ``HotPath`` (``event_intensity``, ``event_categories``, ``occurrence``, ``compound``,
``local_intensity``, ``cell_events``, ``cell_event_records``) hand to the library, to ``_check_fits`` and back to their caller,
and what they refuse, against a recording stub; and the steps per window their wrappers plan.  No device."""
import os
import sys

import numpy as np
import pytest
import torch

import marex_amd
import marex_amd._stream as ms
from marex_amd._keys import float_key
from marex_amd.engine import HotPath
from marex_amd.exceptions import DataValidationError, ProcessingError, TrackingError

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from cell_events_host_engine import HostEngine as CellEventsHost  # noqa: E402
from compound_host_engine import HostEngine as CompoundHost  # noqa: E402
from event_categories_host_engine import HostEngine as CategoriesHost  # noqa: E402
from local_intensity_host_engine import HostEngine as LocalIntensityHost  # noqa: E402

Tb, C, G, G2, R, N_EV, N_DOY, L = 2, 8, 2, 2, 2, 2, 3, 1
T = 2 * Tb
I32, I64, F32, F64, U8 = torch.int32, torch.int64, torch.float32, torch.float64, torch.uint8
GRP, SGRP, DOY = np.array([0, 1, 1, 0]), np.array([1, 0, 0, 1]), np.array([0, 2, 1, 0])
CLS = np.array([0, 1, 0, 1, -1, 1, 0, 2])
TMIN, TMAX = np.array([0, 0, 1]), np.array([0, 1, 3])  # event 1: steps 0..1, event 2: steps 1..3
OFF, SLOTS = [0, 0, 2, 5], 5


class _Ctx:
    handle = object()

    def __init__(self, log):
        self.log = log

    def check(self, rc, what):
        self.log.append(("check", rc, what))


class _Lib:
    def __init__(self, log):
        self.log = log

    def __getattr__(self, name):
        if not name.startswith("marex_"):
            raise AttributeError(name)

        def fn(*args):
            self.log.append((name, args))
            return 0

        return fn


def _engine():
    """``(engine, library calls, _check_fits calls)``."""
    log, fits = [], []
    hot = HotPath.__new__(HotPath)
    hot.device = torch.device("cpu")
    hot.ctx, hot.lib = _Ctx(log), _Lib(log)
    hot._bind_stream = lambda: None
    hot._check_fits = lambda nbytes, what, details: fits.append((nbytes, what, details))
    hot._dev = lambda a, dtype=None: torch.from_numpy(np.ascontiguousarray(a if dtype is None else a.astype(dtype)))
    return hot, log, fits


def _calls(log):
    return [e for e in log if e[0] != "check"]


def _p(t):
    return None if t is None else t.data_ptr()


def _layout(acc):
    """Tensors as (dtype, shape), arrays as their values, the rest as it is."""
    out = {}
    for k, v in acc.items():
        if isinstance(v, torch.Tensor):
            out[k] = (v.dtype, tuple(v.shape))
        elif isinstance(v, np.ndarray):
            out[k] = (str(v.dtype), v.tolist())
        else:
            out[k] = _layout(v) if isinstance(v, dict) else v
    return out


def _zeroed(acc, but=()):
    return all(not v.any() for k, v in acc.items() if isinstance(v, torch.Tensor) and k not in but)


def _bits(v):
    """The bytes of float32 values, every NaN as the one of NumPy (the sign of a zero counts)."""
    v = np.asarray(v)
    assert v.dtype == np.float32
    return np.where(np.isnan(v), np.float32(np.nan), v).tobytes()


def _refused(fn, cls, message, details):
    with pytest.raises(cls) as ei:
        fn()
    assert type(ei.value) is cls and ei.value.message == message and ei.value.details == details, \
        (ei.value.message, ei.value.details)
    return ei.value


def _ids():
    return torch.zeros((Tb, C), dtype=I32)


def _anom():
    return torch.zeros((Tb, C), dtype=F32)


def _mask(dtype=U8):
    return torch.zeros((Tb, C), dtype=dtype)


LABELS = {"grp": 4, "sgrp": 4, "cls": 8}
TAB3 = {"len": LABELS, "tabs": {k: (I32, (n,)) for k, n in LABELS.items()}}


# ------------------------------------------------------------------ valid calls
def test_event_intensity_calls():
    hot, log, fits = _engine()
    ids, anom, w = _ids(), _anom(), torch.ones(C)
    r = hot.event_intensity(ids, anom, TMIN, TMAX, w, finish=False)
    acc = r["acc"]
    assert sorted(r) == ["acc", "off"] and r["off"].tolist() == OFF and r["off"].dtype == np.int64
    assert fits == [(36 * SLOTS + 12 * 4, "event intensity",
                     "5 (timestep, event) slots between each event's first and last timestep, 36 bytes each, and the tables of "
                     "2 events")]
    assert _layout(acc) == {"cnt": (I64, (5, 2)), "sums": (F64, (5, 2)), "vmax": (I32, (5,)), "status": (I64, (1,)),
                            "tmin": (I32, (3,)), "off": (I64, (4,)), "plan": ("int64", OFF)}
    assert _zeroed(acc, ("tmin", "off")) and acc["tmin"].tolist() == [0, 0, 1] and acc["off"].tolist() == OFF

    def want(x, a, t0, wt):
        return ("marex_event_intensity_f32", (hot.ctx.handle, _p(x), _p(a), t0, Tb, C, N_EV, _p(acc["tmin"]), _p(acc["off"]), SLOTS,
                                              _p(wt), _p(acc["cnt"]), _p(acc["sums"]), _p(acc["vmax"]), _p(acc["status"])))

    assert _calls(log) == [want(ids, anom, 0, w)]
    ids2, anom2 = _ids(), _anom()
    acc["vmax"][:] = torch.from_numpy(float_key([1.5, -2.5, 0.0, -0.0, np.inf]).view(np.int32))
    acc["vmax"][2] = 0
    r2 = hot.event_intensity(ids2, anom2, TMIN, TMAX, w, t0=Tb, acc=acc)
    assert r2["acc"] is acc and len(fits) == 1 and _calls(log)[1:] == [want(ids2, anom2, Tb, w)]
    assert sorted(r2) == ["acc", "cnt", "off", "sums", "vmax"]
    assert r2["cnt"].shape == (5, 2) and r2["cnt"].dtype == np.int64 and r2["sums"].shape == (5, 2) and r2["sums"].dtype == np.float64
    assert r2["vmax"].dtype == np.float32 and _bits(r2["vmax"]) == _bits(np.array([1.5, -2.5, np.nan, -0.0, np.inf], np.float32))
    # no event has a step: one slot that nothing addresses, none returned
    hot, log, fits = _engine()
    r = hot.event_intensity(ids, anom, [0, 3, 3], [0, 2, -1])
    assert fits[0][0] == 12 * 4 and _calls(log)[0][1][9:11] == (1, None) and tuple(r["acc"]["cnt"].shape) == (1, 2)
    assert r["cnt"].shape == (0, 2) and r["vmax"].shape == (0,)


@pytest.mark.parametrize("weighted", [True, False])
def test_event_categories_calls(weighted):
    hot, log, fits = _engine()
    ids, anom, thr = _ids(), _anom(), torch.ones((N_DOY, C))
    w = torch.ones(C) if weighted else None
    field = torch.zeros((T, C), dtype=U8)
    r = hot.event_categories(ids, anom, TMIN, TMAX, thr, DOY, w, field=field)
    acc = r["acc"]
    per = 104 if weighted else 56
    assert sorted(r) == ["acc", "off"] and r["off"].tolist() == OFF
    assert fits == [(per * SLOTS + 12 * 4 + 4 * T + 16, "event categories",
                     f"5 (timestep, event) slots between each event's first and last timestep, {per} bytes each, the tables of "
                     "2 events and the row of every step")]
    assert _layout(acc) == {"cnt": (I64, (5, 7)), "area": (F64, (5, 6)) if weighted else None, "status": (I64, (2,)),
                            "tmin": (I32, (3,)), "off": (I64, (4,)), "plan": ("int64", OFF), "n_doy": N_DOY,
                            "len": {"doy": T}, "tabs": {"doy": (I32, (T,))}}
    assert _zeroed(acc, ("tmin", "off")) and acc["tabs"]["doy"].tolist() == DOY.tolist()

    def want(x, a, t0, f):
        return ("marex_event_categories_f32", (hot.ctx.handle, _p(x), _p(a), t0, Tb, C, N_EV, _p(acc["tmin"]), _p(acc["off"]), SLOTS,
                                               _p(thr), _p(acc["tabs"]["doy"]), N_DOY, _p(w), _p(acc["cnt"]), _p(acc["area"]), _p(f),
                                               _p(acc["status"])))

    assert _calls(log) == [want(ids, anom, 0, field)]
    ids2, anom2 = _ids(), _anom()
    acc["cnt"][1, 2] = 7
    r2 = hot.event_categories(ids2, anom2, TMIN, TMAX, thr, DOY, w, t0=Tb, acc=acc, finish=True)
    assert r2["acc"] is acc and len(fits) == 1 and _calls(log)[1:] == [want(ids2, anom2, Tb, None)]
    assert sorted(r2) == ["acc", "cat_area", "cat_cnt", "off"]
    assert r2["cat_cnt"].shape == (5, 7) and r2["cat_cnt"].dtype == np.int64 and r2["cat_cnt"][1, 2] == 7
    assert (r2["cat_area"].shape, r2["cat_area"].dtype) == ((5, 6), np.float64) if weighted else r2["cat_area"] is None


@pytest.mark.parametrize("dtype, ids", [(U8, ()), (torch.bool, ()), (I32, (3, 9))], ids=["u8", "bool", "i32"])
def test_occurrence_calls(dtype, ids):
    hot, log, fits = _engine()
    fn = "marex_occurrence_i32" if dtype == I32 else "marex_occurrence_u8"
    K = len(ids)
    x = _mask(dtype)
    r = hot.occurrence(x, 0, GRP, G, SGRP, G2, CLS, R, event_ids=ids, finish=False)
    acc = r["acc"]
    assert sorted(r) == ["acc"]
    assert fits == [(4 * G * C + 12 * C + 8 * G2 * R + 4 * K * C + 16 + 4 * (T + T + C), "occurrence",
                     f"2 x 8 uint32 counts, 3 x 8 uint32 run statistics, 2 x 2 uint64 section counts, {K} x 8 uint32 counts of "
                     "selected events, and the label tables")]
    assert _layout(acc) == {"cell_cnt": (I32, (G, C)), "runs": (I32, (3, C)), "sec_cnt": (I64, (G2, R)),
                            "dur": (I32, (K, C)) if K else None, "status": (I64, (2,)), "plan": (G, C, G2, R, True, tuple(ids)),
                            **TAB3}
    assert _zeroed(acc) and acc["tabs"]["cls"].tolist() == CLS.tolist()
    tb = acc["tabs"]

    def want(v, t0):
        h = hot.ctx.handle
        return [(fn, (h, _p(v), t0, Tb, C, 0, _p(tb["grp"]), G, _p(tb["sgrp"]), G2, _p(tb["cls"]), R, _p(acc["runs"]),
                      _p(acc["cell_cnt"]), _p(acc["sec_cnt"]), _p(acc["status"])))] + \
            [(fn, (h, _p(v), t0, Tb, C, ev, None, 1, None, 0, None, 0, None, _p(acc["dur"][k]), None, _p(acc["status"])))
             for k, ev in enumerate(ids)]

    assert _calls(log) == want(x, 0)
    if K:
        assert acc["dur"][1].data_ptr() == acc["dur"].data_ptr() + 4 * C
    x2 = _mask(dtype)
    r2 = hot.occurrence(x2, Tb, GRP, G, SGRP, G2, CLS, R, event_ids=ids, acc=acc)
    assert r2["acc"] is acc and len(fits) == 1 and _calls(log)[1 + K:] == want(x2, Tb)
    assert sorted(r2) == ["acc", "cell_cnt", "dur", "runs", "sec_cnt"]
    assert {k: (r2[k].dtype, r2[k].shape) for k in r2 if k != "acc"} == {
        "cell_cnt": (np.uint32, (G, C)), "runs": (np.uint32, (3, C)), "sec_cnt": (np.uint64, (G2, R)), "dur": (np.uint32, (K, C))}
    # no labels, no sections, no runs: NULL and zeros
    hot, log, fits = _engine()
    r = hot.occurrence(x, runs=False)
    a = r["acc"]
    assert fits[0][0] == 4 * C + 16 and "1 x 8 uint32 counts, 0 x 0 uint64 section counts, 0 x 8 uint32" in fits[0][2]
    assert _calls(log) == [(fn, (hot.ctx.handle, _p(x), 0, Tb, C, 0, None, 1, None, 0, None, 0, None, _p(a["cell_cnt"]), None,
                                 _p(a["status"])))]
    assert a["plan"] == (1, C, 0, 0, False, ()) and a["len"] == {"grp": None, "sgrp": None, "cls": None} == a["tabs"]
    assert r["runs"] is None and r["sec_cnt"] is None and r["dur"].shape == (0, C)


def test_compound_calls():
    hot, log, fits = _engine()
    a, b = _mask(), _mask(torch.bool)
    mask = torch.zeros((T, C), dtype=U8)
    r = hot.compound(a, b, 0, L, 1, GRP, G, SGRP, G2, CLS, R, mask=mask, finish=False)
    acc = r["acc"]
    assert sorted(r) == ["acc"]
    assert fits == [(4 * (3 * G + 13 + 3) * C + 24 * G2 * R + 16 + 4 * (T + T + C), "compound",
                     "3 x 2 x 8 uint32 counts, 13 x 8 uint32 of carried state, 3 x 8 uint32 lag counts, 3 x 2 x 2 uint64 section "
                     "counts, and the label tables")]
    assert _layout(acc) == {"cell_cnt": (I32, (3, G, C)), "state": (I32, (13, C)), "lag": (I32, (3, C)), "sec_cnt": (I64, (3, G2, R)),
                            "status": (I64, (2,)), "plan": (G, C, G2, R, L, 1), **TAB3}
    assert _zeroed(acc)
    tb = acc["tabs"]

    def want(u, v, t0, m):
        return ("marex_compound_u8", (hot.ctx.handle, _p(u), _p(v), t0, Tb, C, L, 1, _p(tb["grp"]), G, _p(tb["sgrp"]), G2,
                                      _p(tb["cls"]), R, _p(acc["state"]), _p(acc["cell_cnt"]), _p(acc["lag"]), _p(acc["sec_cnt"]),
                                      _p(m), _p(acc["status"])))

    assert _calls(log) == [want(a, b, 0, mask)]
    a2, b2 = _mask(), _mask()
    acc["state"][:] = torch.arange(13, dtype=I32)[:, None]
    r2 = hot.compound(a2, b2, Tb, L, 1, GRP, G, SGRP, G2, CLS, R, acc=acc)
    assert r2["acc"] is acc and len(fits) == 1 and _calls(log)[1:] == [want(a2, b2, Tb, None)]
    assert sorted(r2) == ["acc", "co", "days", "lag_days", "runs", "sec_cnt"]
    assert {k: (r2[k].dtype, r2[k].shape) for k in r2 if k != "acc"} == {
        "days": (np.uint32, (3, G, C)), "runs": (np.uint32, (3, C)), "co": (np.uint32, (4, C)), "lag_days": (np.uint32, (3, C)),
        "sec_cnt": (np.uint64, (3, G2, R))}
    assert r2["runs"][:, 0].tolist() == [0, 1, 2] and r2["co"][:, 0].tolist() == [7, 8, 9, 10]
    hot, log, fits = _engine()
    r = hot.compound(a, a2)
    assert fits[0][0] == 4 * 16 * C + 16 and _calls(log)[0][1][6:14] == (0, 0, None, 1, None, 0, None, 0)
    assert r["acc"]["lag"] is None and r["lag_days"] is None and r["sec_cnt"] is None and _calls(log)[0][1][16:19] == (None,) * 3


@pytest.mark.parametrize("dtype, match", [(U8, 0), (I32, 3)], ids=["u8", "i32"])
def test_local_intensity_calls(dtype, match):
    hot, log, fits = _engine()
    fn = "marex_local_intensity_i32" if dtype == I32 else "marex_local_intensity_u8"
    x, anom, thr = _mask(dtype), _anom(), torch.ones((N_DOY, C))
    kw = dict(grp=GRP, G=G, thr=thr, doy=DOY, sgrp=SGRP, G2=G2, cls=CLS, R=R, match=match)
    r = hot.local_intensity(x, anom, 0, finish=False, **kw)
    acc = r["acc"]
    assert sorted(r) == ["acc"]
    assert fits == [(G * C * 48 + 48 * G2 * R + 16 + 4 * (T + T + T + C), "local intensity",
                     "2 x 8 cells of 48 bytes (days, invalid, sum, maximum, its step, six category counts), 2 x 2 x 6 uint64 "
                     "section counts, and the label tables")]
    labels = {"grp": T, "doy": T, "sgrp": T, "cls": C}
    assert _layout(acc) == {"days": (I32, (G, C)), "invalid": (I32, (G, C)), "sum": (F64, (G, C)), "vmax": (I32, (G, C)),
                            "tmax": (I32, (G, C)), "cat_days": (I32, (G, 6, C)), "sec_cnt": (I64, (G2, R, 6)),
                            "status": (I64, (2,)), "plan": (G, C, N_DOY, G2, R, match), "len": labels,
                            "tabs": {k: (I32, (n,)) for k, n in labels.items()}}
    assert _zeroed(acc)
    tb = acc["tabs"]

    def want(v, a, t0):
        return (fn, (hot.ctx.handle, _p(v), _p(a), t0, Tb, C, match, _p(tb["grp"]), G, _p(thr), _p(tb["doy"]), N_DOY, _p(tb["sgrp"]),
                     G2, _p(tb["cls"]), R, _p(acc["days"]), _p(acc["invalid"]), _p(acc["sum"]), _p(acc["vmax"]), _p(acc["tmax"]),
                     _p(acc["cat_days"]), _p(acc["sec_cnt"]), _p(acc["status"])))

    assert _calls(log) == [want(x, anom, 0)]
    x2, anom2 = _mask(dtype), _anom()
    acc["vmax"][0, :3] = torch.from_numpy(float_key([-1.5, 2.0, -0.0]).view(np.int32))
    acc["tmax"][0, :4] = torch.tensor([3, 1, 2, 9], dtype=I32)  # cell 3 has no key: its step is not a step
    r2 = hot.local_intensity(x2, anom2, Tb, acc=acc, **kw)
    assert r2["acc"] is acc and len(fits) == 1 and _calls(log)[1:] == [want(x2, anom2, Tb)]
    assert sorted(r2) == ["acc", "cat_days", "days", "invalid", "sec_cnt", "sum", "tmax", "vmax"]
    assert {k: (r2[k].dtype, r2[k].shape) for k in r2 if k != "acc"} == {
        "days": (np.uint32, (G, C)), "invalid": (np.uint32, (G, C)), "sum": (np.float64, (G, C)), "vmax": (np.float32, (G, C)),
        "tmax": (np.int32, (G, C)), "cat_days": (np.uint32, (G, 6, C)), "sec_cnt": (np.uint64, (G2, R, 6))}
    assert _bits(r2["vmax"][0, :4]) == _bits(np.array([-1.5, 2.0, -0.0, np.nan], np.float32))
    assert r2["tmax"][0, :4].tolist() == [3, 1, 2, -1] and np.isnan(r2["vmax"][1]).all() and (r2["tmax"][1] == -1).all()
    hot, log, fits = _engine()
    r = hot.local_intensity(x, anom)
    assert fits[0][0] == 24 * C + 16 and "1 x 8 cells of 24 bytes (days, invalid, sum, maximum, its step), 0 x 0 x 6" in fits[0][2]
    assert _calls(log)[0][1][6:16] == (0, None, 1, None, None, 0, None, 0, None, 0)
    assert r["cat_days"] is None and r["sec_cnt"] is None and r["acc"]["plan"] == (1, C, 0, 0, 0, 0)


@pytest.mark.parametrize("anomalies", [True, False])
def test_cell_events_calls_of_both_passes_and_the_records(anomalies):
    hot, log, fits = _engine()
    x, anom = _mask(), _anom() if anomalies else None
    mask = torch.zeros((T, C), dtype=U8)
    kw = dict(min_duration=2, max_gap=1, grp=GRP, G=G)
    r = hot.cell_events(x, anom, 0, mask=mask, finish=False, **kw)
    acc = r["acc"]
    state, per = (56, 28) if anomalies else (16, 12)
    assert sorted(r) == ["acc"]
    assert fits == [(C * state + G * C * per + 16 + 4 * T, "cell events",
                     f"8 cells of carried state, {state} bytes each, 2 x 8 cells of accumulators, {per} bytes each, and the label "
                     "table")]
    gc = (I32, (G, C))
    assert _layout(acc) == {"state_i32": (I32, (10 if anomalies else 4, C)), "state_f64": (F64, (2, C)) if anomalies else None,
                            "status": (I64, (2,)), "plan": (G, C, anomalies, 2, 1, False), "events": gc, "event_days": gc,
                            "duration_max": gc, "sum": (F64, (G, C)) if anomalies else None, "vmax": gc if anomalies else None,
                            "invalid": gc if anomalies else None, "len": {"grp": T}, "tabs": {"grp": (I32, (T,))}}
    assert _zeroed(acc)

    def want(v, a, t0, fin, ac, m, rec):
        rp = tuple(_p(rec.get(k)) for k in ("off", "start", "end", "vmax", "tmax", "sum", "invalid"))
        return ("marex_cell_events_u8", (hot.ctx.handle, _p(v), _p(a), t0, Tb, C, 2, 1, fin, _p(ac["tabs"]["grp"]), G,
                                         _p(ac["state_i32"]), _p(ac["state_f64"]), _p(ac["events"]), _p(ac["event_days"]),
                                         _p(ac["duration_max"]), _p(ac["sum"]), _p(ac["vmax"]), _p(ac["invalid"]), _p(m)) + rp +
                (_p(ac["status"]),))

    assert _calls(log) == [want(x, anom, 0, 0, acc, mask, {})]
    x2, anom2 = _mask(torch.bool), _anom() if anomalies else None
    acc["events"][0, 0], acc["events"][1, 0], acc["events"][1, 3] = 1, 1, 2
    if anomalies:
        acc["vmax"][0, :2] = torch.from_numpy(float_key([-1.5, 2.0]).view(np.int32))
    r2 = hot.cell_events(x2, anom2, Tb, mask=mask, acc=acc, **kw)
    assert r2["acc"] is acc and len(fits) == 1 and _calls(log)[1:] == [want(x2, anom2, Tb, 1, acc, mask, {})]
    names = ["events", "event_days", "duration_max"] + (["sum", "vmax", "invalid"] if anomalies else [])
    assert sorted(r2) == sorted(["acc"] + names)
    dts = {"sum": np.float64, "vmax": np.float32}
    assert all(r2[k].dtype == dts.get(k, np.uint32) and r2[k].shape == (G, C) for k in names)
    if anomalies:
        assert _bits(r2["vmax"][0, :3]) == _bits(np.array([-1.5, 2.0, np.nan], np.float32)) and np.isnan(r2["vmax"][1]).all()
    # the records of the second pass: offsets from the counts, summed over the groups
    rec = hot.cell_event_records(acc)
    rb = 28 if anomalies else 8
    assert fits[1:] == [(rb * 4, "cell events", "4 event records of " + ("28 bytes (start, end, maximum, its step, float64 sum, "
                         "invalid steps)" if anomalies else "8 bytes (start, end)") + " for the second pass")]
    want_rec = {"off": (I64, (C + 1,)), "n": 4, "start": (I32, (4,)), "end": (I32, (4,))}
    if anomalies:
        want_rec.update(vmax=(I32, (4,)), tmax=(I32, (4,)), sum=(F64, (4,)), invalid=(I32, (4,)))
    assert _layout(rec) == want_rec and rec["off"].tolist() == [0, 2, 2, 2, 4, 4, 4, 4, 4]
    del log[:]
    r3 = hot.cell_events(x, anom, 0, records=rec, finish=False, **kw)
    acc2 = r3["acc"]
    assert fits[2:] == [(C * state + 16 + 4 * T, "cell events",
                         f"8 cells of carried state, {state} bytes each, 2 x 8 cells of accumulators, 0 bytes each, and the label "
                         "table")]
    assert _layout(acc2) == {"state_i32": (I32, (10 if anomalies else 4, C)), "state_f64": (F64, (2, C)) if anomalies else None,
                             "status": (I64, (2,)), "plan": (G, C, anomalies, 2, 1, True), "events": None, "event_days": None,
                             "duration_max": None, "sum": None, "vmax": None, "invalid": None, "len": {"grp": T},
                             "tabs": {"grp": (I32, (T,))}}
    assert _calls(log) == [want(x, anom, 0, 0, acc2, None, rec)]
    rec["start"][:], rec["end"][:] = torch.tensor([0, 2, 1, 3], dtype=I32), torch.tensor([1, 3, 2, 3], dtype=I32)
    if anomalies:
        rec["vmax"][:] = torch.from_numpy(np.concatenate([[0], float_key([-1.5, 2.0, -0.0]).view(np.int32)]).astype(np.int32))
        rec["tmax"][:] = torch.tensor([7, 1, 3, 2], dtype=I32)
        rec["sum"].zero_()
        rec["invalid"].zero_()
    r4 = hot.cell_events(x2, anom2, Tb, records=rec, acc=acc2, **kw)
    assert len(fits) == 3 and _calls(log)[1:] == [want(x2, anom2, Tb, 1, acc2, None, rec)]
    assert sorted(r4) == ["acc", "rec", "records"] and r4["records"] is rec
    h = r4["rec"]
    assert sorted(h) == sorted(k for k in rec if k != "n")
    assert h["off"].tolist() == rec["off"].tolist() and h["start"].tolist() == [0, 2, 1, 3] and h["end"].dtype == np.int32
    if anomalies:
        assert h["vmax"].dtype == np.float32 and _bits(h["vmax"]) == _bits(np.array([np.nan, -1.5, 2.0, -0.0], np.float32))
        assert h["tmax"].dtype == np.int32 and h["tmax"].tolist() == [-1, 1, 3, 2]
        assert h["sum"].dtype == np.float64 and h["invalid"].dtype == np.uint32
    # no event at all: one record that nothing addresses, none returned
    acc["events"].zero_()
    rec0 = hot.cell_event_records(acc)
    assert rec0["n"] == 0 and tuple(rec0["start"].shape) == (1,) and fits[-1][0] == 0
    assert hot.cell_events(x, anom, 0, records=rec0, **kw)["rec"]["start"].shape == (0,)


# ------------------------------------------------------------------ refused calls
GOT_W = "got torch.float64 (8,) on cpu"
GOT_THR = "got torch.float64 (3, 8) on cpu"
GOT_OUT = "got torch.uint8 (3, 8) on cpu"
SPANS = "ev_tmin and ev_tmax must have one entry per event 0..n_ev, n_ev > 0, and t0 must not be negative"
SECT = "the section counts need step labels, cell classes, G2 > 0 and R > 0 together"
OUT = "must be the whole contiguous uint8 [T, 8] output on the engine's device, T >= 4"


def _refusals():
    hot = _engine()[0]
    ids, anom, x, thr = _ids(), _anom(), _mask(), torch.ones((N_DOY, C))
    w64, thr64, short = torch.ones(C, dtype=F64), torch.ones((N_DOY, C), dtype=F64), torch.zeros((T - 1, C), dtype=U8)
    ei, ec, oc, co, li, ce = hot.event_intensity, hot.event_categories, hot.occurrence, hot.compound, hot.local_intensity, hot.cell_events
    return {
        "weights-intensity": (lambda: ei(ids, anom, TMIN, TMAX, w64),
                              "event_intensity: the weights must be a contiguous float32 [8] tensor on the engine's device", GOT_W),
        "weights-categories": (lambda: ec(ids, anom, TMIN, TMAX, thr, DOY, w64),
                               "event_categories: the weights must be a contiguous float32 [8] tensor on the engine's device", GOT_W),
        "spans-intensity": (lambda: ei(ids, anom, TMIN, TMAX[:2]), "event_intensity: " + SPANS, "spans (3,) / (2,), t0 = 0"),
        "spans-intensity-t0": (lambda: ei(ids, anom, TMIN, TMAX, t0=-1), "event_intensity: " + SPANS, "spans (3,) / (3,), t0 = -1"),
        "spans-categories": (lambda: ec(ids, anom, [0], [0], thr, DOY), "event_categories: " + SPANS, "spans (1,) / (1,), t0 = 0"),
        "thresholds-categories": (lambda: ec(ids, anom, TMIN, TMAX, thr64, DOY),
                                  "event_categories: the thresholds must be a contiguous float32 [n_doy, 8] tensor on the engine's "
                                  "device, with the row of every step", GOT_THR),
        "thresholds-categories-doy": (lambda: ec(ids, anom, TMIN, TMAX, thr, None),
                                      "event_categories: the thresholds must be a contiguous float32 [n_doy, 8] tensor on the "
                                      "engine's device, with the row of every step", "one of thr / doy is missing"),
        "thresholds-local": (lambda: li(x, anom, thr=thr64, doy=DOY),
                             "local_intensity: the categories need thresholds, a contiguous float32 [n_doy, 8] tensor on the "
                             "engine's device, and the row of every step", GOT_THR),
        "thresholds-local-doy": (lambda: li(x, anom, doy=DOY),
                                 "local_intensity: the categories need thresholds, a contiguous float32 [n_doy, 8] tensor on the "
                                 "engine's device, and the row of every step", "one of thr / doy is missing"),
        "sections-occurrence": (lambda: oc(x, sgrp=SGRP, G2=G2, R=R), "occurrence: " + SECT, "G2 = 2, R = 2"),
        "sections-compound": (lambda: co(x, x, sgrp=SGRP, cls=CLS, G2=G2), "compound: " + SECT, "G2 = 2, R = 0"),
        "sections-local": (lambda: li(x, anom, sgrp=SGRP, cls=CLS, G2=G2, R=R),
                           "local_intensity: the section counts need step labels, cell classes, G2 > 0, R > 0 and thresholds together",
                           "G2 = 2, R = 2, thresholds missing"),
        "sections-local-R": (lambda: li(x, anom, thr=thr, doy=DOY, sgrp=SGRP, cls=CLS, G2=G2),
                             "local_intensity: the section counts need step labels, cell classes, G2 > 0, R > 0 and thresholds "
                             "together", "G2 = 2, R = 0, thresholds given"),
        "output-categories": (lambda: ec(ids, anom, TMIN, TMAX, thr, DOY, t0=Tb, field=short), "event_categories: the field " + OUT,
                              GOT_OUT),
        "output-compound": (lambda: co(x, x, Tb, mask=short), "compound: the mask " + OUT, GOT_OUT),
        "output-cell-events": (lambda: ce(x, t0=Tb, mask=short), "cell_events: the mask " + OUT + ", and belongs to the summary pass",
                               GOT_OUT),
        "output-cell-events-records": (lambda: ce(x, t0=Tb, mask=torch.zeros((T, C), dtype=U8), records={}),
                                       "cell_events: the mask " + OUT + ", and belongs to the summary pass",
                                       "got torch.uint8 (4, 8) on cpu"),
        "labels-occurrence": (lambda: oc(x, G=G, event_ids=(0,)),
                              "occurrence: t0 must not be negative, G and the event IDs must be positive, and G > 1 needs labels",
                              "t0 = 0, G = 2, labels missing, event_ids [0]"),
        "labels-compound": (lambda: co(x, x, -1, 31, grp=GRP, G=G),
                            "compound: t0 must not be negative, G must be positive, G > 1 needs labels, and max_lag and tolerance "
                            "must lie in 0 .. 30", "t0 = -1, G = 2, labels given, max_lag = 31, tolerance = 0"),
        "labels-local": (lambda: li(x, anom, G=0, match=-1),
                         "local_intensity: t0 and match must not be negative, G must be positive, and G > 1 needs labels",
                         "t0 = 0, G = 0, labels missing, match = -1"),
        "labels-cell-events": (lambda: ce(x, min_duration=0, grp=GRP, G=G),
                               "cell_events: t0 and max_gap must not be negative, G and min_duration must be positive, and G > 1 "
                               "needs labels", "t0 = 0, G = 2, labels given, min_duration = 0, max_gap = 2"),
    }


@pytest.mark.parametrize("case", sorted(_refusals()))
def test_refused_arguments(case):
    fn, message, details = _refusals()[case]
    _refused(fn, ProcessingError, message, details)


def test_accumulators_of_another_plan_are_refused():
    hot, log, fits = _engine()
    ids, anom, x, thr, w = _ids(), _anom(), _mask(), torch.ones((N_DOY, C)), torch.ones(C)
    acc = hot.event_intensity(ids, anom, TMIN, TMAX, finish=False)["acc"]
    _refused(lambda: hot.event_intensity(ids, anom, TMIN, [0, 2, 3], t0=Tb, acc=acc), ProcessingError,
             "event_intensity: the accumulators were planned for other spans", "5 slots there, 6 here")
    _refused(lambda: hot.event_intensity(ids, anom, [0, 0, 2], [0, 2, 3], t0=Tb, acc=acc), ProcessingError,
             "event_intensity: the accumulators were planned for other spans", "5 slots there, 5 here")
    acc = hot.event_categories(ids, anom, TMIN, TMAX, thr, DOY)["acc"]
    _refused(lambda: hot.event_categories(ids, anom, TMIN, TMAX, thr, DOY, w, t0=Tb, acc=acc), ProcessingError,
             "event_categories: the accumulators were planned for another call", "5 slots and 3 threshold rows there, 5 and 3 here")
    _refused(lambda: hot.event_categories(ids, anom, TMIN, [0, 2, 3], thr[:2].contiguous(), DOY, t0=Tb, acc=acc), ProcessingError,
             "event_categories: the accumulators were planned for another call", "5 slots and 3 threshold rows there, 6 and 2 here")
    _refused(lambda: hot.event_categories(ids, anom, TMIN, TMAX, thr, DOY, t0=T - 1, acc=acc), ProcessingError,
             "event_categories: doy has 4 labels, the window ends at step 5", None)
    acc = hot.occurrence(x, 0, GRP, G, finish=False)["acc"]
    _refused(lambda: hot.occurrence(x, Tb, GRP, G, runs=False, acc=acc), ProcessingError,
             "occurrence: the accumulators were planned for another call",
             "(2, 8, 0, 0, True, ()) there, (2, 8, 0, 0, False, ()) here")
    _refused(lambda: hot.occurrence(x, T - 1, GRP, G, acc=acc), ProcessingError,
             "occurrence: grp has 4 labels, the window ends at step 5", None)
    _refused(lambda: hot.occurrence(torch.zeros((0, C), dtype=U8), Tb, GRP, G, acc=acc), ProcessingError,
             "occurrence: an empty window (0 steps of 8 cells)", None)
    acc = hot.compound(x, x, finish=False)["acc"]
    _refused(lambda: hot.compound(x, x, Tb, tolerance=2, acc=acc), ProcessingError,
             "compound: the accumulators were planned for another call", "(1, 8, 0, 0, 0, 0) there, (1, 8, 0, 0, 0, 2) here")
    acc = hot.local_intensity(x, anom, finish=False)["acc"]
    _refused(lambda: hot.local_intensity(x, anom, Tb, match=1, acc=acc), ProcessingError,
             "local_intensity: the accumulators were planned for another call", "(1, 8, 0, 0, 0, 0) there, (1, 8, 0, 0, 0, 1) here")
    acc = hot.cell_events(x, finish=False)["acc"]
    _refused(lambda: hot.cell_events(x, t0=Tb, max_gap=3, acc=acc), ProcessingError,
             "cell_events: the accumulators were planned for another call",
             "(1, 8, False, 5, 2, False) there, (1, 8, False, 5, 3, False) here")
    rec = hot.cell_event_records(hot.cell_events(x)["acc"])
    _refused(lambda: hot.cell_events(x, anom, records=rec), ProcessingError,
             "cell_events: the record buffers were planned for another call", "8 cells there, 8 here")
    assert len(log) == 2 * 7  # the first windows and the summary pass, nothing after a refusal


# ------------------------------------------------------------------ the host finish
def _finish(first, again, status):
    """The second window of a call whose status words the first one left at ``status``."""
    acc = first()["acc"]
    acc["status"][:] = torch.tensor(status, dtype=I64)
    return lambda: again(acc)


def test_status_words_raise_with_the_counts():
    hot = _engine()[0]
    ids, anom, x, thr = _ids(), _anom(), _mask(), torch.ones((N_DOY, C))
    xi = _mask(I32)
    neg = "Object IDs must be non-negative"
    lost = "present cells lie under a step label outside its range"
    tail = "; the cells were counted, nothing was written out of range"
    span = ("cells belong to an event outside its declared span of timesteps",
            "ev_tmin / ev_tmax do not cover the field; the cells were counted, not accumulated")
    e = _refused(_finish(lambda: hot.occurrence(xi, event_ids=(3,), finish=False), lambda a: hot.occurrence(xi, Tb, event_ids=(3,), acc=a),
                         [4, 9]), DataValidationError, neg, "2 negative cells; 0 is background")
    assert e.context == {"negative_cells": 2}
    _refused(_finish(lambda: hot.occurrence(x, 0, GRP, G, SGRP, G2, CLS, R, finish=False),
                     lambda a: hot.occurrence(x, Tb, GRP, G, SGRP, G2, CLS, R, acc=a), [0, 3]), ProcessingError,
             "occurrence: 3 " + lost, "grp must hold 0 .. 1, sgrp 0 .. 1" + tail)
    e = _refused(_finish(lambda: hot.compound(x, x, finish=False), lambda a: hot.compound(x, x, Tb, acc=a), [5, 0]),
                 DataValidationError, neg, "5 negative cells; 0 is background")
    assert e.context == {"negative_cells": 5}
    _refused(_finish(lambda: hot.compound(x, x, finish=False), lambda a: hot.compound(x, x, Tb, acc=a), [0, 1]), ProcessingError,
             "compound: 1 " + lost, "grp must hold 0 .. 0, sgrp 0 .. -1" + tail)
    kw = dict(grp=GRP, G=G, thr=thr, doy=DOY)
    _refused(_finish(lambda: hot.local_intensity(x, anom, finish=False, **kw), lambda a: hot.local_intensity(x, anom, Tb, acc=a, **kw),
                     [0, 7]), ProcessingError, "local_intensity: 7 " + lost, "grp must hold 0 .. 1, doy 0 .. 2, sgrp 0 .. -1" + tail)
    _refused(_finish(lambda: hot.local_intensity(xi, anom, finish=False), lambda a: hot.local_intensity(xi, anom, Tb, acc=a), [1, 0]),
             DataValidationError, neg, "1 negative cells; 0 is background")
    _refused(_finish(lambda: hot.event_intensity(ids, anom, TMIN, TMAX, finish=False),
                     lambda a: hot.event_intensity(ids, anom, TMIN, TMAX, t0=Tb, acc=a), [2]), ProcessingError,
             "event_intensity: 2 " + span[0], span[1])
    cat = lambda a=None, t0=0: hot.event_categories(ids, anom, TMIN, TMAX, thr, DOY, t0=t0, acc=a, finish=a is not None)  # noqa: E731
    _refused(_finish(cat, lambda a: cat(a, Tb), [2, 3]), ProcessingError, "event_categories: 2 " + span[0], span[1])
    _refused(_finish(cat, lambda a: cat(a, Tb), [0, 3]), ProcessingError,
             "event_categories: 3 event cells lie under a step label outside its range",
             "doy must hold 0 .. 2; the cells were counted, nothing was read out of range")
    ce = lambda a=None, t0=0: hot.cell_events(x, t0=t0, grp=GRP, G=G, acc=a, finish=a is not None)  # noqa: E731
    _refused(_finish(ce, lambda a: ce(a, Tb), [6, 1]), ProcessingError, "cell_events: 6 events start under a step label outside its range",
             "grp must hold 0 .. 1; the events were counted, nothing was written out of range")
    _refused(_finish(ce, lambda a: ce(a, Tb), [0, 1]), ProcessingError, "cell_events: 1 events found no room in the records of their cell",
             "the record offsets do not belong to this field; nothing was written out of range")


# ------------------------------------------------------------------ the window planner of the wrappers
BIG = (3, 10**6)  # the refusals come before any engine call: a shape whose gigabytes show in three decimals
AUTO = ["Pass block_steps='auto'", "Pass block_steps=<timesteps per window>"]


def _host(monkeypatch, eng, free):
    import marex_amd.detect as det

    monkeypatch.setattr(det, "get_engine", lambda device=0: eng)
    monkeypatch.setattr(ms, "_free_bytes", lambda e: free)
    return eng


def _windows(eng, name):
    return [tuple(c[-2:]) for c in eng.calls if c[0] == name and "records" not in c]


def _too_large(fn, message, details, suggestions):
    e = _refused(fn, TrackingError, message, details)
    assert e.suggestions == suggestions


def _plan_cases(fixed, per_step, free_auto):
    """``(block_steps, free bytes, windows)`` of a field of 6 steps; the arithmetic of the planner, written out."""
    assert (free_auto - free_auto // 16 - fixed) // per_step == 4 and fixed + per_step <= free_auto
    return [(None, fixed + 6 * per_step, [(0, 6)]), ("auto", free_auto, [(0, 4), (4, 2)]), (5, fixed + per_step, [(0, 5), (5, 1)]),
            ("auto", fixed + per_step, [(t, 1) for t in range(6)])]


def test_local_intensity_plans_its_windows(monkeypatch):
    x, a = np.ones((6, 5), bool), np.ones((6, 5), np.float32)
    for b, free, wins in _plan_cases(24 * 5, 5 + 20, 240):
        eng = _host(monkeypatch, LocalIntensityHost(), free)
        marex_amd.local_intensity(x, a, block_steps=b)
        assert [c[2:4] for c in eng.calls] == wins, (b, eng.calls)
    C_ = BIG[1]
    x, a = np.zeros(BIG, bool), np.zeros(BIG, np.float32)
    det = ("1 x 1000000 cells of accumulators, 24 bytes each, 0 x 1000000 float32 thresholds, and the field and the anomalies of "
           "3 timesteps, 1 + 4 bytes per cell, as far as they are not on the device already")
    sug = AUTO + ["Group by fewer labels"]
    _host(monkeypatch, LocalIntensityHost(), 24 * C_ + 15 * C_ - 1)
    _too_large(lambda: marex_amd.local_intensity(x, a), "local_intensity: needs 0.039 GB of device memory, 0.039 GB are free", det, sug)
    _host(monkeypatch, LocalIntensityHost(), 24 * C_ + 5 * C_ - 1)
    for b in ("auto", 2):
        _too_large(lambda: marex_amd.local_intensity(x, a, block_steps=b),
                   "local_intensity: needs 0.029 GB of device memory, 0.029 GB are free", det, sug)
    thr = torch.ones(C_)  # resident thresholds are no part of the need, a copy of them is
    det = det.replace("24 bytes each, 0 x", "48 bytes each, 1 x")
    _host(monkeypatch, LocalIntensityHost(), 48 * C_ + 15 * C_ - 1)
    for th, gb in ((thr, "0.063"), (thr.numpy(), "0.067"), (thr.to(torch.float64), "0.067")):
        _too_large(lambda: marex_amd.local_intensity(x, a, th), f"local_intensity: needs {gb} GB of device memory, 0.063 GB are free",
                   det, sug)


def test_cell_events_plans_its_windows(monkeypatch):
    x = np.ones((6, 5), bool)
    for b, free, wins in _plan_cases(16 * 5 + 12 * 5, 5, 172):
        eng = _host(monkeypatch, CellEventsHost(), free)
        marex_amd.cell_events(x, block_steps=b)
        assert _windows(eng, "cell_events") == wins, (b, eng.calls)
    C_ = BIG[1]
    x, a = np.zeros(BIG, bool), np.zeros(BIG, np.float32)
    _host(monkeypatch, CellEventsHost(), (56 + 28) * C_ + 3 * C_ + 15 * C_ - 1)
    _too_large(lambda: marex_amd.cell_events(x, a, return_mask=True), "cell_events: needs 0.102 GB of device memory, 0.102 GB are free",
               "1000000 cells of state and 1 x 1000000 cells of accumulators, 56 and 28 bytes each, the mask of 3 x 1000000 bytes, "
               "and the field and the anomalies of 3 timesteps, 1 + 4 bytes per cell, as far as they are not on the device already",
               AUTO + ["Group by fewer labels", "Pass return_mask=False"])
    _host(monkeypatch, CellEventsHost(), (16 + 12) * C_ + C_ - 1)
    _too_large(lambda: marex_amd.cell_events(x, block_steps="auto"), "cell_events: needs 0.029 GB of device memory, 0.029 GB are free",
               "1000000 cells of state and 1 x 1000000 cells of accumulators, 16 and 12 bytes each, and the field of 3 timesteps, "
               "1 bytes per cell, as far as they are not on the device already", AUTO + ["Group by fewer labels"])


def test_compound_events_plans_its_windows(monkeypatch):
    x = np.ones((6, 5), bool)
    for b, free, wins in _plan_cases(4 * 16 * 5, 5 + 5, 384):
        eng = _host(monkeypatch, CompoundHost(), free)
        marex_amd.compound_events(x, x, block_steps=b)
        assert _windows(eng, "compound") == wins, (b, eng.calls)
    C_ = BIG[1]
    x, y = np.zeros(BIG, bool), np.zeros(BIG, np.int32)
    _host(monkeypatch, CompoundHost(), 4 * 19 * C_ + 3 * C_ + 15 * C_ - 1)
    _too_large(lambda: marex_amd.compound_events(x, y, max_lag=1, return_mask=True),
               "compound_events: needs 0.094 GB of device memory, 0.094 GB are free",
               "19 x 1000000 uint32 of counts and carried state, 0 bytes of section counts, the joint mask of 3 x 1000000 bytes, and "
               "both fields of 3 timesteps, 1 and 4 bytes per cell, as far as they are not on the device already",
               AUTO + ["Pass return_mask=False"])
    _host(monkeypatch, CompoundHost(), 4 * 16 * C_ + 2 * C_ - 1)
    _too_large(lambda: marex_amd.compound_events(x, x, block_steps=1), "compound_events: needs 0.066 GB of device memory, 0.066 GB are free",
               "16 x 1000000 uint32 of counts and carried state, 0 bytes of section counts, and both fields of 3 timesteps, 1 and 1 "
               "bytes per cell, as far as they are not on the device already", AUTO)


def test_event_categories_plans_its_windows(monkeypatch):
    ids, a, thr = np.zeros((6, 5), np.int32), np.ones((6, 5), np.float32), np.ones(5, np.float32)
    ids[0, 0] = 1  # one slot of 104 bytes
    for b, free, wins in _plan_cases(4 * 5, 20 + 20, 200)[:3]:  # the slots need their own 104 bytes
        eng = _host(monkeypatch, CategoriesHost(), max(free, 4 * 5 + 104 + (240 if b is None else 40)))
        marex_amd.event_categories(ids, a, thr, block_steps=b)
        assert _windows(eng, "event_categories") == wins, (b, eng.calls)
        assert [c[1] for c in eng.calls if c[0] == "id_spans"] == [w[1] for w in wins]
    C_ = BIG[1]
    ids, a, thr = np.zeros(BIG, np.int32), np.zeros(BIG, np.float32), np.ones(C_, np.float32)
    _host(monkeypatch, CategoriesHost(), 4 * C_ + 3 * C_ + 24 * C_ - 1)
    _too_large(lambda: marex_amd.event_categories(ids, a, thr, return_field=True),
               "event_categories: needs 0.031 GB of device memory, 0.031 GB are free",
               "1 x 1000000 float32 thresholds, 0 (timestep, event) slots of 104 bytes, the category field of 3 x 1000000 bytes, and "
               "the ID field and the anomalies of 3 timesteps, 4 bytes per cell each, as far as they are not on the device already",
               AUTO + ["Pass return_field=False"])
    _host(monkeypatch, CategoriesHost(), 8 * C_ - 1)
    _too_large(lambda: marex_amd.event_categories(ids, a, torch.ones(C_), block_steps=2),
               "event_categories: needs 0.008 GB of device memory, 0.008 GB are free",
               "1 x 1000000 float32 thresholds (resident already), 0 (timestep, event) slots of 104 bytes, and the ID field and the "
               "anomalies of 3 timesteps, 4 bytes per cell each, as far as they are not on the device already", AUTO)
