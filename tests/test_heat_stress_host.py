"""Heat stress on the host: the two restatements of tests/heat_stress_oracle.py against each other and against hand-computed
columns, the exactness of the running sum, the refusals (raised before any device work), what ``HotPath.group_mean`` and
``HotPath.heat_stress`` hand to the library against a recording stub, and the public path -- labels, baseline, windows with
their history rows, the carried state, the Dataset -- on a NumPy stand-in for the engine calls.  No GPU needed."""
import math
import os
import sys

import numpy as np
import pytest
import torch

import marex_amd
import marex_amd._stream as ms
from marex_amd.engine import HotPath
from marex_amd.exceptions import ConfigurationError, DataValidationError, ProcessingError, TrackingError
from marex_amd.xr_compat import DataArray

hs = sys.modules["marex_amd.heat_stress"]  # the package exports the function under the module's name

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import heat_stress_cases as hc  # noqa: E402
import heat_stress_oracle as ho  # noqa: E402
from heat_stress_host_engine import HostEngine  # noqa: E402

F = np.float32


def same_bytes(a, b, what=""):
    a, b = np.asarray(a), np.asarray(b)
    assert a.dtype == b.dtype and a.shape == b.shape, (what, a.dtype, b.dtype, a.shape, b.shape)
    if a.dtype.kind == "f":  # every NaN as one
        a, b = np.where(np.isnan(a), np.nan, a).astype(a.dtype), np.where(np.isnan(b), np.nan, b).astype(b.dtype)
    assert a.tobytes() == b.tobytes(), what


def run_walk(x, m, kw, B=None):
    """The row-loop oracle over the whole field in windows of ``B`` steps: ``(summary, dhw, alert)``."""
    T, C = x.shape
    W = kw.get("window", 84)
    dhw, alert, st = np.full((T, C), -7, F), np.full((T, C), 77, np.uint8), None
    for a in range(0, T, B or T):
        lead = min(W, a)
        st = ho.walk(x[a - lead:min(T, a + (B or T))], m, a, lead, dhw=dhw, alert=alert, state=st, **kw)
    return st, dhw, alert


@pytest.mark.parametrize("case", hc.columns(), ids=lambda c: c["name"])
def test_the_oracles_agree_on_the_hand_built_columns_and_with_the_hand(case):
    for x, m, at in ((case["x"][:, None], np.array([case["m"]], F), 0), (*hc.in_a_row(case), 37)):
        kw = case["kw"]
        st, dhw, alert = run_walk(x, m, kw)
        d = ho.direct(x, m, **kw)
        assert np.array_equal(dhw, d["dhw"], equal_nan=True) and np.array_equal(alert, d["alert"])
        for k in ho.SUMMARY:
            assert np.array_equal(st[k], d[k], equal_nan=True), k
        e = case["expect"]
        if "alert" in e:
            assert alert[:, at].tolist() == e["alert"]
        for t, v in e.get("dhw", {}).items():
            assert dhw[t, at] == F(v), (t, dhw[t, at], v)
        for k in ("dhw_max", "tmax", "hotspot_max", "invalid"):
            if k in e:
                assert st[k][0, at] == e[k], k
        if "onset" in e:
            assert st["onset"][0, :, at].tolist() == e["onset"]
        for B in (1, 2, 3):  # any cut into windows: the same bytes
            st2, dhw2, alert2 = run_walk(x, m, kw, B)
            same_bytes(dhw2, dhw), same_bytes(alert2, alert), same_bytes(st2["S"], st["S"])
            for k in ho.SUMMARY:
                same_bytes(st2[k], st[k], k)


def test_special_columns_by_hand():
    by = {c["name"]: c for c in hc.columns()}
    c = by["no_mmm"]
    st, dhw, alert = run_walk(c["x"][:, None], np.array([c["m"]], F), c["kw"])
    assert np.isnan(dhw).all() and (alert == 255).all() and st["invalid"][0, 0] == 4 and np.isnan(st["dhw_max"][0, 0])
    c = by["group_without_valid_step"]
    st, dhw, alert = run_walk(c["x"][:, None], np.array([c["m"]], F), c["kw"])
    # dhw = 2, 4, 2, 0, 2 at window 2: group 0 (steps 0, 1, 4) peaks at step 1, group 1 (steps 2, 3) still carries step 1's heat
    assert st["dhw_max"][:, 0].tolist()[:2] == [4.0, 2.0] and np.isnan(st["dhw_max"][2, 0]) and st["tmax"][:, 0].tolist() == [1, 2, -1]
    assert np.isnan(st["hotspot_max"][1, 0]) and st["invalid"][:, 0].tolist() == [0, 2, 0]
    assert st["alert_steps"][:, :, 0].sum(axis=1).tolist() == [3, 0, 0]


@pytest.mark.parametrize("window", [1, 2, 84, 366])
def test_the_running_sum_is_the_exact_sum_in_any_order(window):
    """Magnitudes over the whole allowed range [2^-10, 2^10): the carried sum, math.fsum and np.sum forwards and backwards
    agree in every step."""
    rng = np.random.default_rng(window)
    T = 2 * window + 40
    h = np.ldexp(rng.uniform(0.5, 1.0, T), rng.integers(-9, 11, T)).astype(F)  # [2^-10, 2^10)
    h[rng.random(T) < 0.3] = 0
    h[:4] = [F(1023.99), F(2.0 ** -10), np.nextafter(F(1024), F(0)), F(2.0 ** -10)]
    assert ((h == 0) | ((h >= F(2.0 ** -10)) & (h < 1024))).all()
    S = 0.0
    for t in range(T):
        S += float(h[t])
        if t >= window:
            S -= float(h[t - window])
        win = [float(v) for v in h[max(0, t - window + 1):t + 1]]
        assert S == math.fsum(win) == float(np.sum(np.array(win, np.float64))) == float(np.sum(np.array(win[::-1], np.float64)))
        assert S == sum(reversed(win))


def test_the_climatology_sums_have_an_order_and_the_counts_do_not():
    rng = np.random.default_rng(5)
    T, C = 60, 7
    x = (300.0 + rng.normal(0, 3, (T, C))).astype(F)
    x[rng.random((T, C)) < 0.1] = np.nan
    lab = rng.integers(-1, 12, T).astype(np.int32)
    lab[lab == 4] = 3  # month 5 has no sample
    st = ho.group_walk(x, 0, lab, 12)
    assert np.array_equal(st["cnt"], ho.group_direct_counts(x, lab, 12)) and not st["cnt"][4].any()
    st2 = None
    for a in range(0, T, 7):
        st2 = ho.group_walk(x[a:a + 7], a, lab, 12, st2)
    same_bytes(st2["sum"], st["sum"]), same_bytes(st2["cnt"], st["cnt"])
    mean, mmm, month = ho.climatology(st["sum"], st["cnt"])
    mean2, mmm2, month2 = hs.climatology_of(st["sum"], st["cnt"])
    same_bytes(mean, mean2), same_bytes(mmm, mmm2), same_bytes(month, month2)
    assert np.isnan(mean[4]).all() and (month != 5).all() and month.min() >= 1
    # two months with the same mean: the first; no sample at all: NaN and month 0
    total, cnt = np.array([[2.0, 0.0], [6.0, 0.0], [6.0, 0.0]]), np.array([[1, 0], [2, 0], [2, 0]], np.uint32)
    for f in (ho.climatology, hs.climatology_of):
        mean, mmm, month = f(total, cnt)
        assert mmm[0] == 3.0 and month.tolist() == [2, 0] and np.isnan(mmm[1]) and np.isnan(mean[:, 1]).all()


def _no_gpu(monkeypatch):
    import marex_amd.detect as det

    def no_gpu(*a, **k):
        raise AssertionError("the validation touched the GPU engine")

    monkeypatch.setattr(det, "get_engine", no_gpu)


def _dated(T, C=4, start="2000-01-01", shape=None):
    tv = np.datetime64(start) + np.arange(T).astype("timedelta64[D]")
    rng = np.random.default_rng(T)
    x, _ = hc.field(T, int(np.prod(shape)) if shape else C, rng)
    if shape:
        return DataArray(x.reshape((T,) + shape), dims=("time", "lat", "lon"), coords={"time": ("time", tv)})
    return DataArray(x, dims=("time", "cells"), coords={"time": ("time", tv)})


def test_refusals_come_before_the_device(monkeypatch):
    _no_gpu(monkeypatch)
    x = _dated(40, shape=(2, 2))
    raw = np.asarray(x.values)
    m = np.full((2, 2), 28.0, F)
    V, Cf = DataValidationError, ConfigurationError
    cases = [(dict(window=0), Cf, "window must be an integer in 1 .. 366"), (dict(window=367), Cf, "window must be"),
             (dict(window=7.0), Cf, "window must be"), (dict(window=True), Cf, "window must be"),
             (dict(hotspot_min=2.0 ** -11), Cf, "hotspot_min must satisfy 2\\^-10 <= hotspot_min < 1024"),
             (dict(hotspot_min=1024.0), Cf, "hotspot_min must satisfy"), (dict(hotspot_min=np.nan), Cf, "hotspot_min must satisfy"),
             (dict(hotspot_min=-1.0), Cf, "hotspot_min must satisfy"),
             (dict(levels=(8.0, 4.0)), Cf, "levels must be 0 .. 6 finite float32 values, strictly increasing"),
             (dict(levels=(4.0, 4.0)), Cf, "levels must be"), (dict(levels=tuple(range(7))), Cf, "levels must be"),
             (dict(levels=(4.0, np.inf)), Cf, "levels must be"),
             (dict(steps_per_week=0), Cf, "steps_per_week must be a finite number above 0"),
             (dict(steps_per_week=np.inf), Cf, "steps_per_week must be"), (dict(steps_per_week=-7), Cf, "steps_per_week must be"),
             (dict(sst=raw, mmm=None), Cf, "needs a datetime time coordinate or months="),
             (dict(mmm=None, baseline=(1950, 1960)), V, "baseline selects no timestep"),
             (dict(mmm=None, baseline=np.zeros(40, bool)), V, "baseline selects no timestep"),
             (dict(mmm=None, baseline=(2001, 2000)), Cf, "must be ascending"), (dict(mmm=None, baseline="2000"), Cf, "baseline must be"),
             (dict(sst=raw, mmm=None, months=np.zeros(40, np.int64)), V, "months must hold 1 .. 12"),
             (dict(sst=raw, mmm=None, months=np.ones(39, np.int64)), V, "months must be one integer per timestep"),
             (dict(sst=raw, mmm=None, months=np.ones(40, np.int64), baseline=(2000, 2000)), V, "datetime"),
             (dict(mmm=np.zeros((2, 3), F)), V, "mmm does not match the spatial shape of the field"),
             (dict(mmm=np.zeros(5, F)), V, "mmm does not match"), (dict(mmm=np.zeros((2, 2), np.int32)), V, "mmm must be a floating-point map"),
             (dict(sst=np.zeros(raw.shape, np.int32)), V, "sst must be a floating-point field"), (dict(sst=raw > 28), V, "sst must be a floating-point"),
             (dict(sst=torch.zeros((3, 4), dtype=torch.int64), mmm=np.zeros(4, F)), V, "sst must be a floating-point"),
             (dict(sst=raw[0, 0]), V, "field must be"), (dict(by="week"), Cf, "by must be"), (dict(sst=raw, by="year"), V, "datetime"),
             (dict(block_steps=0), Cf, "block_steps")]
    for kw, err, msg in cases:
        with pytest.raises(err, match=msg):
            marex_amd.heat_stress(**{"sst": x, "mmm": m, **kw})
    for kw, err, msg in [(dict(sst=raw), Cf, "needs a datetime time coordinate or months="), (dict(sst=raw > 0), V, "sst must be a floating"),
                         (dict(baseline=(1900, 1901)), V, "baseline selects no timestep"), (dict(block_steps="big"), Cf, "block_steps")]:
        with pytest.raises(err, match=msg):
            marex_amd.monthly_maximum_climatology(**{"sst": x, **kw})
    # empty fields: the empty Dataset, without a device
    ds = marex_amd.heat_stress(np.zeros((0, 3), F), np.zeros(3, F), return_dhw=True, return_alert=True)
    assert ds["dhw_max"].shape == (3,) and np.isnan(ds["dhw_max"].values).all() and ds["dhw"].shape == (0, 3)
    assert ds["alert_steps"].shape == (5, 3) and ds["level_onset"].shape == (2, 3) and ds.attrs["warmup_steps"] == 83
    ds = marex_amd.heat_stress(np.zeros((4, 0), F), np.zeros(0, F), by=np.array([0, 0, 1, 1]))
    assert ds["dhw_max"].shape == (2, 0)
    ds = marex_amd.monthly_maximum_climatology(np.zeros((0, 3), F), months=np.zeros(0, np.int64))
    assert ds["monthly_mean"].shape == (12, 3) and ds["mmm_month"].values.tolist() == [0, 0, 0]


@pytest.fixture
def host_engine(monkeypatch):
    import marex_amd.detect as det

    eng = HostEngine()
    monkeypatch.setattr(det, "get_engine", lambda device=0: eng)
    monkeypatch.setattr(ms, "_free_bytes", lambda e: 1 << 30)
    return eng


def test_the_dataset_through_the_stand_in(host_engine):
    T = 800
    x = _dated(T, shape=(2, 3), start="2001-06-01")
    flat = np.asarray(x.values).reshape(T, 6)
    ds = marex_amd.heat_stress(x, baseline=(2001, 2002), by="year", return_dhw=True, return_alert=True, window=30, levels=(1.0, 2.0, 4.0))
    assert list(ds.data_vars) == ["dhw_max", "time_of_dhw_max", "hotspot_max", "alert_steps", "invalid_steps", "level_onset", "mmm",
                                  "dhw", "alert_level"]
    assert ds.attrs == {"warmup_steps": 29, "window": 30, "steps_per_week": 7.0, "hotspot_min": 1.0}
    assert ds["dhw_max"].dims == ("year", "lat", "lon") and ds["dhw_max"].shape == (3, 2, 3) and ds["dhw_max"].dtype == F
    assert ds["alert_steps"].dims == ("year", "alert_class", "lat", "lon") and ds["alert_steps"].shape == (3, 6, 2, 3)
    assert ds["level_onset"].dims == ("year", "level", "lat", "lon") and ds["level_onset"].coords["level"].values.tolist() == [1.0, 2.0, 4.0]
    assert ds["dhw_max"].coords["year"].values.tolist() == [2001, 2002, 2003] and ds["mmm"].dims == ("lat", "lon")
    assert ds["dhw"].dims == ("time", "lat", "lon") and ds["dhw"].dtype == F and ds["alert_level"].dtype == np.uint8
    assert ds["time_of_dhw_max"].dtype == np.int32 and ds["alert_steps"].dtype == np.uint32 and ds["level_onset"].dtype == np.int32
    assert isinstance(ds["dhw"].values, np.ndarray) and np.array_equal(ds["dhw"].coords["time"].values, x.coords["time"].values)
    # against the oracles, with the climatology restated
    tv = x.coords["time"].values
    year = tv.astype("datetime64[Y]").astype(int) + 1970
    lab = np.where(year <= 2002, tv.astype("datetime64[M]").astype(int) % 12, -1).astype(np.int32)
    cst = ho.group_walk(flat, 0, lab, 12)
    m = ho.climatology(cst["sum"], cst["cnt"])[1]
    same_bytes(ds["mmm"].values.reshape(-1), m)
    d = ho.direct(flat, m, window=30, lev=(1.0, 2.0, 4.0), grp=year - 2001, G=3)
    for name, k in (("dhw_max", "dhw_max"), ("time_of_dhw_max", "tmax"), ("hotspot_max", "hotspot_max"), ("alert_steps", "alert_steps"),
                    ("invalid_steps", "invalid"), ("level_onset", "onset"), ("dhw", "dhw"), ("alert_level", "alert")):
        same_bytes(ds[name].values.reshape(d[k].shape), d[k], name)
    cl = marex_amd.monthly_maximum_climatology(x, baseline=(2001, 2002))
    assert list(cl.data_vars) == ["monthly_mean", "monthly_count", "mmm", "mmm_month"] and cl["monthly_mean"].dims == ("month", "lat", "lon")
    assert cl["monthly_count"].dtype == np.uint32 and cl["mmm_month"].dtype == np.uint8 and cl["monthly_mean"].dtype == np.float64
    assert cl["monthly_mean"].coords["month"].values.tolist() == list(range(1, 13)) and cl.attrs["baseline_steps"] == int((lab >= 0).sum())
    same_bytes(cl["mmm"].values.reshape(-1), m), same_bytes(cl["monthly_count"].values.reshape(12, 6), cst["cnt"])
    # a resident field gives resident fields; months= and a bool baseline stand in for the calendar
    t = torch.from_numpy(flat.copy())
    ds2 = marex_amd.heat_stress(t, months=lab % 12 + 1, baseline=lab >= 0, by=year - 2001, return_dhw=True, return_alert=True, window=30,
                                levels=(1.0, 2.0, 4.0))
    assert isinstance(ds2["dhw"].data, torch.Tensor) and ds2["dhw"].data.dtype == torch.float32 and ds2["alert_level"].data.dtype == torch.uint8
    same_bytes(ds2["dhw"].data.numpy(), d["dhw"]), same_bytes(ds2["alert_level"].data.numpy(), d["alert"])
    assert ds2["dhw_max"].dims == ("group", "cells")
    same_bytes(ds2["dhw_max"].values, d["dhw_max"])
    # a given mmm, a float64 field: read as float32
    ds3 = marex_amd.heat_stress(flat.astype(np.float64), m.astype(np.float64), window=30, levels=(1.0, 2.0, 4.0))
    d3 = ho.direct(flat, m, window=30, lev=(1.0, 2.0, 4.0))
    same_bytes(ds3["dhw_max"].values, d3["dhw_max"][0]), same_bytes(ds3["alert_steps"].values, d3["alert_steps"][0])
    assert ds3["dhw_max"].dims == ("cells",) and "dhw" not in ds3.data_vars


@pytest.mark.parametrize("window", [1, 5, 9])
def test_windows_of_every_length_give_the_same_bytes(host_engine, window):
    T = 23
    x = _dated(T, C=5)
    by = np.repeat(np.arange(6), 4)[:T]
    kw = dict(months=np.arange(T) % 12 + 1, baseline=np.arange(T) < 20, by=by, window=window, return_dhw=True, return_alert=True,
              hotspot_min=0.5, steps_per_week=2.5, levels=(0.5, 1.5))
    whole = marex_amd.heat_stress(x, **kw)
    assert [c for c in host_engine.calls if c[0] == "heat_stress"] == [("heat_stress", 0, 0, T)]
    for B in list(range(1, T + 1)) + ["auto"]:
        host_engine.calls.clear()
        part = marex_amd.heat_stress(x, block_steps=B, **kw)
        calls = [c for c in host_engine.calls if c[0] == "heat_stress"]
        if B != "auto":
            assert calls == [("heat_stress", a, min(window, a), min(B, T - a)) for a in range(0, T, B)]
            assert [c[1:] for c in host_engine.calls if c[0] == "group_mean"] == [(a, min(B, 20 - a)) for a in range(0, 20, B)]
        for k in whole.data_vars:
            same_bytes(part[k].values, whole[k].values, (k, B))


def test_window_planning_and_the_memory_refusal(monkeypatch):
    import marex_amd.detect as det

    T, C, W = 6, 5, 2
    x, m = np.ones((T, C), F), np.ones(C, F)
    fixed = 12 * C + hs.accumulator_bytes(1, C, 2) + 4 * T * C + W * 4 * C  # state and mmm, accumulators, dhw, history rows
    assert hs.accumulator_bytes(1, C, 2) == C * 44
    per_step = 4 * C
    free_auto = next(f for f in range(fixed, fixed + 400) if (f - f // 16 - fixed) // per_step == 4)
    for b, free, wins in [(None, fixed + T * per_step, [(0, 6)]), ("auto", free_auto, [(0, 4), (4, 2)]),
                          (5, fixed + per_step, [(0, 5), (5, 1)]), ("auto", fixed + per_step, [(t, 1) for t in range(6)])]:
        eng = HostEngine()
        monkeypatch.setattr(det, "get_engine", lambda device=0: eng)
        monkeypatch.setattr(ms, "_free_bytes", lambda e: free)
        marex_amd.heat_stress(x, m, window=W, return_dhw=True, block_steps=b)
        assert [(c[1], c[3]) for c in eng.calls] == wins, (b, eng.calls)
    monkeypatch.setattr(ms, "_free_bytes", lambda e: fixed + T * per_step - 1)
    with pytest.raises(TrackingError) as ei:
        marex_amd.heat_stress(x, m, window=W, return_dhw=True)
    e = ei.value
    assert e.message == "heat_stress: needs 0.000 GB of device memory, 0.000 GB are free"
    assert e.details == ("5 cells of 12 bytes (carried sum, mmm), 1 x 5 cells of accumulators, 44 bytes each, the dhw output of 6 x 5 x 4 "
                         "bytes, and the field of 6 timesteps and 2 of history, 4 bytes per cell, as far as it is not on the device already")
    assert e.suggestions == ["Pass block_steps='auto'", "Pass block_steps=<timesteps per window>", "Group by fewer labels", "Pass return_dhw=False"]
    # a resident float32 field costs nothing per step: the fixed part alone decides
    monkeypatch.setattr(ms, "_free_bytes", lambda e: fixed - W * per_step)
    eng = HostEngine()
    monkeypatch.setattr(det, "get_engine", lambda device=0: eng)
    marex_amd.heat_stress(torch.from_numpy(x), m, window=W, return_dhw=True)
    monkeypatch.setattr(ms, "_free_bytes", lambda e: 12 * 12 * C + 4 * T + T * per_step - 1)
    with pytest.raises(TrackingError, match="monthly_maximum_climatology: needs"):
        marex_amd.monthly_maximum_climatology(x, months=np.arange(T) % 12 + 1)


# ------------------------------------------------------------------ the engine calls against a recording stub
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
    log = []
    hot = HotPath.__new__(HotPath)
    hot.device = torch.device("cpu")
    hot.ctx, hot.lib = _Ctx(log), _Lib(log)
    hot._bind_stream = lambda: None
    hot._check_fits = lambda nbytes, what, details: log.append(("fits", nbytes))
    hot._dev = lambda a, dtype=None: torch.from_numpy(np.ascontiguousarray(a if dtype is None else a.astype(dtype)))
    return hot, log


def test_engine_calls_hand_the_library_what_the_header_declares():
    hot, log = _engine()
    C, T = 8, 10
    x = torch.zeros((4, C))
    lab = np.arange(T) % 3 - 1
    r = hot.group_mean(x, lab, 2, t0=3, finish=False)
    acc = r["acc"]
    name, args = [e for e in log if e[0] == "marex_group_mean_f32"][0]
    assert args == (hot.ctx.handle, x.data_ptr(), 3, 4, C, acc["tabs"]["lab"].data_ptr(), 2, acc["sum"].data_ptr(), acc["cnt"].data_ptr(),
                    acc["status"].data_ptr())
    assert acc["sum"].dtype == torch.float64 and tuple(acc["sum"].shape) == (2, C) and not acc["sum"].any() and ("fits", 12 * 2 * C + 8 + 4 * T) in log
    out = hot.group_mean(x, lab, 2, t0=6, acc=acc)  # t0 + Tb == T is within the labels
    assert out["sum"].shape == (2, C) and out["cnt"].dtype == np.uint32
    log.clear()
    xs = torch.zeros((2 + 3, C))  # two rows of history in front of three
    dhw, alert, m = torch.zeros((T, C)), torch.zeros((T, C), dtype=torch.uint8), np.ones(C, F)
    grp = np.arange(T) // 5
    first = hot.heat_stress(torch.zeros((2, C)), m, t0=0, lead=0, window=2, hotspot_min=0.5, steps_per_week=3.5, levels=(1.0, 2.0, 3.0),
                            grp=grp, G=2, dhw=dhw, alert=alert, finish=False)
    acc = first["acc"]
    out = hot.heat_stress(xs, m, t0=2, lead=2, window=2, hotspot_min=0.5, steps_per_week=3.5, levels=(1.0, 2.0, 3.0), grp=grp, G=2, dhw=dhw,
                          alert=alert, acc=acc)
    name, args = [e for e in log if e[0] == "marex_heat_stress_f32"][1]
    assert args == (hot.ctx.handle, xs.data_ptr(), acc["mmm"].data_ptr(), 2, 2, 3, C, 2, 0.5, 3.5, acc["levels"].data_ptr(), 3,
                    acc["tabs"]["grp"].data_ptr(), 2, acc["state"].data_ptr(), acc["dhw_max"].data_ptr(), acc["tmax"].data_ptr(),
                    acc["hotspot_max"].data_ptr(), acc["alert_steps"].data_ptr(), acc["invalid"].data_ptr(), acc["onset"].data_ptr(),
                    dhw.data_ptr(), alert.data_ptr(), acc["status"].data_ptr())
    assert tuple(acc["alert_steps"].shape) == (2, 6, C) and tuple(acc["onset"].shape) == (2, 3, C) and acc["state"].dtype == torch.float64
    assert ("fits", 8 * C + 2 * C * (16 + 24 + 12) + 8 + 4 * T) in log and acc["next"] == 5
    # the zeroed accumulators come back as "none"
    assert np.isnan(out["dhw_max"]).all() and (out["tmax"] == -1).all() and (out["onset"] == -1).all() and out["onset"].shape == (2, 3, C)
    assert out["alert_steps"].shape == (2, 6, C) and np.isnan(out["hotspot_max"]).all()
    # without a summary and without levels
    r = hot.heat_stress(torch.zeros((2, C)), m, levels=(), summary=False, dhw=dhw)
    assert set(r) == {"acc"} and r["acc"]["dhw_max"] is None and [e for e in log if e[0] == "marex_heat_stress_f32"][-1][1][15:21] == (None,) * 6


def test_engine_refusals():
    hot, log = _engine()
    C = 8
    x, m = torch.zeros((4, C)), np.ones(C, F)
    P = ProcessingError
    field = "the field must be a contiguous float32 \\[T, C\\] tensor on the engine's device"
    for bad in (x.to(torch.float64), x[:, ::2], x[0], x.numpy()):
        with pytest.raises(P, match="group_mean: " + field):
            hot.group_mean(bad, np.zeros(4, np.int64), 1)
        with pytest.raises(P, match="heat_stress: " + field):
            hot.heat_stress(bad, m)
    with pytest.raises(P, match="group_mean: t0 must not be negative, G must be positive"):
        hot.group_mean(x, np.zeros(4, np.int64), 0)
    with pytest.raises(P, match="group_mean: lab has 3 labels, the window ends at step 4"):
        hot.group_mean(x, np.zeros(3, np.int64), 1)
    with pytest.raises(P, match="group_mean: lab must be a vector of int32 values"):
        hot.group_mean(x, np.zeros(4), 1)
    acc = hot.group_mean(x, np.zeros(8, np.int64), 2, finish=False)["acc"]
    with pytest.raises(P, match="group_mean: the accumulators were planned for another call"):
        hot.group_mean(x, np.zeros(8, np.int64), 3, t0=4, acc=acc)
    for kw in (dict(window=0), dict(window=367), dict(window=2.0), dict(hotspot_min=2.0 ** -11), dict(hotspot_min=1024), dict(steps_per_week=0.0),
               dict(steps_per_week=np.inf), dict(levels=(2.0, 1.0)), dict(levels=tuple(range(7))), dict(levels=(np.nan,))):
        with pytest.raises(P, match="heat_stress: window must be an integer in 1 .. 366, hotspot_min in"):
            hot.heat_stress(x, m, **kw)
    for kw in (dict(t0=-1), dict(t0=3, lead=2), dict(t0=100, lead=3, window=84), dict(G=0), dict(G=2)):
        with pytest.raises(P, match="heat_stress: t0 must not be negative, lead must be min\\(window, t0\\)"):
            hot.heat_stress(x, m, **kw)
    with pytest.raises(P, match="heat_stress: mmm must be 8 float32 values"):
        hot.heat_stress(x, np.ones(7, F))
    with pytest.raises(P, match="heat_stress: mmm must be 8 float32 values"):
        hot.heat_stress(x, np.ones(C))
    with pytest.raises(P, match="heat_stress: mmm must be a contiguous float32 \\[8\\] tensor"):
        hot.heat_stress(x, torch.ones(C, dtype=torch.float64))
    with pytest.raises(P, match="heat_stress: the dhw output must be the whole contiguous float32 \\[T, 8\\] output .* T >= 4"):
        hot.heat_stress(x, m, dhw=torch.zeros((3, C)))
    with pytest.raises(P, match="heat_stress: the alert output must be the whole contiguous uint8 \\[T, 8\\] output"):
        hot.heat_stress(x, m, alert=torch.zeros((4, C)))
    with pytest.raises(P, match="heat_stress: grp has 3 labels, the window ends at step 4"):
        hot.heat_stress(x, m, grp=np.zeros(3, np.int64), G=1)
    with pytest.raises(P, match="heat_stress: an empty window"):
        hot.heat_stress(torch.zeros((2, C)), m, t0=2, lead=2, window=2)
    acc = hot.heat_stress(x, m, window=3, finish=False)["acc"]
    for kw in (dict(window=4, lead=4), dict(window=3, lead=3, levels=(4.0,)), dict(window=3, lead=3, hotspot_min=2.0),
               dict(window=3, lead=3, summary=False)):
        with pytest.raises(P, match="heat_stress: the accumulators were planned for another call"):
            hot.heat_stress(torch.zeros((8, C)), m, t0=4, acc=acc, **kw)
    with pytest.raises(P, match="heat_stress: the windows must follow each other"):
        hot.heat_stress(torch.zeros((5, C)), m, t0=5, lead=3, window=3, acc=acc)
    hot.heat_stress(torch.zeros((5, C)), m, t0=4, lead=3, window=3, acc=acc)
    assert not [e for e in log if e[0] == "marex_heat_stress_f32" and e[1][3] == 5]


def test_status_words_raise_with_the_counts():
    hot, _ = _engine()
    x, m = torch.zeros((4, 8)), np.ones(8, F)
    acc = hot.group_mean(x, np.zeros(4, np.int64), 1, finish=False)["acc"]
    acc["status"][0] = 16
    with pytest.raises(ProcessingError, match="group_mean: 16 cells lie under a step label outside its range") as ei:
        hot.group_mean(x, np.zeros(8, np.int64)[:8], 1, t0=0, acc=acc)
    assert ei.value.details == "lab must hold -1 .. 0; the cells were counted, nothing was written out of range"
    acc = hot.heat_stress(x, m, finish=False)["acc"]
    acc["status"][0] = 24
    with pytest.raises(ProcessingError, match="heat_stress: 24 cells lie under a step label outside its range") as ei:
        hot.heat_stress(torch.zeros((8, 8)), m, t0=4, lead=4, acc=acc)
    assert ei.value.details == "grp must hold 0 .. 0; the cells were counted, nothing was written out of range"


def test_the_package_exports_the_functions():
    assert "heat_stress" in marex_amd.__all__ and "monthly_maximum_climatology" in marex_amd.__all__
    assert marex_amd.heat_stress is hs.heat_stress
    from marex_amd import _lib

    assert {"marex_group_mean_f32", "marex_heat_stress_f32"} <= set(_lib.PROTOTYPES)
