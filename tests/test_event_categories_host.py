"""Severity categories of tracked events on the host: the oracle against hand-computed values, the float32 product rule,
unusable thresholds, a leap day, the three threshold layouts, the validation errors (raised before any device work), the
public path -- windows, slots, host finish -- on a NumPy stand-in for the two engine calls, and the tracker's method.  No
GPU needed."""
import importlib
import os
import sys

import numpy as np
import pytest

import marex_amd
import marex_amd._stream as ms
from marex_amd import _lib
from marex_amd.engine import HotPath
from marex_amd.exceptions import ConfigurationError, DataValidationError, ProcessingError, TrackingError
from marex_amd.xr_compat import DataArray

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import event_categories_oracle as co  # noqa: E402
from event_categories_cases import N_EV, public_case, spans, weights  # noqa: E402
from event_categories_host_engine import HostEngine  # noqa: E402

mc = importlib.import_module("marex_amd.event_categories")  # the package attribute of that name is the function
F = np.float32
NAN = np.nan
IDS = np.array([[1, 1, 0, 2, 2, 0],
                [1, 0, 0, 2, 2, 2],
                [0, 0, 0, 2, 0, 0]], np.int32)
THR = np.array([[1, 1, 1, 2, 2, 1],
                [2, 1, 1, 1, NAN, 0.5]], F)
DOY = np.array([0, 1, 0], np.int32)
ANOM = np.array([[0.5, 2.0, 9.0, 4.0, 8.5, 9.0],
                 [6.0, 9.0, 9.0, NAN, 1.0, 1.6],
                 [9.0, 9.0, 9.0, 1.0, 9.0, 9.0]], F)
W = np.array([1, 2, 1, 1, 2, 4], F)


def test_oracle_on_a_hand_computed_field():
    r = co.categories(IDS, ANOM, THR, DOY, W)
    assert r["category_field"].tolist() == [[1, 3, 0, 3, 5, 0], [4, 0, 0, 7, 6, 4], [0, 0, 0, 1, 0, 0]]
    assert r["category_peak"].tolist() == [[2, 4], [3, 3], [0, 0]] and r["category_peak"].dtype == np.uint8
    assert r["category_cells"][0].tolist() == [[1, 0, 1, 0, 0, 0], [0, 0, 1, 0, 1, 0]]
    assert r["category_cells"][1].tolist() == [[0, 0, 0, 1, 0, 0], [0, 0, 0, 1, 0, 1]]
    assert r["slot_cells"][1, 1, 6] == 1 and r["slot_cells"][..., 6].sum() == 1
    assert r["event_category"].tolist() == [3, 4] and r["event_step_of_category"].tolist() == [1, 0]
    assert r["event_category_cell_steps"].tolist() == [[1, 0, 1, 1, 0, 0], [1, 0, 1, 1, 1, 1]]
    assert r["event_category_area"].tolist() == [[1, 0, 2, 1, 0, 0], [1, 0, 1, 4, 2, 2]]
    assert r["event_category_steps"].tolist() == [[0, 0, 1, 1, 0, 0], [1, 0, 0, 1, 1, 0]]
    assert r["event_invalid_cells"].tolist() == [0, 1] and r["event_duration"].tolist() == [2, 3]
    assert co.categories(IDS, ANOM, THR, DOY)["event_category_area"].tolist() == r["event_category_cell_steps"].tolist()
    # a step with nothing but a non-finite anomaly: present, peak 5, no category
    r = co.categories(np.array([[1], [1]], np.int32), np.array([[NAN], [0.5]], F), np.ones((1, 1), F), [0, 0])
    assert r["event_category_steps"].tolist() == [[1, 0, 0, 0, 0, 1]] and r["event_category"].tolist() == [0]
    assert r["event_step_of_category"].tolist() == [-1] and r["category_field"].tolist() == [[7], [1]]
    # lost cells: a span declared too short, a doy label out of range
    r = co.categories(IDS, ANOM, THR, [0, 2, 0], spans=([0, 0, 0], [0, 1, 1]))
    assert r["status"] == [1, 4] and r["category_field"][1:].tolist() == [[0] * 6, [0] * 6]
    assert r["event_duration"].tolist() == [1, 1]


def test_the_products_are_float32_with_one_rounding_each():
    h = F(0.1)
    a = F(3) * h
    below = np.nextafter(a, F(0))
    assert co.classify(np.array([a, below]), np.array([h, h])).tolist() == [3, 2]  # severe, and strong just below
    # where the float32 product rounds DOWN the float64 product would call the same value strong: 3 x 0.7
    h = F(0.7)
    a = F(3) * h
    assert float(a) < 3.0 * float(h) and co.classify(np.array([a]), np.array([h])).tolist() == [3]
    # where it rounds UP the float64 product would call the float32 value between the two severe: 3 x 0.1 in float64
    # terms lies under a, so no float32 value separates them; the rule is the float32 one either way
    for hv in (0.1, 0.2, 0.3, 0.7, 0.9, 1.1, 1.3):
        for k in (1, 2, 3, 4):
            h = F(hv)
            a = F(k) * h
            got = co.classify(np.array([a, np.nextafter(a, F(0))]), np.array([h, h])).tolist()
            assert got == [k, k - 1], (hv, k)


def test_unusable_thresholds_and_anomalies():
    a = np.array([1, 1, 1, 1, -1, 1, NAN, np.inf, -np.inf, NAN], F)
    h = np.array([NAN, np.inf, 0, -2, -2, -np.inf, 1, 1, 1, NAN], F)
    assert co.classify(a, h).tolist() == [5, 5, 5, 5, 5, 5, 6, 6, 6, 6]
    assert co.classify(np.array([-5, 0, 0.999, 1, 8, 1e30], F), np.ones(6, F)).tolist() == [0, 0, 0, 1, 4, 4]
    big = F(3e38)  # 2 h overflows to +inf: nothing finite reaches it
    assert co.classify(np.array([3.3e38], F), np.array([big])).tolist() == [1]
    assert mc.step_peak(np.array([[0, 0, 0, 0, 0, 3, 0], [2, 0, 0, 0, 0, 3, 0], [2, 1, 0, 1, 0, 0, 9], [0, 0, 0, 0, 0, 0, 4]])).tolist() == \
        [5, 0, 3, 5]
    assert mc.CATEGORIES == co.CATEGORIES


def test_abi_and_public_names():
    assert "marex_event_categories_f32" in _lib.PROTOTYPES and len(_lib.PROTOTYPES["marex_event_categories_f32"][1]) == 18
    assert "event_categories" in marex_amd.__all__ and marex_amd.event_categories is mc.event_categories
    assert hasattr(marex_amd.tracker, "event_categories") and hasattr(HotPath, "event_categories")
    assert mc.SLOT_BYTES == 7 * 8 + 6 * 8
    header = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "marex_hip.h")).read()
    assert "int marex_event_categories_f32(marex_ctx* ctx, const int32_t* ids, const float* anom, int64_t t0" in header


def _no_gpu(monkeypatch):
    import marex_amd.detect as det

    def no_gpu(*a, **k):
        raise AssertionError("the validation touched the GPU engine")

    monkeypatch.setattr(det, "get_engine", no_gpu)


def _da(a, tv=None, dims=("time", "lat", "lon")):
    return DataArray(a, dims=dims, coords={dims[0]: (dims[0], np.arange(a.shape[0]) if tv is None else tv)})


def _days(start, T):
    return (np.datetime64(start, "D") + np.arange(T)).astype("datetime64[ns]")


def test_validation_errors_come_before_the_device(monkeypatch):
    _no_gpu(monkeypatch)
    ids = np.zeros((3, 4, 5), np.int32)
    an = np.zeros((3, 4, 5), F)
    th = np.ones((4, 5), F)
    tv = _days("2020-01-01", 3)
    cases = [
        (dict(dat_anomaly=an[:, :, :4]), DataValidationError, "ID_field and dat_anomaly differ in shape"),
        (dict(ID_field=_da(ids), dat_anomaly=_da(an, np.arange(3) + 1)), DataValidationError,
         "ID_field and dat_anomaly differ in their time coordinate"),
        (dict(ID_field=ids[0, 0], dat_anomaly=an[0, 0]), DataValidationError, r"ID_field must be \(time, y, x\) or \(time, cells\)"),
        (dict(ID_field=ids.astype(F)), DataValidationError, "Object IDs must be integers"),
        (dict(ID_field=ids > 0), DataValidationError, "Object IDs must be integers"),
        (dict(dat_anomaly=ids), DataValidationError, "dat_anomaly must be a floating-point field"),
        (dict(cell_areas=-np.ones((4, 5), F)), DataValidationError, "cell_areas must be finite and non-negative"),
        (dict(cell_areas=np.ones(5, F)), DataValidationError, "cell_areas do not match the spatial shape of ID_field"),
        (dict(thresholds=np.ones((4, 5), np.int32)), DataValidationError, "thresholds must be a floating-point field"),
        (dict(thresholds=np.ones((5, 4), F)), DataValidationError, "thresholds do not match the spatial shape of the field"),
        (dict(thresholds=np.ones((4, 5, 365), F)), DataValidationError, "thresholds do not match the spatial shape"),
        (dict(thresholds=np.ones((3, 4, 5), F)), DataValidationError, "thresholds do not match the spatial shape"),
        (dict(ID_field=_da(ids), thresholds=DataArray(np.ones((5, 4), F), dims=("lon", "lat"))), DataValidationError,
         "field and thresholds differ in their dimensions"),
        (dict(ID_field=_da(ids, tv), thresholds=DataArray(np.ones((4, 366, 5), F), dims=("lat", "dayofyear", "lon"))),
         DataValidationError, "thresholds do not match the spatial shape"),
        # thresholds by dayofyear need dates: an integer axis, no axis at all, NaT
        (dict(ID_field=_da(ids), thresholds=np.ones((4, 5, 366), F)), DataValidationError,
         "thresholds by dayofyear needs a datetime time coordinate"),
        (dict(thresholds=np.ones((366, 4, 5), F)), DataValidationError, "thresholds by dayofyear needs a datetime time coordinate"),
        (dict(ID_field=_da(ids, np.array(["2020-01-01", "NaT", "2020-01-03"], "datetime64[ns]")),
              thresholds=np.ones((366, 4, 5), F)), DataValidationError, "the time coordinate holds NaT"),
    ]
    cases += [(dict(block_steps=b), ConfigurationError, "block_steps must be a positive number of timesteps, 'auto' or None")
              for b in (0, -2, 2.5, True, "all")]
    for kw, cls, msg in cases:
        args = dict(ID_field=ids, dat_anomaly=an, thresholds=th)
        args.update(kw)
        with pytest.raises(cls, match=msg):
            marex_amd.event_categories(**args)
    # empty fields need no device either
    ds = marex_amd.event_categories(ids[:0], an[:0], th, per_timestep=True, return_field=True)
    assert ds["ID"].values.size == 0 and np.asarray(ds["category_cells"].values).shape == (0, 0, 6)
    assert np.asarray(ds["category_field"].values).shape == (0, 4, 5) and np.asarray(ds["category_field"].values).dtype == np.uint8


VARS_T = ["category_peak", "category_cells", "category_area"]
VARS_E = ["event_category", "event_time_of_category", "event_category_cell_steps", "event_category_area", "event_category_steps",
          "event_invalid_cells"]
DTYPES = {"category_peak": np.uint8, "category_cells": np.uint32, "category_area": np.float64, "event_category": np.uint8,
          "event_category_cell_steps": np.int64, "event_category_area": np.float64, "event_category_steps": np.int32,
          "event_invalid_cells": np.int64, "category_field": np.uint8}


def assert_equals_oracle(ds, exp, tv, per_timestep=False, weighted=False, field=False):
    want = ([v for v in VARS_T if weighted or v != "category_area"] if per_timestep else []) + VARS_E + \
        (["category_field"] if field else [])
    assert list(ds.data_vars) == want
    for k, dt in DTYPES.items():
        if k in ds.data_vars:
            got = np.asarray(ds[k].values).reshape(exp[k].shape)
            assert got.dtype == dt, (k, got.dtype)
            assert got.tobytes() == exp[k].astype(dt).tobytes(), k  # bit for bit, the float64 areas too
    step = exp["event_step_of_category"]
    toc = np.asarray(ds["event_time_of_category"].values)
    assert np.array_equal(toc[step >= 0], np.asarray(tv)[step[step >= 0]])
    assert all(v != v for v in toc[step < 0])  # NaN / NaT
    N = exp["event_category"].size
    assert np.array_equal(ds["ID"].values, np.arange(1, N + 1, dtype=np.int32)) and ds["ID"].values.dtype == np.int32
    assert list(ds["category"].values) == list(co.CATEGORIES)
    assert tuple(ds["event_category_steps"].dims) == ("ID", "category")
    assert np.array_equal(np.asarray(ds["event_category_steps"].values).sum(axis=1), exp["event_duration"])


@pytest.fixture
def host_engine(monkeypatch):
    import marex_amd.detect as det

    eng = HostEngine()
    monkeypatch.setattr(det, "get_engine", lambda device=0: eng)
    monkeypatch.setattr(ms, "_free_bytes", lambda e: 1 << 30)
    return eng


def _calendar_case(T=7, ny=21, nx=33, start="2020-02-26"):
    """The seeded case on dates that cross a leap day, its three threshold rows spread over the 366 of the year: every
    other row would put every cell into another class."""
    ids, anom, thr, doy = public_case(T, ny * nx)
    tv = _days(start, T)
    day = (tv.astype("datetime64[D]") - tv.astype("datetime64[Y]").astype("datetime64[D]")).astype(np.int64)
    assert day.tolist() == [56, 57, 58, 59, 60, 61, 62]
    thr366 = np.full((366, ny * nx), 1000.0, F)
    for t in range(T):
        thr366[day[t]] = thr[doy[t]]
    return ids, anom, thr, doy, thr366, tv


@pytest.mark.parametrize("weighted", [False, True], ids=["cells", "areas"])
def test_public_path_on_the_host_engine(host_engine, weighted):
    T, ny, nx = 7, 21, 33
    C = ny * nx
    ids, anom, thr, doy, thr366, tv = _calendar_case(T, ny, nx)
    w = weights(C) if weighted else None
    exp = co.categories(ids, anom, thr, doy, w, N_EV)
    assert set(np.unique(exp["category_field"])) == set(range(8)) and (exp["event_category"] == 4).any()
    da_i, da_a = _da(ids.reshape(T, ny, nx), tv), _da(anom.reshape(T, ny, nx), tv)
    th = thr366.reshape(366, ny, nx)
    area = None if w is None else w.reshape(ny, nx)
    whole = marex_amd.event_categories(da_i, da_a, th, area, per_timestep=True, return_field=True)
    assert_equals_oracle(whole, exp, tv, True, weighted, True)
    assert tuple(whole["category_cells"].dims) == ("time", "ID", "category") and np.array_equal(whole["time"].values, tv)
    assert tuple(whole["category_field"].dims) == ("time", "lat", "lon") and isinstance(whole["category_field"].values, np.ndarray)
    assert host_engine.calls == [("id_spans", T), ("event_categories", 0, T)]
    for b in (1, 2, 5, "auto"):  # the block length changes nothing
        host_engine.calls.clear()
        ds = marex_amd.event_categories(da_i, da_a, th, area, per_timestep=True, return_field=True, block_steps=b)
        for k in whole.data_vars:
            assert np.asarray(ds[k].values).tobytes() == np.asarray(whole[k].values).tobytes(), (b, k)
        if b == 5:
            assert host_engine.calls == [("id_spans", 5), ("id_spans", 2), ("event_categories", 0, 5), ("event_categories", 5, 2)]
    default = marex_amd.event_categories(da_i, da_a, th, area)
    assert_equals_oracle(default, exp, tv, False, weighted, False)


def test_the_three_threshold_layouts_by_name_and_by_shape(host_engine):
    import torch

    T, ny, nx = 7, 21, 33
    C = ny * nx
    ids, anom, thr, doy, thr366, tv = _calendar_case(T, ny, nx)
    exp = co.categories(ids, anom, thr, doy, None, N_EV)
    da_i, da_a = _da(ids.reshape(T, ny, nx), tv), _da(anom.reshape(T, ny, nx), tv)
    first = thr366.reshape(366, ny, nx)
    last = np.ascontiguousarray(first.transpose(1, 2, 0))
    for th in (first, last, DataArray(first, dims=("dayofyear", "lat", "lon")), DataArray(last, dims=("lat", "lon", "dayofyear")),
               torch.from_numpy(last), first.astype(np.float64)):
        assert_equals_oracle(marex_amd.event_categories(da_i, da_a, th), exp, tv)
    # a mesh: (time, cells) with (cells, dayofyear) and (dayofyear, cells)
    mi, ma = _da(ids, tv, ("time", "ncells")), _da(anom, tv, ("time", "ncells"))
    for th in (thr366, np.ascontiguousarray(thr366.T), DataArray(thr366, dims=("dayofyear", "ncells"))):
        assert_equals_oracle(marex_amd.event_categories(mi, ma, th, block_steps=2), exp, tv)
    # one threshold per cell (global_extreme), float64 rounded to float32; no dates needed
    g64 = thr[0].astype(np.float64) * (1 + 2.0 ** -40)
    assert (g64 != thr[0]).any() and np.array_equal(g64.astype(F), thr[0], equal_nan=True)
    exp = co.categories(ids, anom, thr[:1], np.zeros(T, np.int32), None, N_EV)
    for th in (g64.reshape(ny, nx), DataArray(thr[0].reshape(ny, nx), dims=("lat", "lon"))):
        ds = marex_amd.event_categories(ids.reshape(T, ny, nx), torch.from_numpy(anom.astype(np.float64).reshape(T, ny, nx)), th)
        assert_equals_oracle(ds, exp, np.arange(T))
    assert all(v != v for v in np.asarray(ds["event_time_of_category"].values)[exp["event_category"] == 0])


def test_a_leap_day_takes_the_row_of_its_day_of_the_year(host_engine):
    tv = np.array(["2020-02-28", "2020-02-29", "2020-03-01", "2021-02-28", "2021-03-01"], "datetime64[D]").astype("datetime64[ns]")
    th = np.full((366, 2), 1000.0, F)
    th[58], th[59], th[60] = 1.0, 2.0, 4.0
    ids = np.ones((5, 2), np.int32)
    anom = np.full((5, 2), 2.5, F)
    ds = marex_amd.event_categories(_da(ids, tv, ("time", "cells")), _da(anom, tv, ("time", "cells")), th, per_timestep=True,
                                    return_field=True)
    # 28 Feb: row 58; 29 Feb 2020: row 59; 1 Mar 2020: row 60; 1 Mar 2021: row 59 -- dayofyear - 1, as preprocess_data compares
    assert np.asarray(ds["category_peak"].values)[:, 0].tolist() == [2, 1, 0, 2, 1]
    assert np.asarray(ds["category_field"].values)[:, 0].tolist() == [3, 2, 1, 3, 2]
    assert np.asarray(ds["event_category"].values).tolist() == [2] and ds["event_time_of_category"].values[0] == tv[0]
    assert np.asarray(ds["event_category_steps"].values).tolist() == [[1, 2, 2, 0, 0, 0]]


def test_no_event_trailing_ids_and_the_memory_check(host_engine, monkeypatch):
    T, C = 7, 693
    ids, anom, thr, doy = public_case(T, C)
    g = thr[0]
    none = marex_amd.event_categories(np.zeros((T, C), np.int32), anom, g, per_timestep=True, return_field=True)
    assert none["ID"].values.size == 0 and np.asarray(none["category_cells"].values).shape == (T, 0, 6)
    assert np.asarray(none["event_category_steps"].values).shape == (0, 6) and not np.asarray(none["category_field"].values).any()
    assert np.asarray(none["category_field"].values).shape == (T, C)
    # the tracker's Dataset may end in events without a cell: they are absent everywhere
    ds = mc._event_categories(ids, anom, g, None, True, False, None, 0, n_events=N_EV + 2)
    exp = co.categories(ids, anom, thr[:1], np.zeros(T, np.int32), None, N_EV + 2)
    assert_equals_oracle(ds, exp, np.arange(T), True)
    assert exp["event_category_steps"][-2:].sum() == 0
    with pytest.raises(ProcessingError, match="the ID field holds event 6, the events Dataset ends at 5"):
        mc._event_categories(ids, anom, g, None, False, False, None, 0, n_events=5)
    # the figures of the memory check: thresholds, slots, the field, the windows
    monkeypatch.setattr(ms, "_free_bytes", lambda e: 4 * C + 8 * C + T * C - 1)
    with pytest.raises(TrackingError, match=r"event_categories: needs .* GB of device memory, .* GB are free") as ei:
        marex_amd.event_categories(ids, anom, g, return_field=True, block_steps=1)
    assert f"the category field of {T} x {C} bytes" in str(ei.value.details) and "104 bytes" in str(ei.value.details)
    slots = int(HotPath.event_slot_plan(*spans(ids))[-1])
    monkeypatch.setattr(ms, "_free_bytes", lambda e: 4 * C + 8 * C + 104 * slots - 1)  # fits until the slots are known
    with pytest.raises(TrackingError, match=r"event_categories: needs") as ei:
        marex_amd.event_categories(ids, anom, g, block_steps=1)
    assert f"{slots} (timestep, event) slots of 104 bytes" in str(ei.value.details)


def test_tracker_method_on_a_stand_in(host_engine):
    T, ny, nx = 7, 21, 33
    ids, anom, thr, doy, thr366, tv = _calendar_case(T, ny, nx)
    w = weights(ny * nx)

    class Trk:  # the attributes the method reads
        device, unstructured_grid, timedim, timecoord, time_values = 0, False, "time", "time", tv
        _cell_weights = w

    events = marex_amd.Dataset({"ID_field": DataArray(ids.reshape(T, ny, nx), dims=("time", "lat", "lon")),
                                "ID": DataArray(np.arange(1, N_EV + 2, dtype=np.int32), dims=("ID",))})
    events.attrs["N_events_final"] = N_EV + 1
    extremes = marex_amd.Dataset({"dat_anomaly": DataArray(anom.reshape(T, ny, nx), dims=("time", "lat", "lon")),
                                  "thresholds": DataArray(thr366.reshape(366, ny, nx), dims=("dayofyear", "lat", "lon"))})
    ds = marex_amd.tracker.event_categories(Trk(), events, extremes, per_timestep=True, block_steps=2)
    exp = co.categories(ids, anom, thr, doy, w, N_EV + 1)
    assert list(ds.data_vars)[:2] == ["ID_field", "ID"] and ds.attrs == events.attrs and "event_category" not in events.data_vars

    class View:
        data_vars = {k: ds[k] for k in VARS_T + VARS_E}

        def __getitem__(self, k):
            return ds[k]

    assert_equals_oracle(View(), exp, tv, True, True)
    # thresholds passed on their own win over those of extremes_ds; a mesh tracker weighs by its cell areas
    Trk.unstructured_grid, Trk.cell_area = True, np.ones(ny * nx)
    ev_m = marex_amd.Dataset({"ID_field": DataArray(ids, dims=("time", "ncells"))})
    ex_m = marex_amd.Dataset({"dat_anomaly": DataArray(anom, dims=("time", "ncells")), "thresholds": DataArray(np.zeros_like(thr366), dims=("dayofyear", "ncells"))})
    ds = marex_amd.tracker.event_categories(Trk(), ev_m, ex_m, thresholds=thr[0], return_field=True)
    exp = co.categories(ids, anom, thr[:1], np.zeros(T, np.int32), np.ones(ny * nx, F), N_EV)
    assert np.array_equal(np.asarray(ds["event_category_area"].values), exp["event_category_area"])
    assert np.array_equal(np.asarray(ds["category_field"].values), exp["category_field"])
    # the Dataset lists fewer events than the field holds
    short = marex_amd.Dataset({"ID_field": events["ID_field"], "ID": DataArray(np.arange(1, N_EV, dtype=np.int32), dims=("ID",))})
    Trk.unstructured_grid = False
    with pytest.raises(ProcessingError, match="the ID field holds event 6, the events Dataset ends at 5"):
        marex_amd.tracker.event_categories(Trk(), short, extremes)
