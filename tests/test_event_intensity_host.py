"""Per-event intensity metrics on the host: the oracle against hand-computed values, the float32 <-> key map, the slot plan,
the validation errors (raised before any device work) and the public path -- windows, slots, host finish -- on a NumPy
stand-in for the two engine calls.  No GPU needed."""
import os
import sys

import numpy as np
import pytest

import marex_amd
import marex_amd._stream as ms
import marex_amd.intensity as mi
from marex_amd.engine import HotPath, _key_to_float
from marex_amd.exceptions import ConfigurationError, DataValidationError
from marex_amd.xr_compat import DataArray

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import intensity_oracle as io  # noqa: E402
from intensity_cases import N_EV, public_field, spans, weights  # noqa: E402
from intensity_host_engine import HostEngine  # noqa: E402

NAN = np.nan
IDS = np.array([[1, 1, 0, 2, 2, 0, 0, 0],
                [1, 0, 0, 2, 2, 2, 0, 0],
                [0, 0, 0, 2, 0, 0, 0, 0]], np.int32)
ANOM = np.array([[1.0, 3.0, 9.0, 2.0, 0.5, 9.0, 9.0, 9.0],
                 [-1.5, 9.0, 9.0, 4.0, NAN, 1.0, 9.0, 9.0],
                 [9.0, 9.0, 9.0, 2.5, 9.0, 9.0, 9.0, 9.0]], np.float32)
W = np.array([1, 2, 1, 1, 2, 4, 1, 1], np.float32)


def test_oracle_on_a_hand_computed_field():
    r = io.intensity(IDS, ANOM)
    assert np.array_equal(r["intensity_cells"], [[2, 2], [1, 2], [0, 1]])
    assert np.array_equal(r["intensity_max"], np.array([[3, 2], [-1.5, 4], [NAN, 2.5]], np.float32), equal_nan=True)
    assert r["intensity_max"][1, 0] == np.float32(-1.5)  # an all-negative slot keeps its negative maximum, not 0
    assert np.array_equal(r["intensity_integral"], [[4, 2.5], [-1.5, 5], [NAN, 2.5]], equal_nan=True)
    assert np.array_equal(r["intensity_mean"], np.array([[2, 1.25], [-1.5, 2.5], [NAN, 2.5]], np.float32), equal_nan=True)
    assert r["event_duration"].tolist() == [2, 3] and r["event_duration"].dtype == np.int32
    assert r["event_intensity_max"].tolist() == [3.0, 4.0] and r["event_step_of_max"].tolist() == [0, 1]
    assert np.array_equal(r["event_intensity_mean"], np.array([2.5 / 3, 2.0], np.float32))
    assert r["event_intensity_cumulative"].tolist() == [0.5, 6.25]
    assert r["event_invalid_cells"].tolist() == [0, 1]
    rw = io.intensity(IDS, ANOM, W)
    assert rw["intensity_integral"][0].tolist() == [7.0, 3.0] and rw["intensity_mean"][0, 0] == np.float32(7 / 3)
    assert rw["intensity_integral"][1].tolist() == [-1.5, 8.0] and rw["intensity_cells"][1].tolist() == [1, 2]
    assert rw["event_intensity_mean"][1] == np.float32((3.0 + 8.0 + 2.5) / (3 + 5 + 1))
    # a slot with only non-finite cells: present for the duration, NaN everywhere else
    r = io.intensity(np.array([[1, 1], [1, 0]], np.int32), np.array([[NAN, np.inf], [2.0, 0.0]], np.float32))
    assert r["event_duration"].tolist() == [2] and r["intensity_cells"][:, 0].tolist() == [0, 1]
    assert np.isnan(r["intensity_max"][0, 0]) and np.isnan(r["intensity_integral"][0, 0]) and r["event_invalid_cells"].tolist() == [2]
    assert r["event_intensity_cumulative"].tolist() == [2.0] and r["event_step_of_max"].tolist() == [1]


def test_key_round_trip_and_order():
    tiny = np.float32(1e-45)  # the smallest denormal
    vals = np.array([-np.inf, -3.4e38, -2.5, -1.0, -1.2e-38, -tiny, -0.0, 0.0, tiny, 1.2e-38, 1.0, 2.5, 3.4e38, np.inf], np.float32)
    keys = mi.float_key(vals)
    assert keys.dtype == np.uint32 and (np.diff(keys.astype(np.int64)) > 0).all() and (keys > 0).all()
    back = mi.key_float(keys)
    assert back.dtype == np.float32 and back.view(np.uint32).tolist() == vals.view(np.uint32).tolist()  # the sign of zero too
    assert np.isnan(mi.key_float(np.zeros(1, np.uint32))[0])                                            # "no finite cell"
    assert np.isnan(mi.key_float(mi.float_key(np.array([np.nan], np.float32)))[0])
    for v, k in zip(vals.tolist(), keys.tolist()):  # the oracle's and the engine's own maps agree
        assert io.float_key(v) == k and io.key_float(k) == v and _key_to_float(k) == v


def test_slot_plan():
    tmin = np.array([0, 3, 2**31 - 1, 0, 5, 7], np.int64)
    tmax = np.array([9, 5, -1, 0, 4, 9], np.int64)  # entry 0 is unused whatever it holds; events 2 and 4 are absent
    off = HotPath.event_slot_plan(tmin, tmax)
    assert off.dtype == np.int64 and off.tolist() == [0, 0, 3, 3, 4, 4, 7]
    assert HotPath.event_slot_plan(tmin, tmax, 9).tolist() == [0, 0, 3, 3, 4, 4, 4]  # a span past the field: no slot
    assert HotPath.event_slot_plan([0, -1], [0, 3]).tolist() == [0, 0, 0]
    ids, _ = public_field(6, 693)
    lo, hi = spans(ids)
    want = np.concatenate([[0], np.cumsum(np.maximum(hi - lo + 1, 0) * (hi >= 0))])  # what the rename test expects of event_rename
    assert HotPath.event_slot_plan(lo, hi, 6).tolist() == want.tolist() == HotPath.event_slot_plan(lo, hi).tolist()


def _no_gpu(monkeypatch):
    import marex_amd.detect as det

    def no_gpu(*a, **k):
        raise AssertionError("the validation touched the GPU engine")

    monkeypatch.setattr(det, "get_engine", no_gpu)


def _da(a, tv=None, dims=("time", "lat", "lon")):
    return DataArray(a, dims=dims, coords={dims[0]: (dims[0], np.arange(a.shape[0]) if tv is None else tv)})


def test_validation_errors_come_before_the_device(monkeypatch):
    _no_gpu(monkeypatch)
    ids = np.zeros((3, 4, 5), np.int32)
    an = np.zeros((3, 4, 5), np.float32)
    cases = [
        (dict(dat_anomaly=an[:, :, :4]), DataValidationError, "ID_field and dat_anomaly differ in shape"),
        (dict(ID_field=_da(ids), dat_anomaly=_da(an, np.arange(3) + 1)), DataValidationError,
         "ID_field and dat_anomaly differ in their time coordinate"),
        (dict(ID_field=_da(ids), dat_anomaly=_da(an.transpose(0, 2, 1), dims=("time", "lon", "lat"))), DataValidationError,
         "ID_field and dat_anomaly differ in shape"),
        (dict(ID_field=ids[0, 0], dat_anomaly=an[0, 0]), DataValidationError, r"ID_field must be \(time, y, x\) or \(time, cells\)"),
        (dict(ID_field=ids.astype(np.float32)), DataValidationError, "Object IDs must be integers"),
        (dict(ID_field=ids > 0), DataValidationError, "Object IDs must be integers"),
        (dict(dat_anomaly=ids), DataValidationError, "dat_anomaly must be a floating-point field"),
        (dict(cell_areas=-np.ones((4, 5), np.float32)), DataValidationError, "cell_areas must be finite and non-negative"),
        (dict(cell_areas=np.full(20, np.nan, np.float32)), DataValidationError, "cell_areas must be finite and non-negative"),
        (dict(cell_areas=np.full(4, np.inf)), DataValidationError, "cell_areas must be finite and non-negative"),
        (dict(cell_areas=np.ones(5, np.float32)), DataValidationError, "cell_areas do not match the spatial shape of ID_field"),
        (dict(cell_areas=np.ones((5, 4), np.float32)), DataValidationError, "cell_areas do not match"),
        (dict(cell_areas=DataArray(np.ones(21, np.float32), dims=("cell",))), DataValidationError, "cell_areas do not match"),
    ]
    cases += [(dict(block_steps=b), ConfigurationError, "block_steps must be a positive number of timesteps, 'auto' or None")
              for b in (0, -2, 2.5, True, "all")]
    for kw, cls, msg in cases:
        args = dict(ID_field=ids, dat_anomaly=an)
        args.update(kw)
        with pytest.raises(cls, match=msg):
            marex_amd.event_intensity(**args)
    ids4 = np.zeros((3, 4, 4), np.int32)  # a square grid: only the names tell (time, x, y) from (time, y, x)
    with pytest.raises(DataValidationError, match="differ in their dimensions"):
        marex_amd.event_intensity(_da(ids4), _da(ids4.astype(np.float32), dims=("time", "lon", "lat")))


def test_event_intensity_is_public():
    assert "event_intensity" in marex_amd.__all__ and marex_amd.event_intensity is mi.event_intensity
    assert hasattr(marex_amd.tracker, "event_intensity") and hasattr(HotPath, "event_intensity")


VARS_T = ["intensity_max", "intensity_mean", "intensity_integral", "intensity_cells"]
VARS_E = ["event_duration", "event_intensity_max", "event_time_of_max", "event_intensity_mean", "event_intensity_cumulative",
          "event_invalid_cells"]
DTYPES = {"intensity_max": np.float32, "intensity_mean": np.float32, "intensity_integral": np.float64, "intensity_cells": np.int64,
          "event_duration": np.int32, "event_intensity_max": np.float32, "event_intensity_mean": np.float32,
          "event_intensity_cumulative": np.float32, "event_invalid_cells": np.int64}


def assert_equals_oracle(ds, exp, tv, per_timestep=True):
    assert list(ds.data_vars) == (VARS_T if per_timestep else []) + VARS_E
    for k, dt in DTYPES.items():
        if k in ds.data_vars:
            got = np.asarray(ds[k].values)
            assert got.dtype == dt and got.shape == exp[k].shape, (k, got.dtype, got.shape)
            assert np.array_equal(got, exp[k], equal_nan=got.dtype.kind == "f"), k
    step = exp["event_step_of_max"]
    tom = np.asarray(ds["event_time_of_max"].values)
    assert np.array_equal(tom[step >= 0], np.asarray(tv)[step[step >= 0]])
    assert all(v != v for v in tom[step < 0])  # NaN / NaT
    N = exp["event_duration"].size
    assert np.array_equal(ds["ID"].values, np.arange(1, N + 1, dtype=np.int32)) and ds["ID"].values.dtype == np.int32


@pytest.fixture
def host_engine(monkeypatch):
    import marex_amd.detect as det

    eng = HostEngine()
    monkeypatch.setattr(det, "get_engine", lambda device=0: eng)
    monkeypatch.setattr(ms, "_free_bytes", lambda e: 1 << 30)
    return eng


@pytest.mark.parametrize("weighted", [False, True], ids=["cells", "areas"])
def test_public_path_on_the_host_engine(host_engine, weighted):
    import torch

    T, C = 6, 693
    ids, anom = public_field(T, C)
    w = weights(C) if weighted else None
    exp = io.intensity(ids, anom, w, N_EV)
    assert exp["event_duration"].tolist()[4] == 1 and exp["intensity_cells"][4, 5] == 0 and exp["event_duration"][5] >= 2
    tv = np.arange(T).astype("datetime64[D]").astype("datetime64[ns]")
    da_i = _da(ids.reshape(T, 21, 33), tv)
    da_a = _da(anom.reshape(T, 21, 33), tv)
    area = None if w is None else w.reshape(21, 33)
    whole = marex_amd.event_intensity(da_i, da_a, area)
    assert_equals_oracle(whole, exp, tv)
    assert tuple(whole["intensity_max"].dims) == ("time", "ID") and np.array_equal(whole["time"].values, tv)
    assert host_engine.calls == [("id_spans", T), ("event_intensity", 0, T)]
    for b in (1, 4, 6, "auto"):  # the block length changes nothing
        host_engine.calls.clear()
        ds = marex_amd.event_intensity(da_i, da_a, area, block_steps=b)
        for k in whole.data_vars:
            assert np.asarray(ds[k].values).tobytes() == np.asarray(whole[k].values).tobytes(), (b, k)
        if b == 4:
            assert host_engine.calls == [("id_spans", 4), ("id_spans", 2), ("event_intensity", 0, 4), ("event_intensity", 4, 2)]
    # tensors, float64 anomalies, int64 IDs and no names: the same numbers over time = 0 .. T - 1
    ds = marex_amd.event_intensity(torch.from_numpy(ids.astype(np.int64)), torch.from_numpy(anom.astype(np.float64)), w,
                                   per_timestep=False, block_steps=4)
    assert_equals_oracle(ds, exp, np.arange(T), per_timestep=False)


def test_areas_along_y_no_event_and_trailing_ids(host_engine):
    T, C = 6, 693
    ids, anom = public_field(T, C)
    wy = (np.arange(21) + 1).astype(np.float32)
    exp = io.intensity(ids, anom, np.repeat(wy, 33), N_EV)
    tv = np.arange(T)
    assert_equals_oracle(marex_amd.event_intensity(ids.reshape(T, 21, 33), anom.reshape(T, 21, 33), wy), exp, tv)
    wxy = DataArray(np.broadcast_to(wy[None, :], (33, 21)).copy(), dims=("lon", "lat"))  # (x, y) areas are transposed
    assert_equals_oracle(marex_amd.event_intensity(_da(ids.reshape(T, 21, 33)), _da(anom.reshape(T, 21, 33)), wxy), exp, tv)
    none = marex_amd.event_intensity(np.zeros((T, C), np.int32), anom)
    assert none["ID"].values.size == 0 and np.asarray(none["intensity_max"].values).shape == (T, 0)
    assert np.asarray(none["event_duration"].values).shape == (0,)
    # the tracker's Dataset may end in events without a cell: they are absent everywhere
    ds = mi._event_intensity(ids, anom, None, True, None, 0, n_events=N_EV + 2)
    exp = io.intensity(ids, anom, None, N_EV + 2)
    assert_equals_oracle(ds, exp, tv)
    assert exp["event_duration"][-2:].tolist() == [0, 0] and np.isnan(np.asarray(ds["event_intensity_max"].values)[-2:]).all()
    with pytest.raises(marex_amd.ProcessingError, match="the ID field holds event 6, the events Dataset ends at 5"):
        mi._event_intensity(ids, anom, None, True, None, 0, n_events=5)
    with pytest.raises(marex_amd.TrackingError, match=r"event_intensity: needs .* GB of device memory, .* GB are free"):
        marex_amd.event_intensity(np.zeros((2, 1 << 28), np.int8), np.zeros((2, 1 << 28), np.float16))
