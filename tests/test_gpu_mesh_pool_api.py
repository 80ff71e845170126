"""GPU: ``neighbour_rings_hobday`` through the public API.  Thresholds and extremes of ``preprocess_data`` /
``identify_extremes`` on a mesh equal tests/mesh_pool_oracle.py applied to the anomalies the call returns; spatial blocks
(cell ranges with the halo cells their pools reach) and two engines give the single-block Dataset bit for bit, warnings and
the low-sample log line included; ``None`` and ``0`` are the call without the keyword."""
import logging
import os
import sys
import warnings

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import marex_amd  # noqa: E402
from marex_amd import binning, calendar, synth  # noqa: E402
from marex_amd.engine import HotPath  # noqa: E402
from marex_amd.exceptions import ConfigurationError  # noqa: E402
from marex_amd.xr_compat import DataArray  # noqa: E402
from mesh_pool_oracle import pooled_extremes, ring_and_chords  # noqa: E402

pytestmark = pytest.mark.gpu

N = 301
DIMS, COORDS = {"time": "time", "x": "ncells"}, {"time": "time", "x": "lon", "y": "lat"}
NBR = ring_and_chords(np.random.default_rng(11), N)

METHODS = {
    "shifting": dict(method_anomaly="shifting_baseline", window_year_baseline=5),
    "fixed": dict(method_anomaly="fixed_baseline"),
    "detrend-stn": dict(method_anomaly="detrend_harmonic", std_normalise=True),
}

_mesh = []


def mesh():
    """The 301-cell mesh of tests/test_gpu_blocks.py::mesh."""
    if not _mesh:
        tm = calendar.daily_time_axis("1990-01-01", 12 * 365 + 3)
        x = synth.synth_field(synth.make_tables(tm, 0, N))
        _mesh.append(DataArray(x, dims=("time", "ncells"), coords={"time": tm, "lat": ("ncells", np.linspace(-80, 80, N)),
                                                                    "lon": ("ncells", np.linspace(0, 359, N))}))
    return _mesh[0]


def run(monkeypatch, caplog, blocks, **kw):
    monkeypatch.setenv("MAREX_BLOCKS", str(blocks))
    caplog.clear()
    with warnings.catch_warnings(record=True) as w, caplog.at_level(logging.WARNING, logger="marex_amd"):
        warnings.simplefilter("always")
        ds = marex_amd.preprocess_data(mesh(), dimensions=DIMS, coordinates=COORDS, **kw)
    return ds, sorted(str(x.message) for x in w), [r.getMessage() for r in caplog.records if "Not enough samples" in r.getMessage()]


def same(a, b):
    assert set(a.data_vars) == set(b.data_vars)
    for k in a.data_vars:
        assert a[k].dims == b[k].dims and a[k].values.dtype == b[k].values.dtype, k
        assert np.array_equal(a[k].values, b[k].values, equal_nan=a[k].values.dtype.kind == "f"), k
    assert a.attrs == b.attrs


def check_against_oracle(ds, anom_name, thr_name, ext_name, rings, pct=95.0, wd=11):
    anom = ds[anom_name].values
    doy = calendar.build_calendar(np.asarray(ds[anom_name].coords["time"].values)).doy_out
    bt = binning.hobday_bins()
    thr, _, ext = pooled_extremes(anom, doy, pct / 100.0, wd, bt.edges, bt.centres, NBR, rings)
    assert ds[thr_name].dims == ("ncells", "dayofyear")
    assert np.array_equal(ds[thr_name].values, thr, equal_nan=True), thr_name
    assert np.array_equal(ds[ext_name].values, ext), ext_name


_single = {}


def single(monkeypatch, caplog, method, rings):
    if (method, rings) not in _single:
        _single[(method, rings)] = run(monkeypatch, caplog, 1, neighbours=NBR, neighbour_rings_hobday=rings, **METHODS[method])
    return _single[(method, rings)]


@pytest.mark.parametrize("rings", [1, 2])
@pytest.mark.parametrize("method", list(METHODS))
def test_preprocess_data_equals_the_oracle(hot, monkeypatch, caplog, method, rings):
    ds, _, logged = single(monkeypatch, caplog, method, rings)
    check_against_oracle(ds, "dat_anomaly", "thresholds", "extreme_events", rings)
    if method == "detrend-stn":
        check_against_oracle(ds, "dat_stn", "thresholds_stn", "extreme_events_stn", rings)
    assert ds.attrs["neighbour_rings_hobday"] == rings
    assert ds.attrs["preprocessing_steps"][-1] == f"Day-of-year thresholds with 11 day window & {rings} neighbour rings"
    assert np.array_equal(ds["neighbours"].values, NBR) and ds["neighbours"].dims == ("nv", "ncells")
    # the low-sample warning counts the pool: years x 11 days x median ocean members x 5 %
    x0 = mesh().values[0]
    samples = marex_amd.detect._pool_samples(HotPath.pool_table(NBR, rings), np.isfinite(x0))
    years = int(np.unique(calendar.build_calendar(np.asarray(ds["dat_anomaly"].coords["time"].values)).year).size)
    assert years == (7 if method == "shifting" else 12)
    n_above = years * 11 * samples * (1.0 - 95 / 100.0)
    assert logged == ([f"Not enough samples for accurate extreme detection: {n_above} < 50. "
                       "Consider using a lower threshold_percentile, increasing your time-series size, "
                       "increasing the window_days_hobday, or using a larger window_spatial_hobday."] if n_above < 50 else [])
    unpooled, _, _ = run(monkeypatch, caplog, 1, **METHODS[method])
    assert (unpooled["thresholds"].values != ds["thresholds"].values).mean() > 0.9     # pooling did change the thresholds
    assert np.array_equal(unpooled["dat_anomaly"].values, ds["dat_anomaly"].values, equal_nan=True)


@pytest.mark.parametrize("rings", [1, 2])
@pytest.mark.parametrize("method", list(METHODS))
def test_blocks_equal_a_single_block(hot, monkeypatch, caplog, method, rings):
    ref, wref, lref = single(monkeypatch, caplog, method, rings)
    for blocks in (3, 10):
        got, wgot, lgot = run(monkeypatch, caplog, blocks, neighbours=NBR, neighbour_rings_hobday=rings, **METHODS[method])
        same(ref, got)
        assert wgot == wref and lgot == lref


@pytest.mark.parametrize("method,rings", [("shifting", 2), ("detrend-stn", 1)])
def test_two_engines_equal_one(hot, monkeypatch, caplog, method, rings):
    ref, wref, lref = single(monkeypatch, caplog, method, rings)
    monkeypatch.delenv("MAREX_BLOCKS", raising=False)
    with warnings.catch_warnings(record=True) as w:
        warnings.simplefilter("always")
        got = marex_amd.preprocess_data(mesh(), dimensions=DIMS, coordinates=COORDS, devices=[0, 0], neighbours=NBR,
                                        neighbour_rings_hobday=rings, **METHODS[method])
    same(ref, got)
    assert sorted(str(x.message) for x in w) == wref


def test_neighbours_as_a_labelled_array_and_transposed(hot, monkeypatch, caplog):
    ref, _, _ = single(monkeypatch, caplog, "fixed", 1)
    monkeypatch.setenv("MAREX_BLOCKS", "1")
    for nbr in (DataArray(NBR, dims=("nv", "ncells")), DataArray(np.ascontiguousarray(NBR.T), dims=("ncells", "nv"))):
        got = marex_amd.preprocess_data(mesh(), dimensions=DIMS, coordinates=COORDS, neighbours=nbr, neighbour_rings_hobday=1,
                                        **METHODS["fixed"])
        for k in ("thresholds", "extreme_events", "dat_anomaly"):
            assert np.array_equal(ref[k].values, got[k].values, equal_nan=True), k


@pytest.mark.parametrize("rings", [1, 2])
def test_identify_extremes_equals_the_oracle(hot, monkeypatch, caplog, rings):
    ds, _, _ = single(monkeypatch, caplog, "fixed", 1)
    anom = ds["dat_anomaly"]
    ext, thr = marex_amd.identify_extremes(anom, dimensions=DIMS, coordinates=COORDS, neighbours=NBR, neighbour_rings_hobday=rings,
                                           threshold_percentile=90, window_days_hobday=5)
    doy = calendar.build_calendar(np.asarray(anom.coords["time"].values)).doy_out
    bt = binning.hobday_bins()
    exp_thr, _, exp_ext = pooled_extremes(anom.values, doy, 0.90, 5, bt.edges, bt.centres, NBR, rings)
    assert np.array_equal(thr.values, exp_thr, equal_nan=True) and np.array_equal(ext.values, exp_ext)
    plain = marex_amd.identify_extremes(anom, dimensions=DIMS, coordinates=COORDS, threshold_percentile=90, window_days_hobday=5)
    for none in (None, 0):
        e0, t0 = marex_amd.identify_extremes(anom, dimensions=DIMS, coordinates=COORDS, threshold_percentile=90, window_days_hobday=5,
                                             neighbours=NBR, neighbour_rings_hobday=none)
        assert np.array_equal(t0.values.view(np.uint32), plain[1].values.view(np.uint32)) and np.array_equal(e0.values, plain[0].values)


@pytest.mark.parametrize("method", ["shifting", "detrend-stn"])
def test_none_and_zero_are_the_call_without_the_keyword(hot, monkeypatch, caplog, method):
    ref, wref, lref = run(monkeypatch, caplog, 1, neighbours=DataArray(NBR, dims=("nv", "ncells")), **METHODS[method])
    for none in (None, 0):
        got, wgot, lgot = run(monkeypatch, caplog, 1, neighbours=DataArray(NBR, dims=("nv", "ncells")), neighbour_rings_hobday=none,
                              **METHODS[method])
        same(ref, got)
        for k in ref.data_vars:
            if ref[k].values.dtype.kind == "f":
                assert np.array_equal(ref[k].values.view(np.uint32), got[k].values.view(np.uint32)), k
        assert wgot == wref and lgot == lref
    assert "neighbour_rings_hobday" not in ref.attrs and len(lref) == 1       # the unpooled mesh run is the one that is warned


def test_the_bin_matrix_path_cannot_pool(hot, monkeypatch):
    monkeypatch.setenv("MAREX_BLOCKS", "1")
    hot.hobday_path = "bins"
    try:
        with pytest.raises(ConfigurationError, match="neighbour_rings_hobday needs the sorted key lists"):
            marex_amd.preprocess_data(mesh(), dimensions=DIMS, coordinates=COORDS, neighbours=NBR, neighbour_rings_hobday=1,
                                      **METHODS["fixed"])
    finally:
        hot.hobday_path = None
