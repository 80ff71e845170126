"""``marex_amd.cell_trends`` without a GPU: every refusal before the device; the public path -- the abscissae, a Dataset with
``var=``, dtypes, resident and host maps, grid and mesh outputs -- on a host stand-in for the two engine calls; the oracle
itself (tests/trends_oracle.py) against ``scipy.stats.theilslopes`` and hand-worked Mann-Kendall series."""
import math
import os
import sys

import numpy as np
import pytest
import torch

import marex_amd
import marex_amd._stream as ms
import marex_amd.trends as mt
from marex_amd.engine import HotPath
from marex_amd.exceptions import ConfigurationError, DataValidationError, TrackingError
from marex_amd.xr_compat import DataArray, Dataset

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import trends_cases as tc  # noqa: E402
import trends_oracle as to  # noqa: E402
from trends_host_engine import HostEngine  # noqa: E402

DTYPES = {"n": np.int32, "mk_s": np.int32, "significant": np.bool_}
FLOATS = ("mk_var", "mk_z", "mk_p", "sen_slope", "sen_slope_lo", "sen_slope_hi", "sen_intercept", "ols_slope", "ols_intercept",
          "ols_stderr")
DTYPES.update({k: np.float64 for k in FLOATS})


def assert_equals_oracle(ds, exp, space):
    assert sorted(ds.data_vars) == sorted(exp) == sorted(DTYPES)
    for k, want in exp.items():
        got = np.asarray(ds[k].values)
        assert got.dtype == DTYPES[k], (k, got.dtype)
        assert got.shape == tuple(space), (k, got.shape)
        np.testing.assert_array_equal(got.reshape(-1), want, err_msg=k)


# ------------------------------------------------------------------ refusals
def test_refusals_come_before_the_device(monkeypatch):
    import marex_amd.detect as det

    def no_gpu(*a, **k):
        raise AssertionError("the validation touched the GPU engine")

    monkeypatch.setattr(det, "get_engine", no_gpu)
    m = np.zeros((5, 3, 4))
    ds = Dataset({"days": DataArray(m, dims=("year", "lat", "lon"))})
    V, Cf = DataValidationError, ConfigurationError
    cases = [
        (dict(maps=ds), Cf, "a Dataset needs var="),
        (dict(maps=ds, var="nights"), Cf, "the Dataset has no variable 'nights'"),
        (dict(var="days"), Cf, "var names a variable of a Dataset"),
        (dict(maps=m[0, 0]), V, r"maps must be \(group, y, x\) or \(group, cells\)"),
        (dict(maps=np.zeros((2, 2, 2, 2))), V, r"maps must be \(group, y, x\) or \(group, cells\)"),
        (dict(maps=m.astype(np.complex128)), V, "maps must hold real numbers"),
        (dict(maps=m > 0), V, "maps must hold real numbers"),
        (dict(maps=m[:1]), V, "cell_trends takes 2 .. 256 maps"),
        (dict(maps=np.zeros((257, 3))), V, "cell_trends takes 2 .. 256 maps"),
        (dict(x=np.arange(4.0)), V, "x must hold one real number per map"),
        (dict(x=np.array(list("abcde"))), V, "x must hold one real number per map"),
        (dict(x=np.array([0, 1, 2, 2, 3.0])), V, "x must be finite and strictly increasing"),
        (dict(x=np.array([0, 1, 3, 2, 4.0])), V, "x must be finite and strictly increasing"),
        (dict(x=np.array([0, 1, 2, np.nan, 4.0])), V, "x must be finite and strictly increasing"),
        (dict(x=np.array([0, 1, 2, 3, np.inf])), V, "x must be finite and strictly increasing"),
        (dict(x=np.array([2**53, 2**53 + 1, 2**53 + 2, 2**53 + 3, 2**53 + 4])), V, "x must be finite and strictly increasing"),
        (dict(maps=DataArray(m, dims=("year", "lat", "lon"), coords={"year": ("year", [5, 4, 3, 2, 1])})), V,
         "x must be finite and strictly increasing"),
    ]
    cases += [(dict(alpha=a), Cf, "alpha must lie strictly between 0 and 1") for a in (0, 1, -0.1, 1.5, "0.05", None, True, np.nan)]
    for kw, cls, msg in cases:
        args = dict(maps=m)
        args.update(kw)
        with pytest.raises(cls, match=msg):
            marex_amd.cell_trends(**args)


def test_too_many_cells_is_refused_without_touching_them(monkeypatch):
    import marex_amd.detect as det

    monkeypatch.setattr(det, "get_engine", lambda *a, **k: (_ for _ in ()).throw(AssertionError("touched the engine")))
    huge = np.lib.stride_tricks.as_strided(np.zeros(1), shape=(2, 2**31 - 1), strides=(0, 0))
    with pytest.raises(TrackingError, match="reaches 2\\^31 - 1"):
        marex_amd.cell_trends(huge)


def test_cell_trends_is_public():
    assert "cell_trends" in marex_amd.__all__ and marex_amd.cell_trends is mt.cell_trends
    assert hasattr(HotPath, "trend_stats") and hasattr(HotPath, "trend_select") and HotPath.TREND_MAX_STEPS == mt.MAX_STEPS == 256
    from marex_amd import _lib

    assert "marex_trend_stats_f64" in _lib.PROTOTYPES and "marex_trend_select_f64" in _lib.PROTOTYPES


# ------------------------------------------------------------------ the public path on the host engine
@pytest.fixture
def host_engine(monkeypatch):
    import marex_amd.detect as det

    eng = HostEngine()
    monkeypatch.setattr(det, "get_engine", lambda device=0: eng)
    monkeypatch.setattr(ms, "_free_bytes", lambda e: 1 << 30)
    return eng


def test_grid_with_years_on_the_host_engine(host_engine):
    G, ny, nx = 12, 4, 9
    y = tc.special(G, ny * nx)
    yrs = np.arange(1990, 1990 + G)
    lat, lon = np.linspace(-30, 30, ny), np.linspace(0, 100, nx)
    da = DataArray(y.reshape(G, ny, nx), dims=("year", "lat", "lon"),
                   coords={"year": ("year", yrs), "lat": ("lat", lat), "lon": ("lon", lon)})
    ds = marex_amd.cell_trends(da)
    assert_equals_oracle(ds, to.cell_trends(y, yrs.astype(np.float64)), (ny, nx))
    assert [c[:2] for c in host_engine.calls] == [("trend_stats", (G, ny * nx)), ("trend_select", (4, ny * nx))]
    for k in ds.data_vars:
        assert tuple(ds[k].dims) == ("lat", "lon"), k
        np.testing.assert_array_equal(ds[k].coords["lat"].values, lat)
        np.testing.assert_array_equal(ds[k].coords["lon"].values, lon)
        assert "year" not in ds[k].coords
    # x= overrides the coordinate; a Dataset is taken by var=; alpha moves the bounds only
    x2 = tc.irregular_x(G)
    assert_equals_oracle(marex_amd.cell_trends(da, x=x2), to.cell_trends(y, x2), (ny, nx))
    wide = marex_amd.cell_trends(Dataset({"days": da, "other": da}), var="days", alpha=0.32)
    assert_equals_oracle(wide, to.cell_trends(y, yrs.astype(np.float64), 0.32), (ny, nx))
    for k in ("sen_slope", "mk_p", "ols_slope", "n"):
        np.testing.assert_array_equal(wide[k].values, ds[k].values)
    assert not np.array_equal(wide["sen_slope_lo"].values, ds["sen_slope_lo"].values, equal_nan=True)


def test_mesh_without_a_numeric_coordinate_falls_back_to_arange(host_engine):
    G, C = 9, 70
    y = tc.special(G, C)
    exp = to.cell_trends(y, np.arange(G, dtype=np.float64))
    assert_equals_oracle(marex_amd.cell_trends(y), exp, (C,))
    labels = np.array([f"p{k}" for k in range(G)])
    da = DataArray(y, dims=("period", "ncells"), coords={"period": ("period", labels), "ncells": ("ncells", np.arange(C) * 3)})
    ds = marex_amd.cell_trends(da)
    assert_equals_oracle(ds, exp, (C,))
    assert tuple(ds["n"].dims) == ("ncells",)
    np.testing.assert_array_equal(ds["n"].coords["ncells"].values, np.arange(C) * 3)
    days = np.datetime64("2001-01-01") + np.arange(G)
    dt = DataArray(y, dims=("time", "ncells"), coords={"time": ("time", days)})
    assert_equals_oracle(marex_amd.cell_trends(dt), exp, (C,))  # datetimes are not numbers: arange


@pytest.mark.parametrize("dtype", [np.float64, np.float32, np.uint32, np.int16, np.int64, np.uint8, np.float16])
def test_dtypes_host_and_resident(host_engine, dtype):
    G, C = 10, 33
    rng = np.random.default_rng(8)
    y = rng.poisson(4.0, (G, C)).astype(dtype)
    if np.dtype(dtype).kind == "f":
        y[rng.random((G, C)) < 0.2] = np.nan
    exp = to.cell_trends(y.astype(np.float64), np.arange(G, dtype=np.float64))
    assert_equals_oracle(marex_amd.cell_trends(y), exp, (C,))
    t = torch.from_numpy(y.copy())
    assert_equals_oracle(marex_amd.cell_trends(t), exp, (C,))
    assert_equals_oracle(marex_amd.cell_trends(DataArray(t.reshape(G, 3, 11), dims=("year", "y", "x"))), exp, (3, 11))
    if dtype is np.float64:  # a resident float64 field is read in place, by both launches
        ptrs = {c[2] for c in host_engine.calls[-4:]}
        assert ptrs == {t.data_ptr()}


def test_a_call_that_does_not_fit_says_so_in_bytes(host_engine, monkeypatch):
    G, C = 10, 1000
    y = np.zeros((G, C), np.float32)
    need = mt.device_bytes(G, C, True, 4)
    assert need == 8 * G * C + 4 * G * C + 68 * C + 48 * C + 8 * G + 32
    monkeypatch.setattr(ms, "_free_bytes", lambda e: need - 1)
    with pytest.raises(TrackingError, match="cell_trends: needs .* GB of device memory") as ei:
        marex_amd.cell_trends(y)
    assert str(need) in ei.value.details and str(need - 1) in ei.value.details and host_engine.calls == []
    monkeypatch.setattr(ms, "_free_bytes", lambda e: need)
    marex_amd.cell_trends(y)
    # resident float64 maps are read in place: only the results count
    t = torch.zeros((G, C), dtype=torch.float64)
    monkeypatch.setattr(ms, "_free_bytes", lambda e: mt.device_bytes(G, C, False, 0))
    marex_amd.cell_trends(t)
    assert mt.device_bytes(G, C, False, 0) == 116 * C + 8 * G + 32


# ------------------------------------------------------------------ the oracle itself
def test_vectorised_oracle_equals_the_per_cell_one():
    for name, y, x in [c for c in tc.all_cases() if c[1].shape[1] <= 130 and c[1].shape[0] <= 40]:
        y = y[:, :80]
        for alpha in tc.ALPHAS[:2]:
            vec = to.cell_trends(y, x, alpha)
            for c in range(y.shape[1]):
                one = to.cell_trend(y[:, c], x, alpha)
                for k, v in one.items():
                    np.testing.assert_array_equal(vec[k][c], v, err_msg=f"{name} cell {c} {k}")


def test_rank_rule_of_the_package_equals_the_oracle():
    rng = np.random.default_rng(0)
    n = rng.integers(0, 257, 3000)
    ties = np.array([min(int(rng.integers(0, 3)) * int(rng.integers(0, k * (k - 1) * (2 * k + 5) + 1)), k * (k - 1) * (2 * k + 5))
                     if k > 1 else 0 for k in n])
    for alpha in tc.ALPHAS:
        got = mt.slope_ranks(n, ties, alpha)
        want = np.array([to.ranks_of(int(a), int(b), alpha) for a, b in zip(n, ties)]).T
        np.testing.assert_array_equal(got, want)
        assert got.dtype == np.int32


def test_oracle_equals_scipy_theilslopes():
    stats = pytest.importorskip("scipy.stats")
    rng = np.random.default_rng(2024)
    for k in range(400):
        n_all = int(rng.integers(4, 48))
        x = np.cumsum(rng.integers(1, 3, n_all)).astype(np.float64) if k % 2 else np.arange(n_all, dtype=np.float64)
        y = np.round(rng.normal(0, 1, n_all) + 0.05 * x, 1) if k % 3 else rng.poisson(2.0, n_all).astype(np.float64)
        y[rng.random(n_all) < 0.15] = np.nan
        ok = np.isfinite(y)
        if not 3 <= ok.sum() <= 40:
            continue
        for alpha in (0.05,):
            got = to.cell_trend(y, x, alpha)
            slope, intercept, lo, hi = stats.theilslopes(y[ok], x[ok], 1 - alpha)
            assert (got["sen_slope"], got["sen_intercept"], got["sen_slope_lo"], got["sen_slope_hi"]) == (slope, intercept, lo, hi), k


def test_ranks_from_the_stdlib_z_equal_those_from_scipys_z():
    """``NormalDist().inv_cdf`` and ``scipy.stats.norm.ppf`` differ in the last bits; on these seeded (n, ties, alpha) the
    rounded ranks do not."""
    stats = pytest.importorskip("scipy.stats")
    rng = np.random.default_rng(6023)
    for _ in range(3000):
        n = int(rng.integers(2, 257))
        full = n * (n - 1) * (2 * n + 5)
        ties = int(rng.integers(0, full + 1)) if rng.random() < 0.5 else 0
        alpha = float(rng.choice([0.01, 0.05, 0.1, 0.32, 0.5, rng.uniform(0.001, 0.999)]))
        P = n * (n - 1) // 2
        z = stats.norm.ppf(alpha / 2.0)
        sigma = np.sqrt((full - ties) / 18.0)
        want = ((P - 1) // 2, P // 2, max(int(np.round((P + z * sigma) / 2.0)) - 1, 0), min(int(np.round((P - z * sigma) / 2.0)), P - 1))
        assert to.ranks_of(n, ties, alpha) == want, (n, ties, alpha)


def test_mann_kendall_on_hand_worked_series():
    x = np.arange(5.0)
    inc = to.cell_trend(np.array([1.0, 2.0, 3.5, 4.0, 9.0]), x)
    assert inc["mk_s"] == 10 and inc["mk_var"] == 300 / 18.0  # 5 * 4 * 15 = 300, no ties
    z = 9 / math.sqrt(300 / 18.0)
    assert inc["mk_z"] == z and inc["mk_p"] == math.erfc(z / math.sqrt(2.0)) and inc["significant"]
    const = to.cell_trend(np.full(5, 2.0), x)
    assert (const["mk_s"], const["mk_var"], const["mk_z"], const["mk_p"]) == (0, 0.0, 0.0, 1.0) and not const["significant"]
    assert const["sen_slope"] == 0.0 and const["ols_slope"] == 0.0
    # 1 1 2 2 2: the pairs across the groups are 2 * 3 = 6 rises; ties 2 * 1 * 9 + 3 * 2 * 11 = 84; v18 = 300 - 84 = 216
    two = to.cell_trend(np.array([1.0, 1.0, 2.0, 2.0, 2.0]), x)
    assert two["mk_s"] == 6 and two["mk_var"] == 216 / 18.0 == 12.0
    assert two["mk_z"] == 5 / math.sqrt(12.0) and two["mk_p"] == math.erfc(5 / math.sqrt(12.0) / math.sqrt(2.0))
    dec = to.cell_trend(np.array([3.0, np.nan, 2.0, -np.inf, 1.0]), x)  # three valid samples, falling
    assert dec["n"] == 3 and dec["mk_s"] == -3 and dec["mk_var"] == 66 / 18.0 and dec["mk_z"] == -2 / math.sqrt(66 / 18.0)
    assert dec["sen_slope"] == -0.5 and dec["ols_slope"] == -0.5 and dec["sen_intercept"] == 2.0 - (-0.5) * 2.0
    for few in (np.array([np.nan] * 5), np.array([np.nan, 1.0, np.nan, np.nan, np.inf])):
        r = to.cell_trend(few, x)
        assert all(np.isnan(r[k]) for k in ("mk_z", "mk_p", "sen_slope", "sen_slope_lo", "sen_slope_hi", "sen_intercept",
                                            "ols_slope", "ols_stderr")) and not r["significant"] and r["mk_var"] == 0.0
    # the package's own finish gives the same from the integers
    var, zz, pp = mt.mann_kendall(np.array([5, 5, 5, 3, 0]), np.array([10, 0, 6, -3, 0]), np.array([0, 300, 84, 0, 0]))
    np.testing.assert_array_equal(var, [300 / 18.0, 0.0, 12.0, 66 / 18.0, 0.0])
    np.testing.assert_array_equal(zz, [inc["mk_z"], 0.0, two["mk_z"], dec["mk_z"], np.nan])
    np.testing.assert_array_equal(pp, [inc["mk_p"], 1.0, two["mk_p"], dec["mk_p"], np.nan])
