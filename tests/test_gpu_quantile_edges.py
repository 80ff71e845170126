"""GPU: the quantile kernels (csrc/marex_quantiles.hip) and the constant-threshold mask (csrc/marex_mask.hip) at the edges
where the host switches between them: counter width (uint16 up to 65 535 steps), kernel generation (`GLOBAL_V1`), the
rank lo + 1 shortcut of k_global_exact16, the (K, workgroup, LDS) classes and the refusal of the exact Hobday percentile,
four cells per lane or one in the mask.  The cases come from tests/quantile_cases.py (checked on the host by
tests/test_quantile_cases_host.py); every comparison is bit for bit against NumPy through the oracle."""
import functools
import os
import sys

import numpy as np
import pytest
import torch

from marex_amd import binning
from marex_amd.exceptions import ProcessingError
from oracle import marex_oracle as orc
from tests.test_gpu_nonfinite_inputs import _field

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import quantile_cases as qc  # noqa: E402

pytestmark = [pytest.mark.gpu, pytest.mark.filterwarnings("ignore::RuntimeWarning")]  # inf - inf inside np.quantile

GENERATIONS = ("dispatched", "v1")
SMALL_T = (1, 2, 15, 16, 17, 400)
DEFAULT_BINS = (0.01, 5.0)
DYADIC_BINS = (0.25, 2.0)  # every edge is a float32 value
PCTS = (0.0, 50.0, 95.0, 100.0)


def _generation(hot, gen):
    """Option context: the kernels the host would pick, or the first generation (32-bit counters) forced."""
    return hot.ctx.options(GLOBAL_V1=1) if gen == "v1" else hot.ctx.options()


def _dev(hot, x):
    return torch.from_numpy(np.array(x, copy=True)).to(hot.device)  # the cases are read-only arrays


def _same(a, b):
    return a == b or (a != a and b != b)


def _check_exact(hot, xd, x, pct, what):
    got = hot.global_threshold(xd, pct, "exact", None)["thr_f64"].cpu().numpy()
    exp = orc.global_threshold_exact(x, pct)
    assert got.dtype == np.float64 and np.array_equal(got, exp, equal_nan=True), (what, pct, np.flatnonzero(~((got == exp) | ((got != got) & (exp != exp)))))


def _check_approx(hot, xd, x, pct, what, bins=DEFAULT_BINS):
    gb = binning.global_bins(*bins)
    g = hot.global_threshold(xd, pct, "approximate", binning.hobday_bins(*bins))
    got = g["thr_f64"].cpu().numpy()
    exp, st = orc.global_threshold_approx(x, pct / 100.0, gb.edges, gb.centres)
    assert np.array_equal(got, exp, equal_nan=True), (what, pct, bins, np.flatnonzero(~((got == exp) | ((got != got) & (exp != exp)))))
    for k in ("n_too_low", "n_too_high", "min", "max"):
        assert _same(g["stats"][k], st[k]), (what, pct, bins, k, g["stats"], st)


# ------------------------------------------------------------------------------------------------------------------------
# counter width and dispatch
# ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("T,pcts", [(65535, PCTS), (65536, (50.0, 95.0))])
@pytest.mark.parametrize("method", ["exact", "approximate"])
def test_counter_saturation_and_dispatch(hot, method, T, pcts):
    """65 535 steps are the most the packed uint16 counters hold (the constant columns fill one counter to 0xFFFF in every
    pass); one step more must take the 32-bit kernels -- on the uint16 kernels those counters would wrap to 0."""
    x, names = qc.global_columns(T)
    xd = _dev(hot, x)
    for pct in pcts:
        (_check_exact if method == "exact" else _check_approx)(hot, xd, x, pct, ("global_columns", T, names))


# ------------------------------------------------------------------------------------------------------------------------
# both generations against NumPy
# ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("T", SMALL_T)
@pytest.mark.parametrize("gen", GENERATIONS)
def test_global_columns_both_generations(hot, gen, T):
    x, names = qc.global_columns(T)
    xd = _dev(hot, x)
    with _generation(hot, gen):
        for pct in PCTS:
            _check_exact(hot, xd, x, pct, (gen, T, names))
            _check_approx(hot, xd, x, pct, (gen, T, names))
    x2, _ = qc.global_columns(T, *DYADIC_BINS)
    xd = _dev(hot, x2)
    with _generation(hot, gen):
        for pct in PCTS:
            _check_approx(hot, xd, x2, pct, (gen, T, names), DYADIC_BINS)


@pytest.mark.parametrize("gen", GENERATIONS)
def test_rank_and_tie_sweeps_both_generations(hot, gen):
    """Every sample count m = 0..m_max in one launch at percentiles whose virtual index is an integer, just either side of
    a half and exactly a half; and every split of 16 samples into copies of a and b, where rank lo + 1 is the last a, the
    first b and everything between."""
    with _generation(hot, gen):
        for m_max in qc.SWEEP_M_MAX:
            x = qc.rank_sweep(m_max)
            xd = _dev(hot, x)
            for pct in qc.SWEEP_PCTS:
                _check_exact(hot, xd, x, pct, (gen, "rank_sweep", m_max))
                _check_approx(hot, xd, x, pct, (gen, "rank_sweep", m_max))  # one NaN-free cell, the rest NaN
        x, splits = qc.tie_sweep()
        xd = _dev(hot, x)
        for pct in qc.TIE_PCTS:
            _check_exact(hot, xd, x, pct, (gen, "tie_sweep", splits))
        for pct in (0.0, 50.0, 100.0):
            _check_approx(hot, xd, x, pct, (gen, "tie_sweep", splits))


@pytest.mark.parametrize("gen", GENERATIONS)
def test_cdf_landings_both_generations(hot, gen):
    with _generation(hot, gen):
        for case in qc.cdf_landings():
            _check_approx(hot, _dev(hot, case.field), case.field, case.pct, (gen, "cdf_landings", case.T, case.names))


@pytest.mark.parametrize("method", ["approximate", "exact"])
def test_special_values_first_generation(hot, method):
    """test_gpu_nonfinite_inputs.test_global_thresholds_on_special_values on the kernels that long series run."""
    a = _field(T=400, C=130, seed=9)
    with hot.ctx.options(GLOBAL_V1=1):
        (_check_exact if method == "exact" else _check_approx)(hot, _dev(hot, a), a, 95.0, "special values, v1")


# ------------------------------------------------------------------------------------------------------------------------
# seeded fuzz
# ------------------------------------------------------------------------------------------------------------------------
_lo, _hi = (int(v) for v in os.environ.get("MAREX_FUZZ_QUANTILE_SEEDS", "0:16").split(":"))


@pytest.mark.parametrize("seed", list(range(_lo, _hi)))
def test_random_global_thresholds(hot, seed):
    rng = np.random.default_rng(7000 + seed)
    T, C = int(rng.integers(1, 701)), int(rng.integers(1, 201))
    pct = float(rng.choice([0, 0.1, 12.5, 50, 90, 95, 99.9, 100]))
    nan_share = float(rng.choice([0.0, 0.0, 0.02, 0.3, 0.9]))
    step = float(rng.choice([0.0, 0.0, 0.01, 0.25, 1.0]))
    method = str(rng.choice(["exact", "approximate"]))
    gen = str(rng.choice(GENERATIONS))
    x = rng.normal(0.5, 1.5, (T, C)).astype(np.float32)
    if step:
        x = (np.round(x / np.float32(step)) * np.float32(step)).astype(np.float32)
    if nan_share:
        nan = rng.random((T, C)) < nan_share
        if method == "approximate":  # one NaN makes a whole cell NaN there: keep some cells without
            nan[:, rng.random(C) < 0.5] = False
        x[nan] = np.nan
    case = (seed, T, C, pct, nan_share, step, method, gen)
    with _generation(hot, gen):
        (_check_exact if method == "exact" else _check_approx)(hot, _dev(hot, x), x, pct, case)


# ------------------------------------------------------------------------------------------------------------------------
# exact Hobday percentile: every (K, workgroup, LDS) class
# ------------------------------------------------------------------------------------------------------------------------
_HOBDAY_RUNS = [(c, C) for c in qc.hobday_cases() if not qc.hobday_refused(c) for C in c.Cs]


@functools.lru_cache(maxsize=None)
def _hobday_reference(years, wd, pct, C):
    """np.nanpercentile itself, once per case at its widest field: the narrower fields are its leading columns."""
    x, _ = qc.hobday_field(years, C)
    exp = orc.hobday_thresholds_exact(x, qc.hobday_calendar(years).doy_out, pct, wd)
    exp.setflags(write=False)
    return exp


def _hobday_check(hot, years, wd, pct, C, C_ref=None):
    x, names = qc.hobday_field(years, C)
    cal = qc.hobday_calendar(years)
    exp = np.ascontiguousarray(_hobday_reference(years, wd, pct, C_ref or C)[:, :C])
    dcal = hot.upload_calendar(cal)
    xd = _dev(hot, x)
    thr = hot.hobday_thresholds_exact(xd, dcal, pct, wd)  # raises when the kernel's overflow counter is not 0
    hot.sync()
    got = thr.cpu().numpy()
    assert got.shape == (366, C)
    bad = ~((got == exp) | ((got != got) & (exp != exp)))
    assert np.array_equal(got, exp, equal_nan=True), (years, wd, pct, C, sorted({names[j] for j in np.nonzero(bad)[1]}), int(bad.sum()))
    m = hot.mask_ge_doy(xd, thr, dcal)
    exp_mask = orc.mask_ge_doy(x, np.ascontiguousarray(exp.T), cal.doy_out)
    assert np.array_equal(m["extreme"].cpu().numpy().astype(bool), exp_mask)
    assert int(m["n_true"].item()) == int(exp_mask.sum())


@pytest.mark.parametrize("case,C", _HOBDAY_RUNS, ids=[f"{c.years}y-wd{c.wd}-p{c.pct:g}-K{c.K}-BT{c.BT}-C{C}" for c, C in _HOBDAY_RUNS])
def test_exact_hobday_launch_classes(hot, case, C):
    _hobday_check(hot, case.years, case.wd, case.pct, C, max(case.Cs))


def test_exact_hobday_refuses_a_window_beyond_the_lds(hot):
    """K > 256 does not fit 64 KiB at the smallest workgroup: an error that names the entry point and the bytes, nothing
    launched, and the engine is as usable as before."""
    case = next(c for c in qc.hobday_cases() if qc.hobday_refused(c))
    (C,) = case.Cs
    x, _ = qc.hobday_field(case.years, C)
    dcal = hot.upload_calendar(qc.hobday_calendar(case.years))
    with pytest.raises(ProcessingError, match="marex_hobday_exact_f32") as e:
        hot.hobday_thresholds_exact(_dev(hot, x), dcal, case.pct, case.wd)
    assert f"{case.lds} bytes of LDS" in str(e.value) and "code -4" in str(e.value)
    _hobday_check(hot, 3, 1, 50.0, 8, 65)


# ------------------------------------------------------------------------------------------------------------------------
# constant-threshold mask
# ------------------------------------------------------------------------------------------------------------------------
def test_constant_mask_one_and_four_cells_per_lane(hot):
    """float64 thresholds strictly between two float32 neighbours, equal to one, NaN, +-inf and +-0.0, at widths that take
    k_mask_ge_const4 (C % 4 == 0) and widths that take k_mask_ge_const, lengths around the 64-row blocks and the 4 rows in
    flight; fresh (poisoned) outputs and one workspace reused by cases of every size."""
    wsp, got_by_case = {}, {}
    for T, C in qc.mask_const_cases():
        anom, thr, kinds = qc.mask_const_case(T, C)
        exp = orc.mask_ge_const(anom, thr)
        ad, td = _dev(hot, anom), _dev(hot, thr)
        for w in (None, wsp):
            m = hot.mask_ge_const(ad, td, wsp=w)
            got = m["extreme"].cpu().numpy()
            assert got.shape == (T, C) and got.dtype == np.uint8 and got.max(initial=0) <= 1
            bad = got.astype(bool) != exp
            assert not bad.any(), (T, C, w is not None, sorted({kinds[j] for j in np.nonzero(bad)[1]}), np.argwhere(bad)[:8])
            assert int(m["n_true"].item()) == int(exp.sum()), (T, C, w is not None)
        got_by_case[T, C] = got
    for T in qc.MASK_T:
        for c4, c1 in zip(qc.MASK_C[:3], qc.MASK_C[3:]):  # (4, 1), (64, 65), (1028, 1027)
            n = min(c4, c1)
            assert np.array_equal(got_by_case[T, c4][:, :n], got_by_case[T, c1][:, :n]), (T, c4, c1)
