"""Host checks of the quantile cases (tests/quantile_cases.py): no device.

* The cases are what they claim to be: each exact-Hobday case lands in its (K, BT, LDS) class under the sizing rule of
  marex_hobday_exact_f32 (restated in quantile_cases.hobday_sizing and pinned to the source lines it restates), the rank
  sweeps hit integer and exactly-half virtual indices, the tie sweep puts rank lo + 1 on the last copy of a and on the first
  b, every CDF landing takes the branch of the approximate rule it names.
* A second, independent reference for the exact global threshold (sort + NumPy's float64 lerp by hand) equals
  oracle.global_threshold_exact on every case, and the constant columns of the approximate method have the closed forms
  asserted here literally: a disagreement on the device cannot be an oracle quirk.
"""
import os
import re
import sys

import numpy as np
import pytest

from marex_amd import binning
from marex_amd._keys import float_key
from oracle import marex_oracle as orc

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import quantile_cases as qc  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HOST_T = (1, 2, 15, 16, 17, 400, 65535, 65536)


# ------------------------------------------------------------------------------------------------------------------------
# exact Hobday cases
# ------------------------------------------------------------------------------------------------------------------------
def test_sizing_rule_is_the_one_in_the_source():
    """quantile_cases.hobday_sizing restates these lines; when they change, the restatement (and the classes below) must
    be looked at again."""
    src = re.sub(r"\s+", " ", open(os.path.join(ROOT, "marex_amd", "csrc", "marex_quantiles.hip")).read())
    for line in (
        "const int upper = q >= 0.5;",
        "const double tail = upper ? (1.0 - q) : q;",
        "int K = (int)ceil(tail * max_window_rows) + 4;",
        "if (K > max_window_rows) K = max_window_rows;",
        "int BT = 256;",
        "while (BT > 64 && (size_t)K * BT * 4 > 64 * 1024) BT >>= 1;",
        "const size_t lds = (size_t)K * BT * 4;",
        "if (lds > 64 * 1024) return fail(ctx, -4,",
        "if (lds > 48 * 1024) HIP_TRY(ctx, hipFuncSetAttribute((const void*)k_hobday_exact,",
    ):
        assert line in src, line
    eng = re.sub(r"\s+", " ", open(os.path.join(ROOT, "marex_amd", "engine.py")).read())
    assert "q32 = np.float32(percentile) / np.float32(100)" in eng
    assert 'self.call("marex_hobday_exact_f32", anom, T_out, Cn, dcal.doy_start, dcal.doy_rows, max(max_rows, 1), float(q32), float(q32),' in eng


@pytest.mark.parametrize("case", qc.hobday_cases(), ids=lambda c: f"{c.years}y-wd{c.wd}-p{c.pct:g}")
def test_hobday_case_lands_in_its_class(case):
    cal = qc.hobday_calendar(case.years)
    assert cal.doy_out.size == case.years * 365 + 3
    rows = qc.max_window_rows(cal, case.wd)
    # the engine's own expression (HotPath.hobday_thresholds_exact)
    nd = np.diff(cal.doy_start).astype(np.int64)
    half = case.wd // 2
    ext = np.concatenate([nd[-half:], nd, nd[:half]]) if half else nd
    assert rows == int(np.convolve(ext, np.ones(case.wd, dtype=np.int64), mode="valid").max()) == case.max_rows
    assert qc.hobday_sizing(rows, case.pct) == (case.K, case.BT, case.lds)
    assert qc.hobday_refused(case) == (case.lds > 65536)


def test_hobday_cases_cover_every_launch_class():
    cases = qc.hobday_cases()
    run = [c for c in cases if not qc.hobday_refused(c)]
    assert {c.BT for c in run} == {256, 128, 64}
    for bt in (128, 64):  # either side of the 48 KiB attribute branch at both halved sizes
        assert any(c.BT == bt and c.lds > qc.LDS_ATTRIBUTE for c in run) and any(c.BT == bt and c.lds <= qc.LDS_ATTRIBUTE for c in run)
    assert any(c.pct < 50 and c.lds > qc.LDS_ATTRIBUTE for c in run)                  # negated keys in a large launch
    assert any((c.years, c.wd, c.pct) == (12, 11, 50.0) and (c.K, c.BT) == (70, 128) for c in run)  # median, default window
    assert [c for c in cases if qc.hobday_refused(c)] and all(c.K > 256 for c in cases if qc.hobday_refused(c))
    # the clamp: the unclamped K exceeds the window
    assert any(int(np.ceil(0.5 * c.max_rows)) + 4 > c.max_rows == c.K for c in run if c.pct == 50.0)
    assert sum(130 in c.Cs for c in run) == 2 and all(set(c.Cs) >= {1, 63, 65} for c in run)


def test_hobday_fields_take_m_from_below_k_to_the_full_window():
    case = next(c for c in qc.hobday_cases() if (c.years, c.wd, c.pct) == (13, 31, 50.0))
    x, names = qc.hobday_field(case.years, 65)
    assert set(names) == set(qc.HOBDAY_KINDS) and x.dtype == np.float32 and x.shape == (13 * 365 + 3, 65)
    masks = orc.doy_window_masks(qc.hobday_calendar(case.years).doy_out, case.wd)
    m = np.stack([(~np.isnan(x[w])).sum(axis=0) for w in masks])  # non-NaN samples [366, C]
    col = lambda k: names.index(k)  # noqa: E731
    assert m[:, col("normal")].max() == case.max_rows
    assert 0 < m[:, col("nan90")].min() and m[:, col("nan90")].max() < case.K
    assert m[:, col("nan50")].min() < case.K < m[:, col("nan50")].max()
    assert set(np.unique(m[:, col("one_sample")])) == {0, 1} and (m[:, col("all_nan")] == 0).all()
    assert np.isposinf(x[:, col("inf_ends")]).sum() == 1 and np.isneginf(x[:, col("inf_ends")]).sum() == 1
    z = x[:, col("zeros")]
    assert (z == 0).all() and 0 < np.signbit(z).sum() < z.size
    # the single column of C = 1 is not the same kind for every series length
    assert [qc.hobday_field(y, 1)[1][0] for y in (3, 12, 13)] == ["nan50", "normal", "rounded"]
    # narrower fields are the leading columns of wider ones (the device test shares one reference per case)
    wide = qc.hobday_field(13, 130)
    for C in (1, 8, 63, 65):
        f, n = qc.hobday_field(13, C)
        assert np.array_equal(f, wide[0][:, :C], equal_nan=True) and n == wide[1][:C]
    # 3-year series: day 366 has one sample, 1 January four
    cal3 = qc.hobday_calendar(3)
    assert np.diff(cal3.doy_start)[365] == 1 and np.diff(cal3.doy_start)[0] == 4


# ------------------------------------------------------------------------------------------------------------------------
# global columns, rank sweeps
# ------------------------------------------------------------------------------------------------------------------------
def test_global_columns_are_what_they_claim():
    gb = binning.global_bins()
    for T in (1, 2, 17, 400, 65535):
        x, names = qc.global_columns(T)
        assert x.shape == (T, 66) and x.dtype == np.float32 and set(names) == set(qc.GLOBAL_KINDS)
        for j, k in enumerate(names):
            v = x[:, j]
            if k == "const":
                assert (v == 1.5).all()
            elif k in ("one_larger", "one_smaller"):
                assert (v == 0.75).sum() == T - 1 and ((v > 0.75) if k == "one_larger" else (v < 0.75)).sum() == 1
            elif k == "low_byte":
                key = float_key(v)
                assert np.unique(key >> 8).size == 1 and np.unique(key & 255).size == min(T, 256)
            elif k == "subnormals" and T >= 400:
                assert sorted(np.unique(float_key(v)).tolist()) == sorted(float_key(np.array([qc.TINY, -qc.TINY, 0.0, -0.0], np.float32)).tolist())
                assert abs(int((v > 0).sum()) - T // 4) <= 1 and abs(int((v < 0).sum()) - T // 4) <= 1
            elif k == "zeros":
                assert (v == 0).all() and (T == 1 or abs(int(np.signbit(v).sum()) - T / 2) <= 0.5)
            elif k == "inf_ends":
                assert np.isposinf(v).sum() == 1 and np.isneginf(v).sum() == (T > 1)
            elif k == "nan30" and T >= 400:
                assert 0.2 < np.isnan(v).mean() < 0.4
            elif k == "one_sample":
                assert (~np.isnan(v)).sum() == 1
            elif k == "all_nan":
                assert np.isnan(v).all()
            elif k == "one_bin":
                assert (v >= gb.edges[2]).all() and (v < gb.edges[3]).all()
            elif k == "below":
                assert (v < gb.edges[1]).all()
            elif k == "last_edge":
                assert (v.astype(np.float64) == gb.edges[-1]).all()  # the float64 compare of the kernels can be true
            elif k == "beyond":
                assert (v > gb.edges[-1]).all()
            elif k == "edges" and T >= 65535:
                e32 = gb.edges[1:].astype(np.float32)
                for w in (e32, np.nextafter(e32, np.float32(np.inf)), np.nextafter(e32, np.float32(-np.inf))):
                    assert np.isin(w, v).all()
    x, _ = qc.global_columns(65535)
    assert (x[:, 0] == 1.5).sum() == 0xFFFF          # one uint16 counter filled to exactly its maximum
    assert qc.global_columns(65536)[0].shape[0] == 0x10000
    # a table whose edges are all float32 values: every edge compare of the approximate kernels can hit equality
    x, names = qc.global_columns(400, 0.25, 2.0)
    g2 = binning.global_bins(0.25, 2.0)
    assert (g2.edges[1:].astype(np.float32) == g2.edges[1:]).all() and (x[:, names.index("last_edge")] == 2.0).all()


@pytest.mark.parametrize("m_max", qc.SWEEP_M_MAX)
def test_rank_sweep_hits_integer_and_half_indices(m_max):
    x = qc.rank_sweep(m_max)
    assert x.shape == (m_max, m_max + 1)
    assert np.array_equal((~np.isnan(x)).sum(axis=0), m_max - np.arange(m_max + 1))
    frac = {pct: [qc.rank_indices(m, pct)[2] for m in range(2, m_max + 1)] for pct in qc.SWEEP_PCTS}
    for pct in (100.0 * 5 / 32, 96.875):
        g = np.array(frac[pct])
        assert (g == 0.0).any() and (g == 0.5).any() and ((g > 0) & (g < 0.5)).any() and (g > 0.5).any(), pct
    assert (np.array(frac[50.0]) == 0.5).any() and (np.array(frac[50.0]) == 0.0).any()
    assert all(g == 0.0 for g in frac[0.0]) and all(g == 0.0 for g in frac[100.0])
    m33 = 33
    assert qc.rank_indices(m33, 100.0 * 5 / 32)[::2] == (5, 0.0) and qc.rank_indices(m33, 96.875)[::2] == (31, 0.0)


def test_tie_sweep_puts_hi_on_the_last_a_and_on_the_first_b():
    x, splits = qc.tie_sweep()
    assert x.shape == (16, 17 * len(qc.TIE_PAIRS))
    last_a, first_b, inside_a, inside_b = set(), set(), set(), set()
    for col, (p, n_a) in enumerate(splits):
        a, b = qc.TIE_PAIRS[p]
        ka, kb = float_key(np.array([a, b], np.float32))
        assert ka < kb
        assert (float_key(x[:, col]) == ka).sum() == n_a and (float_key(x[:, col]) == kb).sum() == 16 - n_a
        for pct in qc.TIE_PCTS:
            lo, hi, _ = qc.rank_indices(16, pct)
            if hi == lo:
                continue
            if hi == n_a - 1:
                last_a.add(p)
            if hi == n_a:
                first_b.add(p)
            if hi < n_a - 1:
                inside_a.add(p)
            if hi > n_a:
                inside_b.add(p)
    every = set(range(len(qc.TIE_PAIRS)))
    assert last_a == first_b == inside_a == inside_b == every
    # lowest key byte apart; either side of the sign change; two keys of one float value
    k = [float_key(np.array(p, np.float32)) for p in qc.TIE_PAIRS]
    assert k[0][1] - k[0][0] == 1 and (k[0][0] >> 8) == (k[0][1] >> 8)
    assert k[1][0] < 0x80000000 <= k[1][1]
    assert k[2][1] - k[2][0] == 1 and qc.TIE_PAIRS[2][0] == qc.TIE_PAIRS[2][1]


# ------------------------------------------------------------------------------------------------------------------------
# second reference of the exact global threshold
# ------------------------------------------------------------------------------------------------------------------------
def sorted_lerp_reference(x, pct):
    """np.quantile's "linear" method by hand, per cell: sort the non-NaN float32 samples, take ranks floor((m - 1) q) and
    the next, subtract in float32 (the dtype of the data), scale and add in float64 (the dtype of q)."""
    out = np.full(x.shape[1], np.nan, np.float64)
    q = pct / 100.0
    with np.errstate(invalid="ignore", over="ignore"):
        for c in range(x.shape[1]):
            v = np.sort(x[~np.isnan(x[:, c]), c])
            m = v.size
            if m == 0:
                continue
            virt = (m - 1) * q
            lo = int(np.floor(virt))
            g = virt - lo
            hi = lo + 1
            if lo >= m - 1:
                lo = hi = m - 1
            a, b = v[lo], v[hi]
            d = np.float64(np.float32(b - a))
            out[c] = np.float64(b) - d * (1.0 - g) if g >= 0.5 else np.float64(a) + d * g
    return out


@pytest.mark.filterwarnings("ignore::RuntimeWarning")  # inf - inf inside np.quantile
@pytest.mark.parametrize("T", HOST_T)
def test_second_reference_equals_the_oracle_on_global_columns(T):
    x, names = qc.global_columns(T)
    for pct in (0.0, 50.0, 95.0, 100.0):
        exp = orc.global_threshold_exact(x, pct)
        assert np.array_equal(sorted_lerp_reference(x, pct), exp, equal_nan=True), (T, pct)
        assert np.isnan(exp[[j for j, k in enumerate(names) if k == "all_nan"]]).all()
        assert (exp[[j for j, k in enumerate(names) if k == "const"]] == 1.5).all()


@pytest.mark.filterwarnings("ignore::RuntimeWarning")
def test_second_reference_equals_the_oracle_on_rank_and_tie_sweeps():
    for m_max in qc.SWEEP_M_MAX:
        for pct in qc.SWEEP_PCTS:
            x = qc.rank_sweep(m_max)
            assert np.array_equal(sorted_lerp_reference(x, pct), orc.global_threshold_exact(x, pct), equal_nan=True), (m_max, pct)
    x, _ = qc.tie_sweep()
    for pct in qc.TIE_PCTS:
        assert np.array_equal(sorted_lerp_reference(x, pct), orc.global_threshold_exact(x, pct), equal_nan=True), pct


# ------------------------------------------------------------------------------------------------------------------------
# approximate method: branches and closed forms
# ------------------------------------------------------------------------------------------------------------------------
def approx_intermediates(v, q, gb):
    """The steps of _compute_histogram_quantile_1d on one NaN-free column, with np.histogram itself for the counts:
    ``(threshold before the clamp, branch, il, iu)``."""
    nb, eps = gb.nb, 1e-10
    hist = np.histogram(v.astype(np.float64), bins=gb.edges)[0].astype(np.float64)
    cdf = np.cumsum(hist / (hist.sum() + 1e-10))
    iu = int(np.argmax(cdf >= q - eps))
    il = int(np.argmax(cdf > cdf[max(iu - 1, 0)]))
    il, iu = min(il, nb - 2), min(max(iu, 1), nb - 1)
    cl, cu = cdf[il], cdf[iu]
    bl, bu = gb.centres[il], gb.centres[iu]
    if abs(cl - q) < eps:
        return bl, "exact", il, iu
    if abs(cu - cl) <= eps:
        return (bl + bu) / 2, "zero", il, iu
    return bl + (q - cl) / (cu - cl) * (bu - bl), "interp", il, iu


def test_cdf_landings_take_the_branch_they_name():
    gb = binning.global_bins()
    seen = set()
    cases = qc.cdf_landings()
    assert {c.T for c in cases} == {20, 40, 100, 200}
    for case in cases:
        q = case.pct / 100.0
        thr, st = orc.global_threshold_approx(case.field, q, gb.edges, gb.centres)
        assert st["n_too_low"] == 0 and not np.isnan(case.field).any()
        for j, name in enumerate(case.names):
            r, branch, il, iu = approx_intermediates(case.field[:, j], q, gb)
            assert r == thr[j], (case.T, case.pct, name)          # the restated steps are the oracle's
            assert branch == case.branch[j], (case.T, case.pct, name, branch)
            assert (il == iu) == (branch != "interp")
            if name.startswith("near+0") or name.startswith("far+0"):
                assert r == gb.centres[qc.LAND_A]
            if name.startswith("far-1"):
                assert r == gb.centres[qc.LAND_FAR]
            seen.add(branch)
        assert {n[:4] for n in case.names} >= {"near", "far-", "far+", "last"}
    assert seen == {"exact", "zero", "interp"}


@pytest.mark.parametrize("precision,max_anomaly", [(0.01, 5.0), (0.25, 2.0)])
def test_approximate_constant_columns_have_their_closed_forms(precision, max_anomaly):
    gb = binning.global_bins(precision, max_anomaly)
    nb, c = gb.nb, gb.centres
    for T in (1, 17, 400):
        x, names = qc.global_columns(T, precision, max_anomaly)
        kinds = ("one_bin", "below", "beyond", "last_edge")
        x = np.ascontiguousarray(x[:, [names.index(k) for k in kinds]])
        col = lambda k: kinds.index(k)  # noqa: E731
        for q in (0.5, 0.95):
            thr, st = orc.global_threshold_approx(x, q, gb.edges, gb.centres)
            # all mass in the bin [0, precision): both searches stop there, cl = cu: the "mean" of one centre, which lies
            # below the clamp edges[3]
            assert approx_intermediates(x[:, col("one_bin")], q, gb) == (c[2], "zero", 2, 2)
            assert c[2] == precision / 2 < gb.lower_bound == thr[col("one_bin")]
            # all below edges[1] (bin 0): iu = 0 is raised to 1, il = argmax of an all-False mask = 0, cl = cu -> the mean
            # of centres 0 and 1, which lies below the clamp
            assert (c[0] + c[1]) / 2 == -precision / 4 and thr[col("below")] == gb.lower_bound
            # nothing counted: the CDF is 0 everywhere, both argmax see all-False masks: the same two centres
            assert thr[col("beyond")] == gb.lower_bound
            # all on the last edge -> last bin (closed): il is clamped to nb - 2 where the CDF is 0, the rule interpolates
            cu = T / (T + 1e-10)
            assert thr[col("last_edge")] == c[nb - 2] + (q - 0.0) / (cu - 0.0) * (c[nb - 1] - c[nb - 2])
            assert thr[col("last_edge")] > gb.lower_bound
            # the un-clamped minimum the warning reports is that mean of centres 0 and 1
            assert st["min"] == -precision / 4 and st["n_too_low"] == 3
            assert st["n_too_high"] == int(thr[col("last_edge")] > gb.upper_bound)
            assert st["max"] == thr[col("last_edge")]
            for k in kinds:
                r, _, _, _ = approx_intermediates(x[:, col(k)], q, gb)
                assert max(r, gb.lower_bound) == thr[col(k)], k


# ------------------------------------------------------------------------------------------------------------------------
# constant-threshold mask cases
# ------------------------------------------------------------------------------------------------------------------------
def test_mask_cases_are_what_they_claim():
    cases = qc.mask_const_cases()
    assert len(cases) == 42 and {C % 4 for _, C in cases} == {0, 1, 3} and {T for T, _ in cases} == set(qc.MASK_T)
    anom, thr, kinds = qc.mask_const_case(130, 1028)
    assert set(kinds) == set(qc.MASK_KINDS) and anom.dtype == np.float32 and thr.dtype == np.float64
    flips = 0
    for j, k in enumerate(kinds):
        a = anom[:, j]
        if k == "midpoint":
            v = a[0]
            up = np.nextafter(v, np.float32(np.inf))
            assert float(v) < thr[j] < float(up) and thr[j] == (float(v) + float(up)) / 2
            assert np.float32(thr[j]) in (v, up) and (a[1], a[2]) == (up, np.nextafter(v, np.float32(-np.inf)))
            # a float32 compare gives another answer for v whenever the midpoint rounds down to it
            flips += int(np.float32(thr[j]) == v)
        elif k == "equal":
            assert np.float64(np.float32(thr[j])) == thr[j] and a[0] == thr[j] and a[1] > thr[j] > a[2]
        elif k == "nan":
            assert np.isnan(thr[j]) and np.isnan(a).any() and np.isinf(a).any()
        elif k == "pinf":
            assert thr[j] == np.inf and np.isposinf(a).any() and (a == qc.F32_MAX).any()
        elif k == "ninf":
            assert thr[j] == -np.inf and np.isneginf(a).any() and np.isnan(a).any()
        elif k in ("neg_zero", "pos_zero"):
            assert thr[j] == 0 and np.signbit(thr[j]) == (k == "neg_zero")
            assert ((a == 0) & np.signbit(a)).any() and ((a == 0) & ~np.signbit(a)).any()
    # every position of the four cells a lane handles sees a midpoint that rounds down (a float32 compare would differ)
    for pos in range(4):
        assert any(k == "midpoint" and j % 4 == pos and np.float32(thr[j]) == anom[0, j] for j, k in enumerate(kinds))
    assert flips > 10
    # leading columns and rows are shared between widths and lengths
    for T in qc.MASK_T:
        wide = qc.mask_const_case(T, 1028)
        for C in qc.MASK_C:
            a, t, _ = qc.mask_const_case(T, C)
            n = min(C, 1028)
            assert np.array_equal(a[:, :n], wide[0][:, :n], equal_nan=True) and np.array_equal(t[:n], wide[1][:n], equal_nan=True)
            assert np.array_equal(a, qc.mask_const_case(130, C)[0][:T], equal_nan=True)
