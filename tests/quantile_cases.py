"""Seeded cases for the quantile kernels (csrc/marex_quantiles.hip: k_hobday_exact, k_global_exact, k_global_approx,
k_global_exact16, k_global_approx16) and the constant-threshold mask (csrc/marex_mask.hip: k_mask_ge_const,
k_mask_ge_const4): plain NumPy, no device.  Not a test module.

Every builder is a pure function of its arguments (fixed seeds), returns float32 fields laid out ``[T, C]`` as the kernels
take them, and names what each column is for.  tests/test_quantile_cases_host.py checks that the cases are what they claim
to be; tests/test_gpu_quantile_edges.py runs them on the device against the oracle.
"""
import functools
from types import SimpleNamespace

import numpy as np

from marex_amd import binning, calendar

#: smallest positive float32 subnormal
TINY = np.float32(1e-45)
F32_MAX = np.finfo(np.float32).max

#: columns of ``global_columns``: 64 + 2 lanes of the 64-lane kernels, 32 + 32 + 2 of the 32-lane k_global_approx
GLOBAL_C = 66


def _shuffled(rng, v):
    v = np.asarray(v, dtype=np.float32).copy()
    rng.shuffle(v)
    return v


def _fill(pattern, T):
    """``pattern`` repeated to T entries."""
    pattern = np.asarray(pattern, dtype=np.float32)
    return np.tile(pattern, T // pattern.size + 1)[:T]


def _edge_neighbours(gb):
    """float32(edge), the float32 above it and the float32 below it, for every finite edge of the table."""
    e = gb.edges[1:].astype(np.float32)
    return np.stack([e, np.nextafter(e, np.float32(np.inf)), np.nextafter(e, np.float32(-np.inf))], axis=1).reshape(-1)


# one builder per column kind: f(rng, T, gb) -> float32 [T]
def _k_const(rng, T, gb):
    """All samples 1.5: one uint16 counter takes all T counts in each of the four radix passes (0xFFFF at T = 65 535);
    rank lo + 1 is another copy of a."""
    return np.full(T, 1.5, np.float32)


def _k_one_larger(rng, T, gb):
    """T - 1 copies of 0.75 and one larger sample: at pct 100 `hi` is the first sample after the copies."""
    v = np.full(T, 0.75, np.float32)
    v[-1] = 2.5
    return _shuffled(rng, v)


def _k_one_smaller(rng, T, gb):
    """T - 1 copies of 0.75 and one smaller sample: `below` is 1 while one counter holds T - 1."""
    v = np.full(T, 0.75, np.float32)
    v[-1] = -2.5
    return _shuffled(rng, v)


def _k_low_byte(rng, T, gb):
    """1 + k * 2^-23, k = 0..255 repeated: three radix passes put every sample in one bucket, the last spreads them over
    all 256; neighbouring ranks differ in the lowest key byte only."""
    return _shuffled(rng, _fill(np.float32(1) + np.arange(256, dtype=np.float32) * np.float32(2.0 ** -23), T))


def _k_subnormals(rng, T, gb):
    """+-smallest subnormal and +-0.0 in equal shares: neighbours either side of the sign change of ordered_key."""
    return _shuffled(rng, _fill([TINY, -TINY, 0.0, -0.0], T))


def _k_zeros(rng, T, gb):
    """Half -0.0, half +0.0: equal as floats, different keys."""
    return _shuffled(rng, _fill([-0.0, 0.0], T))


def _k_inf_ends(rng, T, gb):
    """Normal samples with +inf on top and -inf at the bottom (first and last radix bucket)."""
    v = rng.normal(0, 1, T).astype(np.float32)
    v[0] = np.inf
    if T > 1:
        v[1] = -np.inf
    return _shuffled(rng, v)


def _k_rounded(rng, T, gb):
    """Normal samples rounded to integers: long runs of ties around every rank."""
    return np.round(rng.normal(0, 1.5, T)).astype(np.float32)


def _k_normal(rng, T, gb):
    """Plain normal samples."""
    return rng.normal(0, 1, T).astype(np.float32)


def _k_nan30(rng, T, gb):
    """Normal samples, a random 30 % NaN: m differs from T."""
    v = rng.normal(0, 1, T).astype(np.float32)
    v[rng.random(T) < 0.3] = np.nan
    return v


def _k_one_sample(rng, T, gb):
    """All NaN but one sample: m = 1."""
    v = np.full(T, np.nan, np.float32)
    v[int(rng.integers(T))] = 0.625
    return v


def _k_all_nan(rng, T, gb):
    """All NaN: m = 0, the threshold is NaN."""
    return np.full(T, np.nan, np.float32)


def _k_one_bin(rng, T, gb):
    """Approximate method: every sample 0.0, all mass in one interior bin."""
    return np.zeros(T, np.float32)


def _k_below(rng, T, gb):
    """Approximate method: every sample below edges[1] (bin 0, whose centre is 0)."""
    return np.full(T, np.float32(gb.edges[1]) - np.float32(1), np.float32)


def _k_last_edge(rng, T, gb):
    """Approximate method: every sample equal to the last edge (closed last bin; the default 5.0 is a float32)."""
    return np.full(T, gb.edges[-1], np.float32)


def _k_beyond(rng, T, gb):
    """Approximate method: every sample beyond the last edge: nothing is counted."""
    return np.full(T, np.float32(gb.edges[-1]) * np.float32(2), np.float32)


def _k_edges(rng, T, gb):
    """float32(edge) and its float32 neighbours above and below, for every finite edge, repeated to fill T (in edge order:
    a short series holds the lowest edges)."""
    return _fill(_edge_neighbours(gb), T)


GLOBAL_KINDS = {
    "const": _k_const, "one_larger": _k_one_larger, "one_smaller": _k_one_smaller, "low_byte": _k_low_byte,
    "subnormals": _k_subnormals, "zeros": _k_zeros, "inf_ends": _k_inf_ends, "rounded": _k_rounded, "normal": _k_normal,
    "nan30": _k_nan30, "one_sample": _k_one_sample, "all_nan": _k_all_nan, "one_bin": _k_one_bin, "below": _k_below,
    "last_edge": _k_last_edge, "beyond": _k_beyond, "edges": _k_edges,
}


@functools.lru_cache(maxsize=None)
def global_columns(T, precision=0.01, max_anomaly=5.0):
    """``(field [T, 66] float32, names)``: the 17 kinds of GLOBAL_KINDS, repeated with fresh seeds until the 66 columns are
    full (every kind at three or four lanes; the last two columns are lanes of a second workgroup).  The columns for the
    approximate method are placed on the bin table ``global_bins(precision, max_anomaly)``.  Read-only."""
    gb = binning.global_bins(precision, max_anomaly)
    kinds = list(GLOBAL_KINDS)
    names = [kinds[j % len(kinds)] for j in range(GLOBAL_C)]
    x = np.empty((T, GLOBAL_C), np.float32)
    for j, k in enumerate(names):
        x[:, j] = GLOBAL_KINDS[k](np.random.default_rng([17, T, j]), T, gb)
    x.setflags(write=False)
    return x, tuple(names)


#: percentiles of the rank sweep: (m - 1) q is an integer for m = 33 (5 and 31), has a fraction of exactly 0.5 for m = 17
#: (2.5 and 15.5) and fractions either side of 0.5 for the other m
SWEEP_PCTS = (0.0, 100.0 * 5 / 32, 50.0, 96.875, 100.0)
SWEEP_M_MAX = (33, 65)


@functools.lru_cache(maxsize=None)
def rank_sweep(m_max):
    """``[m_max, m_max + 1]`` float32: column j starts with j NaNs, so column j has m = m_max - j samples and one launch
    covers every m from m_max down to 0.  Use with SWEEP_PCTS."""
    rng = np.random.default_rng([23, m_max])
    x = rng.normal(0, 1, (m_max, m_max + 1)).astype(np.float32)
    for j in range(m_max + 1):
        x[:j, j] = np.nan
    x.setflags(write=False)
    return x


TIE_N = 16
#: pct 0, 50 and 100 k / 15: (m - 1) q visits every rank of the 16 samples
TIE_PCTS = tuple(sorted({0.0, 50.0} | {100.0 * k / 15 for k in range(16)}))
#: (a, b), a before b in key order: lowest key byte apart; across the sign change; -0.0 / +0.0 (equal floats, two keys);
#: far apart; largest finite next to +inf
TIE_PAIRS = (
    (np.float32(1.0), np.nextafter(np.float32(1.0), np.float32(2.0))),
    (-TINY, TINY),
    (np.float32(-0.0), np.float32(0.0)),
    (np.float32(-1.5), np.float32(2.25)),
    (F32_MAX, np.float32(np.inf)),
)


@functools.lru_cache(maxsize=None)
def tie_sweep():
    """``(field [16, 17 * len(TIE_PAIRS)], splits)``: column ``p * 17 + n_a`` is ``[a] * n_a + [b] * (16 - n_a)`` of pair p,
    shuffled; ``splits[col] = (p, n_a)``.  Over TIE_PCTS rank lo + 1 falls on the last copy of a (hi = n_a - 1), on the first
    b (hi = n_a) and everywhere between: the two sides of `hi >= below + n_final` in k_global_exact16."""
    rng = np.random.default_rng(29)
    cols, splits = [], []
    for p, (a, b) in enumerate(TIE_PAIRS):
        for n_a in range(TIE_N + 1):
            cols.append(_shuffled(rng, [a] * n_a + [b] * (TIE_N - n_a)))
            splits.append((p, n_a))
    x = np.stack(cols, axis=1)
    x.setflags(write=False)
    return x, tuple(splits)


def rank_indices(m, pct):
    """``(lo, hi, g)`` of NumPy's linear method for m samples, float64 q (what the global kernels compute)."""
    virt = (m - 1) * (pct / 100.0)
    lo = int(np.floor(virt))
    if lo >= m - 1:
        return m - 1, m - 1, virt - lo
    return lo, lo + 1, virt - lo


#: bins the landing cases put their mass in (default table: bin k = [0.01 (k - 2), 0.01 (k - 1)))
LAND_A, LAND_NEAR, LAND_FAR, LAND_LOW = 52, 53, 352, 12


@functools.lru_cache(maxsize=None)
def cdf_landings():
    """Cases for the CDF rule of the approximate kernels: namespaces with ``T, pct, field [T, ncols], names, branch``.

    With n = q T samples at or below bin A the CDF at A is n / (T + 1e-10), within the rule's 1e-10 of q: the first
    search stops at A and `|cl - q| < eps` holds (branch "exact", the threshold is the centre of A).  One sample fewer
    ("-1") and the search passes on to the next occupied bin B; one more ("+1") and it stops at A with the CDF above q.  The
    second search then finds the same bin, so cl = cu (branch "zero": one centre, as the mean of itself) -- unless B is
    the last bin, where `il` is clamped to the bin before it and the rule interpolates (branch "interp").  B is the bin
    next to A, 300 bins away, or the last; "_low" moves one sample from A to a bin far below, so the CDF below A is not 0.
    ``branch[j]`` is what the host test must find for column j from the oracle's intermediate values."""
    gb = binning.global_bins()
    mid = lambda k: np.float32((gb.edges[k] + gb.edges[k + 1]) / 2)  # noqa: E731
    out = []
    for T in (20, 40, 100, 200):
        for pct in (95.0, 50.0):
            n = int(round(pct / 100.0 * T))
            assert n * 100 == pct * T
            cols, names, branch = [], [], []
            rng = np.random.default_rng([31, T, int(pct)])
            for where, B in (("near", LAND_NEAR), ("far", LAND_FAR), ("last", gb.nb - 1)):
                for delta in (-1, 0, 1):
                    for low in (0, 1):
                        cols.append(_shuffled(rng, [mid(LAND_LOW)] * low + [mid(LAND_A)] * (n + delta - low)
                                              + [mid(B)] * (T - n - delta)))
                        names.append(f"{where}{delta:+d}{'_low' if low else ''}")
                        branch.append("exact" if delta == 0 else ("interp" if where == "last" and delta < 0 else "zero"))
            f = np.stack(cols, axis=1)
            f.setflags(write=False)
            out.append(SimpleNamespace(T=T, pct=pct, field=f, names=tuple(names), branch=tuple(branch)))
    return tuple(out)


# ------------------------------------------------------------------------------------------------------------------------
# exact Hobday percentile
# ------------------------------------------------------------------------------------------------------------------------
HOBDAY_START = "2000-01-01"
LDS_LIMIT = 64 * 1024
LDS_ATTRIBUTE = 48 * 1024


def hobday_days(years):
    return years * 365 + 3


@functools.lru_cache(maxsize=None)
def hobday_calendar(years):
    return calendar.build_calendar(calendar.daily_time_axis(HOBDAY_START, hobday_days(years)))


def max_window_rows(cal, wd):
    """Most timesteps any wrapped wd-day window of days of the year holds (HotPath.hobday_thresholds_exact, engine.py:
    ``nd`` ... ``max_rows``)."""
    nd = np.diff(cal.doy_start).astype(np.int64)
    return max(int(sum(nd[(d + o) % nd.size] for o in range(-(wd // 2), wd // 2 + 1))) for d in range(nd.size))


def hobday_sizing(max_rows, pct):
    """``(K, BT, lds_bytes)`` as marex_hobday_exact_f32 sizes its launch (csrc/marex_quantiles.hip, the lines from
    ``const int upper = q >= 0.5;`` to the ``lds > 64 * 1024`` refusal): q is the float32 quotient pct / 100 widened to
    double, K = ceil(tail * max_rows) + 4 clamped to max_rows, the workgroup halves from 256 while K * BT * 4 exceeds
    64 KiB and BT > 64.  ``lds_bytes > LDS_LIMIT`` means the call is refused (-4)."""
    q = float(np.float32(pct) / np.float32(100))
    tail = (1.0 - q) if q >= 0.5 else q
    K = int(np.ceil(tail * max_rows)) + 4
    K = min(K, max_rows)
    BT = 256
    while BT > 64 and K * BT * 4 > LDS_LIMIT:
        BT >>= 1
    return K, BT, K * BT * 4


HOBDAY_KINDS = ("normal", "rounded", "const", "zeros", "inf_ends", "all_nan", "nan10", "nan50", "nan90", "one_sample")
HOBDAY_C = (1, 63, 65, 130)
HOBDAY_FIRST = {3: "nan50", 12: "normal", 13: "rounded"}


def hobday_cases():
    """``(years, wd, pct)`` with the ``(max_rows, K, BT, lds)`` class each must land in (pinned by the host test), what it
    reaches, and the cell counts to run it at (C = 130 costs the NumPy oracle seconds: two cases only).  Series start on
    2000-01-01 and have years * 365 + 3 days; the 3-year series has four 1 and 2 January, and day 366 has one sample."""
    N = SimpleNamespace
    small = HOBDAY_C[:3]
    return (
        N(years=12, wd=11, pct=50.0, max_rows=132, K=70, BT=128, lds=35840, Cs=small, reaches="first halving; median, default window"),
        N(years=12, wd=31, pct=70.0, max_rows=372, K=116, BT=128, lds=59392, Cs=HOBDAY_C, reaches="> 48 KiB attribute branch"),
        N(years=12, wd=31, pct=30.0, max_rows=372, K=116, BT=128, lds=59392, Cs=small, reaches="same, lower tail (negated keys)"),
        N(years=12, wd=31, pct=50.0, max_rows=372, K=190, BT=64, lds=48640, Cs=small, reaches="second halving, below 48 KiB"),
        N(years=13, wd=31, pct=50.0, max_rows=403, K=206, BT=64, lds=52736, Cs=HOBDAY_C, reaches="BT = 64 and > 48 KiB"),
        N(years=17, wd=31, pct=50.0, max_rows=527, K=268, BT=64, lds=68608, Cs=(8,), reaches="refusal (-4)"),
        N(years=3, wd=1, pct=50.0, max_rows=4, K=4, BT=256, lds=4096, Cs=small, reaches="K = 6 clamped to the 4-row window"),
        N(years=3, wd=1, pct=0.0, max_rows=4, K=4, BT=256, lds=4096, Cs=small, reaches="K = the whole window, lowest sample"),
        N(years=3, wd=1, pct=100.0, max_rows=4, K=4, BT=256, lds=4096, Cs=small, reaches="K = the whole window, highest sample"),
    )


def hobday_refused(case):
    return case.lds > LDS_LIMIT


@functools.lru_cache(maxsize=None)
def hobday_field(years, C):
    """``(field [years * 365 + 3, C] float32, names)``: the kinds of HOBDAY_KINDS in turn, starting at HOBDAY_FIRST[years]
    so that the single column of C = 1 differs between series lengths.  The NaN shares take m from far below K to the
    full window."""
    T = hobday_days(years)
    first = HOBDAY_KINDS.index(HOBDAY_FIRST.get(years, "normal"))
    names = tuple(HOBDAY_KINDS[(j + first) % len(HOBDAY_KINDS)] for j in range(C))
    x = np.empty((T, C), np.float32)
    for j, k in enumerate(names):
        rng = np.random.default_rng([37, years, j])
        v = rng.normal(0, 1, T).astype(np.float32)
        if k == "rounded":       # ties at the K boundary and around the two ranks
            v = np.round(v * 2) / 2
        elif k == "const":
            v[:] = 1.5
        elif k == "zeros":
            v = _shuffled(rng, _fill([0.0, -0.0], T))
        elif k == "inf_ends":
            v[int(rng.integers(T))] = np.inf
            v[int(rng.integers(T))] = -np.inf
        elif k == "all_nan":
            v[:] = np.nan
        elif k.startswith("nan"):
            v[rng.random(T) < int(k[3:]) / 100.0] = np.nan
        elif k == "one_sample":
            keep = int(rng.integers(T))
            v[np.arange(T) != keep] = np.nan
        x[:, j] = v
    x.setflags(write=False)
    return x, names


# ------------------------------------------------------------------------------------------------------------------------
# constant-threshold mask
# ------------------------------------------------------------------------------------------------------------------------
MASK_C = (4, 64, 1028, 1, 65, 1027)
MASK_T = (1, 3, 63, 64, 65, 67, 130)
MASK_KINDS = ("midpoint", "equal", "nan", "pinf", "ninf", "neg_zero", "pos_zero")


@functools.lru_cache(maxsize=None)
def _mask_column(j):
    """``(threshold float64, anomalies float32 [max(MASK_T)])`` of column j: a function of j alone, so fields of different
    widths share their leading columns and fields of different lengths their leading rows."""
    rng = np.random.default_rng([41, j])
    kind = MASK_KINDS[j % len(MASK_KINDS)]
    n = max(MASK_T)
    v = np.float32(rng.normal(0, 2))
    up, dn = np.nextafter(v, np.float32(np.inf)), np.nextafter(v, np.float32(-np.inf))
    specials = [np.float32(s) for s in (np.nan, np.inf, -np.inf, 0.0, -0.0)]
    if kind == "midpoint":    # strictly between two float32 neighbours: rounding it to float32 moves it onto one of them
        thr, pool = (float(v) + float(up)) / 2, [v, up, dn]
    elif kind == "equal":
        thr, pool = float(v), [v, up, dn]
    elif kind == "nan":
        thr, pool = float("nan"), [v] + specials
    elif kind == "pinf":
        thr, pool = float("inf"), [v, F32_MAX] + specials
    elif kind == "ninf":
        thr, pool = float("-inf"), [v, -F32_MAX] + specials
    elif kind == "neg_zero":
        thr, pool = -0.0, [np.float32(0.0), np.float32(-0.0), TINY, -TINY]
    else:
        thr, pool = 0.0, [np.float32(0.0), np.float32(-0.0), TINY, -TINY]
    # the pool in order first (T = 1 and 3 see the neighbours), then random picks from the pool and plain samples
    a = np.where(rng.random(n) < 0.7, rng.choice(np.array(pool, np.float32), n), rng.normal(0, 2, n).astype(np.float32))
    a[:len(pool)] = pool
    return thr, a.astype(np.float32)


@functools.lru_cache(maxsize=None)
def mask_const_case(T, C):
    """``(anom [T, C] float32, thr [C] float64, kinds)``; column j of every case is `_mask_column(j)` cut to T rows."""
    cols = [_mask_column(j) for j in range(C)]
    anom = np.ascontiguousarray(np.stack([a[:T] for _, a in cols], axis=1))
    thr = np.array([t for t, _ in cols], np.float64)
    anom.setflags(write=False)
    thr.setflags(write=False)
    return anom, thr, tuple(MASK_KINDS[j % len(MASK_KINDS)] for j in range(C))


def mask_const_cases():
    """Every (T, C) of MASK_T x MASK_C: widths that are multiples of 4 (k_mask_ge_const4) and widths that are not
    (k_mask_ge_const), lengths around the 64 rows of a block and the 4 rows in flight."""
    return tuple((T, C) for C in MASK_C for T in MASK_T)
