"""Hand-built columns and shapes of the heat stress tests, shared by tests/test_heat_stress_host.py (the two oracles against
each other and against the expectations written here) and tests/test_gpu_heat_stress.py (the kernel against both).  Not
collected by pytest."""
import numpy as np

F = np.float32
NAN, INF = F(np.nan), F(np.inf)
BELOW_ONE = np.nextafter(F(1), F(0))  # one ulp below hotspot_min = 1
TINY = F(2.0 ** -10)


def _case(name, d, m=0.0, expect=None, **kw):
    """A column given as differences ``d`` to ``m`` (m = 0 or a power of two keeps ``x - m == d`` exact)."""
    d = np.asarray(d, F)
    return {"name": name, "x": (d + F(m)).astype(F), "m": F(m), "kw": kw, "expect": expect or {}}


def columns():
    """The cases: ``x [T]`` float32, ``m``, the keyword arguments (``window``, ``hmin``, ``spw``, ``lev``, ``grp``, ``G``) and
    ``expect``: what a reader can check by hand -- ``alert`` (the class of every step), ``dhw`` ({step: value}) and entries
    of the summary of group 0."""
    c = []
    # d == hotspot_min counts (class 2), one ulp below does not (class 1, no HotSpot); d == 0 and d < 0 are class 0
    c.append(_case("hotspot_min_edge", [1.0, BELOW_ONE, 0.0, -0.5, 1.0], window=3, spw=1.0,
                   expect={"alert": [2, 1, 0, 0, 2], "dhw": {0: 1.0, 1: 1.0, 2: 1.0, 3: 0.0, 4: 1.0}, "hotspot_max": 1.0}))
    # fourteen steps of 2.0 at seven steps per week are exactly 4.0: Alert Level 1 on the fourteenth, Warning before
    c.append(_case("exactly_on_a_level", [2.0] * 14 + [0.5], m=16.0,
                   expect={"alert": [2] * 13 + [3, 1], "dhw": {12: F(26.0 / 7.0), 13: 4.0, 14: 4.0}, "onset": [13, -1],
                           "dhw_max": 4.0, "tmax": 13}))
    # a hot step leaves after exactly `window` steps without a residue, beside neighbours at both ends of the range
    c.append(_case("leaves_without_residue", [0.0, F(1023.99), F(3.3), TINY, 0.0, 0.0, 0.0, 0.0, 0.0], window=4, hmin=TINY, spw=3.0,
                   expect={"dhw": {4: F((float(F(1023.99)) + float(F(3.3)) + 2.0 ** -10) / 3.0), 5: F((float(F(3.3)) + 2.0 ** -10) / 3.0),
                                   6: F(2.0 ** -10 / 3.0), 7: 0.0, 8: 0.0}, "tmax": 3}))
    # NaN and +-Inf samples are invalid steps: class 255, nothing added, nothing removed when they leave
    c.append(_case("non_finite_samples", [2.0, NAN, INF, -INF, 2.0, 0.0], window=3, spw=1.0,
                   expect={"alert": [2, 255, 255, 255, 2, 0], "dhw": {0: 2.0, 2: 2.0, 3: 0.0, 4: 2.0, 5: 2.0}, "invalid": 3}))
    # a cell without mmm: a NaN column, class 255 throughout
    c.append({"name": "no_mmm", "x": np.array([29.0, 30.0, 31.0, NAN], F), "m": NAN, "kw": {"window": 2},
              "expect": {"alert": [255] * 4, "invalid": 4, "tmax": -1}})
    # |d| >= 1024 is not valid, on either side; 1023.5 is
    c.append(_case("difference_out_of_range", [1024.0, -1024.0, -2000.0, 1023.5, -1023.5], window=5, spw=1.0,
                   expect={"alert": [255, 255, 255, 4, 0], "dhw": {4: 1023.5}, "invalid": 3, "hotspot_max": 1023.5}))
    # the maximum is attained at steps 1 and 5: the first wins
    c.append(_case("maximum_twice", [0.0, 3.0, 0.0, 0.0, 0.0, 3.0, 0.0], window=2, spw=1.0, expect={"dhw_max": 3.0, "tmax": 1}))
    # group 1 holds no valid step; group 2 holds no step at all
    c.append(_case("group_without_valid_step", [2.0, 2.0, NAN, NAN, 2.0], window=2, spw=1.0, grp=[0, 0, 1, 1, 0], G=3))
    # no levels: the classes end at 2
    c.append(_case("no_levels", [5.0] * 6 + [0.5], window=84, lev=(), expect={"alert": [2] * 6 + [1]}))
    # negative throughout: hotspot_max is negative, dhw stays 0
    c.append(_case("always_below", [-3.0, -1.5, -2.0], m=32.0, expect={"hotspot_max": -1.5, "dhw_max": 0.0, "tmax": 0, "alert": [0, 0, 0]}))
    return c


def in_a_row(case, C=65, at=37, seed=3):
    """The column as cell ``at`` of a row of ``C`` cells with seeded neighbours: ``(x [T, C], m [C])``."""
    rng = np.random.default_rng(seed)
    T = case["x"].size
    x, m = field(T, C, rng)
    x[:, at], m[at] = case["x"], case["m"]
    return x, m


def field(T, C, rng, nan_share=0.03):
    """A seeded SST-like field in degrees Celsius around a per-cell mmm: ``(x [T, C], m [C])`` with hot spells, NaN and
    Inf samples and a few cells without mmm."""
    m = rng.uniform(24.0, 31.0, C).astype(F)
    x = (m[None, :] + rng.normal(0.0, 1.2, (T, C))).astype(F)
    x[rng.random((T, C)) < nan_share] = NAN
    if T * C > 8:
        x.reshape(-1)[rng.integers(0, T * C, 2)] = [INF, -INF]
        m[rng.integers(0, C, max(1, C // 40))] = NAN
    return x, m


C_EDGES = (1, 3, 63, 64, 65, 255, 256, 257, 1021)
WINDOWS = (1, 2, 7, 84, 366)


def t_edges(window):
    return sorted({1, max(window - 1, 1), window, window + 1, 2 * window + 3})
