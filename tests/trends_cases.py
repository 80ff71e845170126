"""The case tables shared by tests/test_cell_trends_host.py and tests/test_gpu_cell_trends.py: series of maps ``y [G, C]``
over abscissae ``x [G]``, seeded.  Not collected by pytest."""
import numpy as np

ALPHAS = (0.05, 0.01, 0.32)


def years(G, start=1982):
    return np.arange(start, start + G, dtype=np.float64)


def irregular_x(G, seed=5):
    """Increasing, irregularly spaced, not integers."""
    rng = np.random.default_rng(seed)
    return np.cumsum(rng.uniform(0.1, 2.7, G)) - 3.3


def mixed(G, C, seed, missing=0.15):
    """Every third cell small integer counts (most slopes coincide), every third a float series with a trend of either
    sign, every third a two-decimal series with ties; ``missing`` of the samples NaN, a few of them +-Inf."""
    rng = np.random.default_rng(seed)
    t = np.arange(G, dtype=np.float64)[:, None]
    counts = rng.poisson(3.0, (G, C)).astype(np.float64)
    trend = rng.normal(0, 1, (G, C)) + t * rng.normal(0, 0.2, (1, C))
    coarse = np.round(rng.normal(0, 0.4, (G, C)), 1)
    kind = np.arange(C) % 3
    y = np.where(kind == 0, counts, np.where(kind == 1, trend, coarse))
    gone = rng.random((G, C)) < missing
    y[gone] = np.nan
    y[gone & (rng.random((G, C)) < 0.1)] = np.inf
    y[gone & (rng.random((G, C)) < 0.05)] = -np.inf
    return y


def special(G, C=70, seed=11):
    """One cell per edge, the rest of the wave and the tail of a second wave filled with a different missing pattern in
    every lane.  ``G >= 4``."""
    rng = np.random.default_rng(seed)
    y = rng.normal(0, 1, (G, C))
    for c in range(C):  # lane c: its own pattern of missing steps
        y[(np.arange(G) * 2654435761 + c * 40503) % 7 < (c % 7), c] = np.nan
    y[:, 0] = np.nan                                # all samples missing
    y[:, 1] = np.nan
    y[G // 2, 1] = 1.5                              # exactly one valid
    y[:, 2] = np.nan
    y[1, 2], y[G - 2, 2] = 2.0, -1.0                # exactly two valid
    y[:, 3] = np.nan
    y[0, 3], y[G - 1, 3] = -3.0, 4.0                # valid only at the first and the last step
    y[:, 4] = 7.25                                  # constant
    y[:, 5] = np.where(np.arange(G) % 3 == 0, 1.0, 2.0)  # two values
    y[:, 6] = rng.integers(0, 4, G)                 # small counts
    y[:, 7] = np.where(np.arange(G) % 2 == 0, 0.0, -0.0)  # +-0.0 only
    y[:, 8] = np.where(np.arange(G) % 3 == 0, -0.0, rng.integers(-1, 2, G) * 1.0)  # +-0.0 among others
    y[:, 9] = 10.0 ** rng.integers(-30, 31, G) * rng.choice([-1.0, 1.0], G)  # 1e-30 .. 1e30, both signs
    y[:, 10] = np.arange(G) * -0.75 + 3                 # exact negative slope
    y[:, 11] = np.arange(G) * 1e-30                      # tiny slopes
    y[:, 12] = np.inf                                   # non-finite only: land
    y[::2, 13] = -np.inf                                # half missing through -Inf
    y[:, 14] = np.nan
    y[0, 14], y[1, 14], y[2, 14] = 1.0, 1.0, 1.0    # three equal: var 0 with n = 3
    return y


def shape_cases():
    """``(id, y, x)``: the cell counts at one G, the step counts at one C (at most 200 cells for the long ones)."""
    out = []
    for C in (1, 63, 64, 65, 257, 4001):
        out.append((f"cells{C}", mixed(40, C, 100 + C), years(40)))
    for G in (2, 3, 40, 64, 65, 128, 129, 256):
        out.append((f"steps{G}", mixed(G, 130, 200 + G), years(G) if G % 2 == 0 else irregular_x(G, G)))
    return out


def edge_cases():
    out = [(f"special{G}_{'irr' if irr else 'yr'}", special(G), irregular_x(G) if irr else years(G))
           for G, irr in ((4, False), (5, True), (12, False), (33, True), (130, False))]
    out.append(("nomissing_counts", np.random.default_rng(3).poisson(2.0, (40, 200)).astype(np.float64), years(40)))
    return out


def all_cases():
    return shape_cases() + edge_cases()


def rank_table(n, rng):
    """int32 ``[7, C]``: -1, P, 0, P - 1, the lower middle twice, and a random rank, also past the ends."""
    n = np.asarray(n).astype(np.int64)
    P = n * (n - 1) // 2
    mid = (P - 1) // 2
    return np.stack([np.full_like(P, -1), P, np.zeros_like(P), P - 1, mid, mid,
                     rng.integers(-3, P + 3)]).astype(np.int32)
