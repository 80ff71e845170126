"""What tests/test_event_composites_host.py and tests/test_gpu_event_composites.py share: the sizes at which the kernel can
go wrong, and the fields -- all from fixed seeds.  Not collected by pytest."""
import numpy as np

from compound_cases import chain  # noqa: F401  (the two-state chains of the compound-event tests)

UNROLL = 4  # CPS_U of marex_composites.hip: rows whose anchors are found together
CELLS = [1, 63, 64, 65, 257, 1028]  # a partial wave, a full one, one lane of a second, a second block, several blocks
LAGS = [0, 1, 7, 30]
TIMES = [1, 2, 3, UNROLL - 1, UNROLL, UNROLL + 1, 2 * UNROLL + 1, 14, 15, 16, 60, 61, 62]  # around the unroll depth and 2 L + 1
COVERAGES = [0.0, 0.04, 0.5, 1.0]
ANCHORS = ("onset", "end")


def values(T, C, seed, special=True):
    """float32 ``[T, C]`` with magnitudes spread over forty binades and both signs, so that the order of the additions shows
    in the bits of a float64 sum; ``special`` sprinkles NaN, +-inf and signed zeros."""
    rng = np.random.default_rng(1000 + seed)
    v = (rng.standard_normal((T, C)) * np.exp2(rng.integers(-20, 21, (T, C)))).astype(np.float32)
    if special:
        u = rng.random((T, C))
        v[u < 0.05] = np.nan
        v[(u >= 0.05) & (u < 0.07)] = np.inf
        v[(u >= 0.07) & (u < 0.09)] = -np.inf
        v[(u >= 0.09) & (u < 0.12)] = 0.0
        v[(u >= 0.12) & (u < 0.15)] = -0.0
    return v


# anchors of the hand-made columns of edge_field, whatever T >= 10
EDGE_ANCHORS = {"onset": [0, 1, 1, 2, 1, 0, 0, 1, 1, 1], "end": [1, 0, 1, 2, 1, 0, 0, 1, 1, 1]}


def edge_field(T, C=12, seed=5):
    """bool ``[T, C]``, ``T >= 10``, ``C >= 10``: hand-made columns in front of a random rest.
      0: a run from step 0 (``[0, 2]``): no onset, an end at 2         1: a run to ``T - 1`` (``[T - 3, T - 1]``): an onset, no end
      2: the run ``[1, T - 2]``: an onset at step 1, an end at ``T - 2``
      3: the runs ``[4, 5]`` and ``[7, 7]``, one absent step apart: two anchors in one unrolled batch, overlapping windows
      4: a one-step run at 5: onset and end on the same step          5: all present   6: none present
      7, 8: the runs ``[3, 5]`` and ``[3, 4]``: neighbouring cells with onsets on the same row
      9: present at step 0 and at step ``T - 1`` only: the onset at ``T - 1`` and the end at 0 count, the other two are censored."""
    assert T >= 10 and C >= 10
    x = chain(T, C, 0.3, seed)
    x[:, :10] = False
    x[0:3, 0] = True
    x[T - 3:, 1] = True
    x[1:T - 1, 2] = True
    x[4:6, 3] = x[7, 3] = True
    x[5, 4] = True
    x[:, 5] = True
    x[3:6, 7] = True
    x[3:5, 8] = True
    x[0, 9] = x[T - 1, 9] = True
    return x


def labels(T, G=4):
    """Groups that change inside an unrolled batch (every three steps)."""
    return (np.arange(T) // 3 % G).astype(np.int32)
