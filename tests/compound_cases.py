"""What tests/test_compound_events_host.py and tests/test_gpu_compound_events.py share: the sizes at which the kernel can
go wrong, and the fields -- all from fixed seeds.  Not collected by pytest."""
import numpy as np

UNROLL = 8  # CMP_U of marex_compound.hip: rows loaded together
CELLS = [1, 3, 4, 63, 64, 65, 1027, 1028, 4100]  # one- and four-cell layouts, a partial wave, a partial last block, several blocks
TIMES = [1, 2, UNROLL - 1, UNROLL, UNROLL + 1, 97]
LAGS = [0, 1, 7, 30]
TOLERANCES = [0, 1, 30]
COVERAGES = [0.0, 0.05, 0.5, 1.0]


def chain(T, C, cover, seed, mean_run=4.0):
    """bool ``[T, C]``: per cell a two-state chain with the stationary coverage ``cover`` and runs of about ``mean_run``
    steps (shorter ones at high coverage are joined by short gaps); 0 and 1 give the empty and the full field."""
    if cover <= 0.0 or cover >= 1.0:
        return np.full((T, C), cover >= 1.0)
    rng = np.random.default_rng(seed)
    stop = 1.0 / mean_run
    start = min(1.0, stop * cover / (1.0 - cover))
    x = np.zeros((T, C), bool)
    on = rng.random(C) < cover
    for t in range(T):
        u = rng.random(C)
        on = np.where(on, u >= stop, u < start)
        x[t] = on
    return x


def shifted(a, k):
    """``b[t] = a[t - k]``: b follows a by ``k`` steps; the first ``k`` steps of b are absent."""
    b = np.zeros_like(a)
    if k < a.shape[0]:
        b[k:] = a[:a.shape[0] - k]
    return b


def pair(T, C, cover=0.5, seed=0, shift=None):
    """Two bool fields: independent chains, or the second the first shifted by ``shift`` steps."""
    a = chain(T, C, cover, 100 + seed)
    return a, (chain(T, C, cover, 200 + seed) if shift is None else shifted(a, shift))


def edge_pair(T, K, L, C=12):
    """Hand-made columns in front of a random rest, for a record of ``T >= 8 + 2 * max(K, L)`` steps: with the run
    ``[s, s + 2]`` of a, ``s = max(K, L) + 2``, b is present only
      0: at ``s + 2 + K`` (the last step that still meets the run)   1: at ``s + 3 + K`` (one too late)
      2: at ``s - K`` (the first step that meets it)                 3: at ``s - K - 1`` (one too early)
      4: at ``s + 2 + L`` (the largest lag from the run's end)       5: at ``s - L`` (the most negative from its start)
      6: a and b present throughout (one joint run over every window edge)
      7: two one-step runs of a at ``s`` and ``s + 2``, b at ``s + 3`` (both wait when b turns up, if ``K >= 3``)
      8: a present on the record's last step only, b on the step before (a run open at the end)
      9: a present on the record's first step, b on the last."""
    M = max(K, L)
    assert T >= 8 + 2 * M and C >= 10
    s = M + 2
    a, b = pair(T, C, 0.3, 5)
    a[:, :10] = b[:, :10] = False
    a[s:s + 3, :6] = True
    for col, t in enumerate((s + 2 + K, s + 3 + K, s - K, s - K - 1, s + 2 + L, s - L)):
        b[t, col] = True
    a[:, 6] = b[:, 6] = True
    a[[s, s + 2], 7] = True
    b[s + 3, 7] = True
    a[T - 1, 8] = b[T - 2, 8] = True
    a[0, 9] = b[T - 1, 9] = True
    return a, b


def mesh_classes(C, R, seed=3):
    """A shuffled class table with some cells at -1 and one at R (both counted nowhere)."""
    rng = np.random.default_rng(seed)
    cls = rng.integers(0, R, C).astype(np.int32)
    cls[rng.random(C) < 0.1] = -1
    cls[C - 1] = R
    cls[0] = -1
    return cls
