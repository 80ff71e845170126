"""GPU: the pooled threshold kernel (marex_hobday_thresholds_pool_f32: thresholds from the key lists, the histogram of a cell
summed over its pool of mesh neighbours) against tests/mesh_pool_oracle.py, bit for bit: thresholds, mask, n_true, range
statistics.  The cases cover 1, 2, 3 and 6 lists per bucket in 2 and 4 chunks, windows of 3, 11 and 31 days, both rings, the
two places the first chunks can wait (an LDS ring, global memory), several day blocks, an owned cell range
with members outside it, and quantiles low enough that first chunks do not decide the probes."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from marex_amd import binning, calendar  # noqa: E402
from marex_amd.engine import HotPath  # noqa: E402
from marex_amd.exceptions import ProcessingError  # noqa: E402
from mesh_pool_oracle import pooled_extremes, pooled_thresholds, ring_and_chords  # noqa: E402
from oracle import marex_oracle as orc  # noqa: E402

pytestmark = pytest.mark.gpu

C = 333          # not a multiple of 64: the last wave has 51 lanes beyond the cells
LAND, HALF, TIES, BEYOND = 5, 9, 6, 12

_fields, _expected = {}, {}


def field(years):
    """[T, 333] anomalies with a land cell, a cell whose record ends half way, a cell of ties, a cell beyond the table and
    NaN / +-inf sprinkles -- all of them neighbours of ordinary cells on the ring -- and the mesh."""
    if years not in _fields:
        rng = np.random.default_rng(100 + years)
        tm = calendar.daily_time_axis("2000-01-01", years * 365 + 3)
        cal = calendar.build_calendar(tm)
        anom = rng.normal(0, 0.8, (len(tm), C)).astype(np.float32)
        pick = rng.random(anom.shape)
        anom[pick < 0.01] = np.nan
        anom[(pick > 0.01) & (pick < 0.013)] = np.inf
        anom[(pick > 0.013) & (pick < 0.016)] = -np.inf
        anom[(pick > 0.016) & (pick < 0.02)] = 7.5
        anom[0] = np.where(np.isnan(anom[0]), np.float32(0.1), anom[0])   # ocean everywhere but LAND
        anom[:, LAND] = np.nan
        anom[len(tm) // 2:, HALF] = np.nan
        anom[:, TIES] = 0.25
        anom[:, BEYOND] = 7.0
        _fields[years] = (cal, anom, ring_and_chords(rng, C))
    return _fields[years]


def expected(years, pct, wd, rings, cells):
    key = (years, pct, wd, rings, cells)
    if key not in _expected:
        cal, anom, nbr = field(years)
        bt = binning.hobday_bins()
        _expected[key] = pooled_extremes(anom, cal.doy_out, pct / 100.0, wd, bt.edges, bt.centres, nbr, rings) if cells is None \
            else pooled_thresholds(anom, cal.doy_out, pct / 100.0, wd, bt.edges, bt.centres, nbr, rings, cells=cells)
    return _expected[key]


def run_pool(hot, years, pct, wd, list_rows, rings, opts=None, cells=None, table=None):
    cal, anom, nbr = field(years)
    bt = binning.hobday_bins()
    dcal = hot.upload_calendar(cal)
    ad = torch.from_numpy(anom).to(hot.device)
    tl = hot.tail_extract(ad, dcal, bt, list_rows=list_rows)
    tab = HotPath.pool_table(nbr, rings) if table is None else table
    pool = torch.from_numpy(tab).to(hot.device)
    hot.ctx.debug_counters(reset=True)
    with hot.ctx.options(**(opts or {})):
        t = hot.hobday_thresholds_pool(tl, ad, dcal, bt, pct / 100.0, wd, pool, cells=cells)
        m = hot.mask_ge_doy_tails(tl, ad, t["thr_doy_major"], dcal, bt, cells=cells)
        hot.sync()
    counters = hot.ctx.debug_counters(reset=True)
    return t, m, counters, tab


def check_whole(hot, years, pct, wd, list_rows, rings, opts=None):
    t, m, counters, tab = run_pool(hot, years, pct, wd, list_rows, rings, opts)
    exp_thr, exp_stats, exp_ext = expected(years, pct, wd, rings, None)
    thr = t["thr_doy_major"].cpu().numpy().T
    assert np.array_equal(thr, exp_thr, equal_nan=True), "thresholds differ from the oracle"
    assert np.array_equal(m["extreme"].cpu().numpy().astype(bool), exp_ext), "mask differs from the oracle"
    assert int(m["n_true"].item()) == int(exp_ext.sum())
    st = HotPath.decode_thr_stats(t["stats_dev"])
    assert st["n_too_low"] == exp_stats["n_too_low"] and st["n_too_high"] == exp_stats["n_too_high"]
    assert st["min"] == np.float32(exp_stats["min"]) and st["max"] == np.float32(exp_stats["max"])
    assert np.isnan(thr[LAND]).all() and np.isfinite(thr[BEYOND]).all()    # the cell beyond the table gets its neighbours' samples
    return counters, tab


def ring_of(counters):
    """1 when the workgroups kept the first chunks in LDS, 0 when they probed global memory (debug counters: [0] counts the
    workgroups with a ring, [2] all of them)."""
    assert counters[2] > 0 and counters[0] in (0, counters[2])
    return counters[0] // counters[2]


# 1 / 0 / None below: the first chunks are expected in LDS / read from global memory / where the pool sizes of the mesh decide.
# (years, list_rows) -> lists per bucket x chunks per list: (5, 32) 1 x 4, (15, 15) 1 x 2, (30, 15) 2 x 2, (30, 32) 1 x 4,
# (85, 15) 6 x 2, (85, 32) 3 x 4
CASES = [
    # years, pct, wd, list_rows, rings, options, 1 / 0: the first chunks are expected in LDS / read from global memory
    (5, 95.0, 11, 32, 1, {}, 1),                           # 11 x 4 x 1 lists
    (5, 90.0, 3, 32, 2, {"THR_POOL_RING": 1}, 1),
    (15, 95.0, 11, 15, 2, {"THR_POOL_RING": 1}, None),     # 11 x K x 1 lists: in LDS when the largest pool has at most 11 members
    (15, 99.0, 31, 15, 1, {"THR_POOL_RING": 0}, 0),
    (30, 95.0, 11, 15, 1, {"THR_POOL_RING": 1, "THR_POOL_BLOCKS": 7}, 1),   # 11 x 3..4 x 2 lists: a ring of more than 64 KiB
    (30, 95.0, 11, 32, 2, {"THR_POOL_BLOCKS": 3}, None),
    (30, 95.0, 11, 32, 2, {"THR_POOL_RING": 0, "THR_POOL_BLOCKS": 5}, 0),
    (30, 100.0, 11, 15, 1, {}, 1),
    (30, 95.0, 31, 15, 2, {"THR_POOL_RING": 1}, 0),        # 31 x 9..13 x 2 lists: no ring fits the LDS, asked for or not
    (85, 95.0, 3, 15, 1, {"THR_POOL_RING": 1}, 1),         # 3 x 4 x 6 lists
    (85, 95.0, 3, 32, 1, {"THR_POOL_RING": 0, "THR_POOL_BLOCKS": 2}, 0),
    (85, 98.0, 11, 15, 2, {}, 0),                          # 11 x 9..13 x 6 lists
]


@pytest.mark.parametrize("years,pct,wd,list_rows,rings,opts,ring", CASES,
                         ids=[f"{c[0]}y-p{c[1]:g}-wd{c[2]}-l{c[3]}-r{c[4]}-" + "-".join(f"{k[9:]}{v}" for k, v in c[5].items()) for c in CASES])
def test_pooled_thresholds_equal_the_oracle(hot, years, pct, wd, list_rows, rings, opts, ring):
    counters, tab = check_whole(hot, years, pct, wd, list_rows, rings, opts)
    assert tab.shape[0] > (2 if rings == 1 else 6)                        # the mesh does give pools of several members
    if ring is None:  # the wrapper's rule: the ring (1 KiB per list, padded to four) and the member indices within 128 KiB
        lists = wd * tab.shape[0] * -(-int(np.diff(field(years)[0].doy_start).max()) // list_rows)
        ring = int(tab.shape[0] * 256 + ((lists + 3) & ~3) * 1024 <= 128 * 1024 and opts.get("THR_POOL_RING", 1) != 0)
    assert ring_of(counters) == ring, counters
    blocks = opts.get("THR_POOL_BLOCKS")
    if blocks:
        assert counters[2] == blocks * ((C + 63) // 64) and counters[3] == 366 * ((C + 63) // 64)


@pytest.mark.parametrize("ring", [1, 0])
@pytest.mark.parametrize("years,list_rows,rings,wd", [(30, 32, 1, 11), (30, 15, 2, 3)])
def test_a_low_quantile_is_recounted_from_every_chunk(hot, years, list_rows, rings, wd, ring):
    """pct 60: 40 % of a window's samples lie above the quantile, far more than first chunks hold, so probes are decided by
    counting behind the saturated lists (debug counter 1)."""
    counters, _ = check_whole(hot, years, 60.0, wd, list_rows, rings, {"THR_POOL_RING": ring})
    assert counters[1] > 0, counters
    assert ring_of(counters) == ring


def test_owned_range_with_members_outside_it(hot):
    """cells = (64, 200): thresholds and mask for these cells only -- their pools reach cells on both sides (ring links at 64
    and 199, chords anywhere) -- and nothing else is written (the buffers start as 0xCD bytes)."""
    c0, c1 = 64, 200
    for years, wd, list_rows, rings, opts in [(30, 31, 15, 2, {}), (30, 11, 32, 1, {"THR_POOL_RING": 0, "THR_POOL_BLOCKS": 4})]:
        t, m, counters, tab = run_pool(hot, years, 95.0, wd, list_rows, rings, opts, cells=(c0, c1))
        mine = tab[:, c0:c1]
        assert ((mine >= 0) & ((mine < c0) | (mine >= c1))).any()
        exp_thr, exp_stats = expected(years, 95.0, wd, rings, (c0, c1))
        thr = t["thr_doy_major"].cpu().numpy().T
        assert np.array_equal(thr[c0:c1], exp_thr[c0:c1], equal_nan=True)
        poison = np.frombuffer(b"\xcd" * 4, dtype=np.float32)[0]
        assert (thr[:c0].view(np.uint32) == poison.view(np.uint32)).all() and (thr[c1:].view(np.uint32) == poison.view(np.uint32)).all()
        cal, anom, _ = field(years)
        exp_ext = orc.mask_ge_doy(anom[:, c0:c1], exp_thr[c0:c1], cal.doy_out)
        ext = m["extreme"].cpu().numpy()
        assert np.array_equal(ext[:, c0:c1].astype(bool), exp_ext) and int(m["n_true"].item()) == int(exp_ext.sum())
        assert (ext[:, :c0] == 0xCD).all() and (ext[:, c1:] == 0xCD).all()
        st = HotPath.decode_thr_stats(t["stats_dev"])
        assert st["n_too_low"] == exp_stats["n_too_low"] and st["n_too_high"] == exp_stats["n_too_high"]
        assert counters[3] == 366 * ((c1 - c0 + 63) // 64)


@pytest.mark.parametrize("years,list_rows,wd", [(30, 15, 11), (5, 32, 3), (85, 32, 11)])
def test_a_table_of_empty_slots_is_the_unpooled_kernel(hot, years, list_rows, wd):
    """Rows of -1 beyond row 0: every pool is the cell alone and the output equals k_thr_cells' (and the committed oracle)."""
    cal, anom, _ = field(years)
    tab = np.full((4, C), -1, dtype=np.int32)
    tab[0] = np.arange(C)
    t, m, _, _ = run_pool(hot, years, 95.0, wd, list_rows, 1, table=tab)
    bt = binning.hobday_bins()
    dcal = hot.upload_calendar(cal)
    ad = torch.from_numpy(anom).to(hot.device)
    tl = hot.tail_extract(ad, dcal, bt, list_rows=list_rows)
    with hot.ctx.options(THR_CELLS=2):
        u = hot.hobday_thresholds_tails(tl, ad, dcal, bt, 0.95, wd, 1, 0, C)
        hot.sync()
    a, b = t["thr_doy_major"].cpu().numpy(), u["thr_doy_major"].cpu().numpy()
    assert np.array_equal(a.view(np.uint32), b.view(np.uint32))
    assert torch.equal(t["stats_dev"], u["stats_dev"])
    exp_thr, _ = orc.hobday_thresholds_approx(anom, cal.doy_out, 0.95, wd, None, bt.edges, bt.centres, 0, 0)
    assert np.array_equal(a.T, exp_thr, equal_nan=True)


def test_a_bad_table_is_an_error_not_a_fault(hot):
    """Every index is checked on the host before the launch: the library answers -1 and the kernel does not run."""
    cal, anom, nbr = field(5)
    good = HotPath.pool_table(nbr, 1)
    for bad_value, where in [(C, (1, 40)), (-2, (2, 300)), (1 << 30, (1, C - 1)), (7, (0, 3))]:
        tab = good.copy()
        tab[where] = bad_value
        with pytest.raises(ProcessingError, match="marex_hobday_thresholds_pool_f32"):
            run_pool(hot, 5, 95.0, 11, 32, 1, table=tab)
    tab = good.copy()
    tab[1, 10] = C + 5                                      # outside the owned range: not read, not an error
    run_pool(hot, 5, 95.0, 11, 32, 1, table=tab, cells=(64, 200))
    with pytest.raises(ProcessingError, match="marex_hobday_thresholds_pool_f32"):
        run_pool(hot, 5, 95.0, 11, 32, 1, table=np.vstack([good[:1]] + [good[1:2]] * 13))   # 14 rows: more than two rings give
