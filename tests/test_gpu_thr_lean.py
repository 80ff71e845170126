"""GPU: the lean instance of the list threshold kernel (k_thr_tails<.., 6, 2>, option THR_LEAN) against the general body
(THR_LEAN=0) and against the oracle.

Lists come from marex_tail_extract_f32 with 15-row lists on 85 years of daily anomalies, so the geometry is the headline's
6 lists of 2 chunks per bucket.  The grid is the smallest with both kinds of tile seam: 64 rows x 60 columns = three tile
rows (28 + 28 + 8 output rows) and three tile columns (28 + 28 + 4), the longitude wrap goes through the halo, the last row
and column of tiles are partial.

Every case compares, on the WHOLE grid and for equality, the thresholds, the raw marex_thr_stats words and the debug counters
(rebuilds, straggler passes, tile-days) of the two bodies.  The oracle is NumPy and dense: the whole grid takes it over a
minute per case, so it is asked for the two rows on either side of the first tile-row seam (rows 27 and 28) and for rows 55..63
(the second seam, the partial last row of tiles, the grid's edge), all 60 columns of each: every tile column, both column
seams, the wrap.  It is asked through its own stages on the slabs those rows pool over -- the same calls, in the same order, as
orc.hobday_thresholds_approx makes for a block of rows.  Each case puts its feature on the first seam.
"""
import numpy as np
import pytest
import torch

from marex_amd import binning, calendar
from oracle import marex_oracle as orc

pytestmark = pytest.mark.gpu

NY, NX, WD, WS = 64, 60, 11, 5
NDAYS = 85 * 365 + 21             # 85 years: buckets of 85 rows (6 lists of 15), the 29 February bucket holds 21 (lists 2..5 empty)
SEAM = (27, 29)                   # output rows compared with the oracle
SLAB = (SEAM[0] - WS // 2, SEAM[1] + WS // 2)
FOOT = (55, 64)                   # and the second seam (55 | 56), the partial last row of tiles, the grid's last rows
FOOT_SLAB = (FOOT[0] - WS // 2, NY)


@pytest.fixture(scope="module")
def world():
    """Shared, read-only: the base field (sigma 0.8 K noise), the two calendars and a cache of what cases can share."""
    rng = np.random.default_rng(20)
    w = {"base": rng.normal(0, 0.8, (NDAYS, NY * NX)).astype(np.float32), "bt": binning.hobday_bins(), "cal": {}, "dev": {}}
    for start in ("1925-01-01", "1925-07-01"):
        w["cal"][start] = calendar.build_calendar(calendar.daily_time_axis(start, NDAYS))
        assert w["cal"][start].T_out == NDAYS and int(np.diff(w["cal"][start].doy_start).max()) == 85
    yield w
    w.clear()


def _stationary(a, cal):
    pass


def _seasonal(a, cal):
    """sigma 0.1 .. 1.56 K over the year: the 95th percentile swings by 1.645 * 1.46 = 2.4 K, 120 bins, two bands."""
    amp = 1.0375 + 0.9125 * np.sin(2 * np.pi * (cal.doy_out.astype(np.float64) - 40) / 366.0)
    a *= amp[:, None].astype(np.float32)


def _step(a, cal):
    """+1.5 K (75 bins, more than a band) on columns 10..27 of the first tile column: no band holds both sides."""
    a.reshape(-1, NY, NX)[:, :, 10:28] += np.float32(1.5)


def _land(a, cal):
    f = a.reshape(-1, NY, NX)
    f[:, 0:28, 0:14] = np.nan            # tile (0, 0): half land
    f[:, 28:56, 28:56] = np.nan          # tile (1, 1): all land, the tile leaves early
    f[3650:4745, 27, 30:40] = np.nan     # ocean cells with three NaN years: smaller windows, same path
    f[0:400, 28, 0:6] = np.nan           # first kept row NaN: land by the reference's rule, although samples follow


def _beyond(a, cal):
    pick = np.random.default_rng(21).random(a.shape, dtype=np.float32)
    a[pick < 0.004] = np.float32(7.5)    # beyond the table: no key, not counted, flagged in aux
    a[pick > 0.998] = np.float32(-9.0)   # below the first edge: bin 0


FIELDS = {"stationary": _stationary, "seasonal": _seasonal, "step": _step, "land": _land, "beyond": _beyond}


def _device_field(hot, world, field, start, list_rows):
    """(anomalies on the device, calendar, lists, host copy of the oracle slab's columns); the stationary field is kept."""
    key = (field, start, list_rows)
    if key in world["dev"]:
        return world["dev"][key]
    cal = world["cal"][start]
    a = world["base"].copy()
    FIELDS[field](a, cal)
    dcal = hot.upload_calendar(cal)
    ad = torch.from_numpy(a).to(hot.device)
    tl = hot.tail_extract(ad, dcal, world["bt"], list_rows=list_rows)
    hot.sync()
    assert tuple(tl["tails"].shape[1:3]) == ((6, 2) if list_rows == 15 else (3, 4)), tl["tails"].shape   # lists x chunks
    out = (ad, dcal, cal, tl, (np.ascontiguousarray(a[:, SLAB[0] * NX:SLAB[1] * NX]), np.ascontiguousarray(a[:, FOOT_SLAB[0] * NX:])))
    if field == "stationary":
        world["dev"][key] = out
    return out


def _oracle_rows(world, key, slab_vals, cal, q, SEAM=SEAM, SLAB=SLAB):
    """Thresholds [rows * NX, 366] of rows SEAM: the stages of orc.hobday_thresholds_approx on the slab the rows pool over."""
    bt = world["bt"]
    key = key + (SEAM,)
    pooled = world["dev"].get(("pooled",) + key)
    if pooled is None:
        hb = orc.doy_bin_counts(orc.digitize_bins(slab_vals, bt.edges), cal.doy_out, bt.nb)
        hb = orc.spatial_pool(hb, SLAB[1] - SLAB[0], NX, WS)
        pooled = hb.reshape(SLAB[1] - SLAB[0], NX, orc.N_DOY, bt.nb)[SEAM[0] - SLAB[0]:SEAM[1] - SLAB[0]].reshape(-1, orc.N_DOY, bt.nb)
        pooled = np.ascontiguousarray(pooled)
        if key[0] == "stationary" and SEAM[1] - SEAM[0] <= 2:
            world["dev"][("pooled",) + key] = pooled
    thr = orc.rolling_histogram_quantile(pooled, WD, q, bt.centres)
    first = slab_vals[0].reshape(SLAB[1] - SLAB[0], NX)[SEAM[0] - SLAB[0]:SEAM[1] - SLAB[0]].reshape(-1)
    thr[np.isnan(first)] = np.nan
    with np.errstate(invalid="ignore"):
        thr = np.where(thr < bt.edges[3], bt.edges[3], thr).astype(np.float32)
    return thr


def _run(hot, ad, dcal, tl, bt, q, lean, opts):
    hot.ctx.debug_counters(reset=True)
    with hot.ctx.options(THR_LEAN=lean, **opts):
        t = hot.hobday_thresholds_tails(tl, ad, dcal, bt, q, WD, WS, NY, NX)
        hot.sync()
    counters = hot.ctx.debug_counters(reset=True)
    return t["thr_doy_major"].cpu().numpy().copy(), t["stats_dev"].cpu().numpy().view(np.uint32).copy(), counters


CASES = [
    # id, field, calendar start, q, options, rows per list
    ("stationary-q95", "stationary", "1925-01-01", 0.95, {}, 15),
    ("stationary-q100", "stationary", "1925-01-01", 1.0, {}, 15),
    ("stationary-q60-deeper-chunks", "stationary", "1925-01-01", 0.6, {}, 15),
    ("seasonal-rebuilds", "seasonal", "1925-01-01", 0.95, {"THR_DD": 366}, 15),
    ("step-stragglers", "step", "1925-01-01", 0.95, {}, 15),
    ("land-and-nan-years", "land", "1925-01-01", 0.95, {}, 15),
    ("series-from-mid-year", "stationary", "1925-07-01", 0.95, {}, 15),
    ("beyond-the-table", "beyond", "1925-01-01", 0.95, {}, 15),
    ("day-blocks-of-100", "stationary", "1925-01-01", 0.95, {"THR_DD": 100}, 15),   # blocks start at days 0 (the window wraps
                                                                                   # below day 0), 100, 200 and 300 (above 365)
    ("lists-of-32-rows-general-body", "stationary", "1925-01-01", 0.95, {}, 32),    # 3 lists of 4 chunks: not a lean geometry
]


@pytest.mark.parametrize("name,field,start,q,opts,list_rows", CASES, ids=[c[0] for c in CASES])
def test_lean_instance_equals_general_body_and_oracle(hot, world, name, field, start, q, opts, list_rows):
    bt = world["bt"]
    ad, dcal, cal, tl, slab_vals = _device_field(hot, world, field, start, list_rows)
    thr1, st1, c1 = _run(hot, ad, dcal, tl, bt, q, 1, opts)
    thr0, st0, c0 = _run(hot, ad, dcal, tl, bt, q, 0, opts)
    print(f"{name}: rebuilds {c1[0]} / {c0[0]}, straggler passes {c1[2]} / {c0[2]}, tile-days {c1[3]} / {c0[3]}, stats {st1.tolist()}")
    assert np.array_equal(thr1, thr0, equal_nan=True), "lean thresholds differ from the general body's"
    assert np.array_equal(st1, st0), (st1, st0)
    assert c1 == c0, (c1, c0)
    assert int(st1[4]) == 0                                  # nothing unresolved
    exp = _oracle_rows(world, (field, start, list_rows), slab_vals[0], cal, q)
    got = thr1[:, SEAM[0] * NX:SEAM[1] * NX].T
    assert np.array_equal(got, exp, equal_nan=True), "lean thresholds differ from the oracle on the seam rows"
    foot = _oracle_rows(world, (field, start, list_rows), slab_vals[1], cal, q, FOOT, FOOT_SLAB)
    assert np.array_equal(thr1[:, FOOT[0] * NX:FOOT[1] * NX].T, foot, equal_nan=True), "lean thresholds differ from the oracle on the last rows"
    assert np.isfinite(exp).any()
    tiles = 9
    if field != "land":
        assert c1[3] == tiles * 366, c1
    if field == "seasonal":
        assert c1[0] > tiles, c1                             # more rebuilds than the one that starts each tile's walk
    if field == "step":
        assert c1[2] > 0, c1                                 # the first tile column needed extra passes
    if field == "land":
        assert c1[3] == (tiles - 1) * 366, c1                # the all-land tile walked no day
        assert np.isnan(exp).any() and np.isnan(thr1[:, 28 * NX + 2]).all()
