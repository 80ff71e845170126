"""The list mask kernel's row stores (marex_mask_ge_doy_tails_f32): every row position of every bucket size.

The kernel keeps one bit per (cell, row of the bucket) in 32-bit words and writes each row's four mask bytes of a lane as
one word taken from the byte-interleaved words of a group of eight rows; full groups are unrolled, the last group of a
bucket is a loop.  The cases below put extremes on the first and last row of the groups and words (rows 0, 7, 8, 31, 32,
63, 64, 95 and the bucket's last row) for bucket sizes on both sides of every group and word boundary, in both
instances (three and four words of row bits) and both list geometries (15 rows in 2 chunks, 32 rows in 4 chunks).

Anomalies and thresholds are made by hand; the expectation is the definition, extreme[t, c] = anom[t, c] >=
thr[doy(t), c] with NaN never extreme, in NumPy; mask bytes and count must match it exactly.  `test_inputs_*` checks
without a device that the expectation really holds every row position and lane pattern the cases are there for.
"""
import numpy as np
import pytest

from marex_amd import binning, calendar

C_ALL = 904            # cells of the field
CELLS = (260, 860)     # 600 owned cells from a multiple of 4 that is no multiple of 256: lanes start at cell 256
SENTINEL = 0xA7        # bytes outside the owned range keep it
ROWS = (0, 7, 8, 31, 32, 63, 64, 95)

LANE_ROWS = slice(300, 304)     # exactly one extreme per special bucket, on the same row of all four cells
LANE_NONE = slice(304, 308)     # no extreme at all
LANE_ALL = slice(308, 312)      # every sample extreme: first chunks entirely above the threshold, the key-by-key walk
LANE_NAN = slice(312, 316)      # NaN thresholds on cells 313 and 315
LANE_PATTERN = slice(340, 344)  # four different row patterns in bucket D_PATTERN
LANE_EDGES = slice(400, 408)    # two lanes: thresholds and samples on the table's edges and one ulp beside them
CELL_BEYOND1, CELL_BEYOND2, CELL_BEYOND3 = 320, 321, 324  # one, two, three samples beyond the table in one bucket each
D_ROWS0, D_PATTERN, D_BEYOND = 10, 20, 50

CASES = [(7, 15), (8, 15), (9, 15), (31, 15), (32, 15), (33, 15), (63, 15), (64, 15), (65, 15), (95, 32), (96, 32),   # three words
         (97, 32), (100, 32), (128, 32),                                                                              # four words
         (33, 32), (96, 15), (97, 15)]                                                                                # the other geometry


def _inputs(nd):
    """Calendar of `nd` years from 2001 (buckets of nd rows, dayofyear 366 of the leap years only), anomalies, thresholds,
    the expectation, and the facts about it that the cases rely on (asserted here, on the CPU)."""
    days = int((np.datetime64(f"{2001 + nd}-01-01") - np.datetime64("2001-01-01")).astype(np.int64))
    cal = calendar.build_calendar(calendar.daily_time_axis("2001-01-01", days))
    sizes = np.diff(cal.doy_start)
    assert int(sizes.max()) == nd and 0 < int(sizes[365]) < nd, sizes
    rows = lambda d: cal.doy_rows[cal.doy_start[d]:cal.doy_start[d + 1]]
    T = cal.doy_rows.size
    rng = np.random.default_rng(100 + nd)
    bt = binning.hobday_bins()
    anom = rng.standard_normal((T, C_ALL), dtype=np.float32) * np.float32(0.8)
    thr = (np.float32(1.0) + rng.uniform(-0.2, 0.2, size=(366, C_ALL))).astype(np.float32)

    # one extreme per bucket, on the same row of every cell of the lane
    special = {}
    for k, r in enumerate(list(ROWS) + [nd - 1]):
        if r < nd:
            special[D_ROWS0 + k] = r
    special[365] = int(sizes[365]) - 1  # the last row of the partial bucket
    anom[:, LANE_ROWS] = 0.0
    thr[:, LANE_ROWS] = 2.9
    for d, r in special.items():
        anom[rows(d)[r], LANE_ROWS] = 3.0
    np.minimum(anom[:, LANE_NONE], np.float32(4.0), out=anom[:, LANE_NONE])
    thr[:, LANE_NONE] = 4.5
    thr[:, LANE_ALL] = -6.0
    thr[:, [313, 315]] = np.nan
    # four different row patterns in one lane and bucket: cell i has rows i and nd - 1 - i
    anom[rows(D_PATTERN), LANE_PATTERN] = 0.0
    thr[D_PATTERN, LANE_PATTERN] = 2.9
    for i in range(4):
        anom[rows(D_PATTERN)[[i, nd - 1 - i]], LANE_PATTERN.start + i] = 3.0
    # samples beyond the table: their positions come with the aux word (one or two), or the lane compares values (three)
    anom[rows(D_BEYOND)[nd // 2], CELL_BEYOND1] = 7.5
    anom[rows(D_BEYOND + 1)[[1, nd - 2]], CELL_BEYOND2] = [7.5, np.inf]
    anom[rows(D_BEYOND + 2)[[0, nd // 2, nd - 1]], CELL_BEYOND3] = 7.5
    # thresholds on every edge of the table and one ulp below and above, samples drawn from the same values
    e = bt.edges[1:]
    ties = np.concatenate([e, np.nextafter(e, np.float32(-np.inf)), np.nextafter(e, np.float32(np.inf))]).astype(np.float32)
    assert ties.size <= 366 * 8
    t_edges = rng.choice(ties, size=(366, 8))
    t_edges.reshape(-1)[:ties.size] = ties
    thr[:, LANE_EDGES] = t_edges
    anom[:, LANE_EDGES] = rng.choice(ties, size=(T, 8))

    doy_of_row = np.empty(T, dtype=np.int64)
    for d in range(366):
        doy_of_row[rows(d)] = d
    with np.errstate(invalid="ignore"):
        exp = anom >= thr[doy_of_row]

    for d, r in special.items():  # exactly the planted row, on all four cells
        want = np.zeros((rows(d).size, 4), dtype=bool)
        want[r] = True
        assert np.array_equal(exp[rows(d), LANE_ROWS], want), (d, r)
    assert {r for r in ROWS if r < nd} | {nd - 1} <= set(special.values())
    assert not exp[:, LANE_NONE].any() and exp[:, LANE_ALL].all()
    assert not exp[:, [313, 315]].any() and exp[:, 312].any() and exp[:, 314].any()
    pat = exp[rows(D_PATTERN), LANE_PATTERN]
    assert len({pat[:, i].tobytes() for i in range(4)}) == 4 and pat.any(axis=0).all()
    assert exp[rows(D_BEYOND)[nd // 2], CELL_BEYOND1] and exp[rows(D_BEYOND + 1)[[1, nd - 2]], CELL_BEYOND2].all()
    assert exp[rows(D_BEYOND + 2)[[0, nd // 2, nd - 1]], CELL_BEYOND3].all()
    assert exp[:, LANE_EDGES].any() and not exp[:, LANE_EDGES].all()
    return cal, bt, anom, thr, exp


@pytest.mark.parametrize("nd", sorted({nd for nd, _ in CASES}))
def test_inputs_reach_every_row_position(nd):
    _inputs(nd)


@pytest.mark.gpu
@pytest.mark.parametrize("nd,list_rows", CASES)
def test_rows_of_every_bucket_size(hot, nd, list_rows):
    import torch

    cal, bt, anom, thr, exp = _inputs(nd)
    c0, c1 = CELLS
    dcal = hot.upload_calendar(cal)
    ad = torch.from_numpy(anom).to(hot.device)
    td = torch.from_numpy(thr).to(hot.device)
    tl = hot.tail_extract(ad, dcal, bt, list_rows=list_rows)
    assert int(tl["max_bucket"]) == nd and int(tl["list_rows"]) == list_rows
    assert tuple(tl["tails"].shape[1:3]) == (-(-nd // list_rows), 2 if list_rows <= 16 else 4)  # [366, lists, chunks, C, 8]
    wsp = {"extreme": torch.full((anom.size,), SENTINEL, dtype=torch.uint8, device=hot.device)}
    m = hot.mask_ge_doy_tails(tl, ad, td, dcal, bt, cells=CELLS, wsp=wsp)
    hot.sync()
    got = m["extreme"].cpu().numpy()
    assert (got[:, :c0] == SENTINEL).all() and (got[:, c1:] == SENTINEL).all(), "bytes outside the owned cells were written"
    own = got[:, c0:c1]
    assert own.max() <= 1
    bad = np.argwhere(own.astype(bool) != exp[:, c0:c1])
    assert bad.size == 0, f"{len(bad)} mask bytes differ, first (row, cell) {bad[0][0]}, {bad[0][1] + c0}"
    assert int(m["n_true"].item()) == int(exp[:, c0:c1].sum())
