"""Labelling in time blocks, host side (no GPU): the block planner, the algorithm restated in NumPy against one
``scipy.ndimage.label`` over the whole field (which pins the numbering argument of DESIGN.md section 4), the memory
estimate and the tracker's new keyword."""
import os
import sys

import numpy as np
import pytest

import marex_amd
from marex_amd.engine import LABEL_BLOCK_CELLS, plan_time_blocks
from marex_amd.exceptions import ConfigurationError, TrackingError
from marex_amd.track import labelling_memory_need, tracking_memory_need
from marex_amd.xr_compat import DataArray

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import label_blocks_oracle as lbo  # noqa: E402
import track_oracle as tor  # noqa: E402


def _check_plan(blocks, T, C, limit):
    assert blocks[0][0] == 0 and blocks[-1][1] == T
    for (a0, a1), (b0, _) in zip(blocks, blocks[1:]):
        assert a1 == b0
    for t0, t1 in blocks:
        assert t1 > t0 and (t1 - t0) * C <= limit
    # greedy: every block but the last is as long as the limit allows
    for t0, t1 in blocks[:-1]:
        assert (t1 - t0 + 1) * C > limit


@pytest.mark.parametrize("T,C,limit", [(10, 7, 21), (10, 7, 7), (10, 7, 13), (1, 5, 5), (9, 4, 1000), (2072, 720 * 1440, None),
                                       (14610, 720 * 1440, None), (5, 2**31 - 2, None), (3, 2**30, None)])
def test_planner_blocks_are_contiguous_cover_the_axis_and_fit(T, C, limit):
    blocks = plan_time_blocks(T, C, limit)
    _check_plan(blocks, T, C, LABEL_BLOCK_CELLS if limit is None else limit)


def test_planner_on_the_sizes_the_design_names():
    C = 720 * 1440
    assert plan_time_blocks(2072, C) == [(0, 2071), (2071, 2072)]
    assert plan_time_blocks(2071, C) == [(0, 2071)]
    assert len(plan_time_blocks(14610, C)) == 8
    assert plan_time_blocks(4, 2**31 - 2) == [(0, 1), (1, 2), (2, 3), (3, 4)]   # one-step blocks just under the limit
    assert plan_time_blocks(7, 10, 3 * 10) == [(0, 3), (3, 6), (6, 7)]          # a forced block of three steps
    assert plan_time_blocks(7, 10, 10**12) == [(0, 7)]                            # never more than 2^31 - 2 cells a block
    assert plan_time_blocks(3, 2**30, 10**12) == [(0, 1), (1, 2), (2, 3)]


@pytest.mark.parametrize("T,C,limit", [(4, 2**31 - 1, None), (4, 2**31, None), (4, 2**33, None), (4, 10, 9), (0, 10, None),
                                       (4, 0, None), (4, 10, 0), (4, 10, -5)])
def test_planner_refuses_what_cannot_be_a_block(T, C, limit):
    with pytest.raises(TrackingError):
        plan_time_blocks(T, C, limit)


def test_label_whole_is_the_track_oracle_and_scipy():
    from scipy import ndimage as ndi

    rng = np.random.default_rng(11)
    for shape, dens in (((6, 9, 12), 0.3), ((5, 1, 20), 0.5), ((7, 6, 1), 0.5), ((4, 7, 2), 0.4)):
        x = rng.random(shape) < dens
        for wrap in (True, False):
            exp, n = tor.label_3d(x, wrap_x=wrap)
            got, m = lbo.label_whole(x, wrap, True)
            assert m == n and np.array_equal(got, exp)
        exp, n = ndi.label(x, structure=np.ones((3, 3, 3), bool))
        got, m = lbo.label_whole(x, False, True)
        assert m == n and np.array_equal(got, exp)
        # without time links: every step labelled on its own, numbered on through time
        got, m = lbo.label_whole(x, False, False)
        k = 0
        for t in range(shape[0]):
            e, nt = ndi.label(x[t], structure=np.ones((3, 3), bool))
            assert np.array_equal(got[t], np.where(e > 0, e + k, 0))
            k += nt
        assert m == k


def _block_lengths(T):
    return sorted({b for b in (1, 2, 3, 7, T - 1) if 1 <= b})


def _check_blocked(x, wrap, connect_t, what):
    exp, n = lbo.label_whole(x, wrap, connect_t)
    exp_areas = np.bincount(exp.reshape(-1), minlength=n + 1)[1:]
    for b in _block_lengths(x.shape[0]):
        got, m, areas = lbo.label_blocked(x, b, wrap, connect_t)
        assert m == n, (what, b, m, n)
        assert np.array_equal(got, exp), (what, b)
        assert np.array_equal(areas, exp_areas), (what, b)
    return n


def test_blocked_labelling_equals_one_labelling_on_random_blobby_fields():
    rng = np.random.default_rng(2031)
    k = 0
    for shape in ((9, 12, 16), (12, 7, 20), (10, 1, 24), (8, 9, 1), (11, 10, 2)):
        for dens in (0.05, 0.2, 0.5):
            x = lbo.blobby(rng, shape, dens)
            for wrap in (True, False):
                for connect_t in (True, False):
                    _check_blocked(x, wrap, connect_t, (shape, dens, wrap, connect_t))
                    k += 1
        x = rng.random(shape) < 0.3  # salt and pepper: many small objects, many unions per seam
        _check_blocked(x, True, True, (shape, "noise"))
    assert k == 60


def test_blocked_labelling_equals_one_labelling_on_the_hand_built_seam_cases():
    cases = lbo.seam_cases()
    assert len(cases) >= 50
    for name, x, wrap, n_exp in cases:
        n = _check_blocked(x, wrap, True, name)
        if n_exp is not None:
            assert n == n_exp, name
        _check_blocked(x, wrap, False, name + " (no time links)")


def test_joining_through_the_later_block_shifts_every_later_id():
    """Two events of block 0 meet only in block 1: the second disappears into the first and every ID behind it moves down
    by one -- also inside block 0, which therefore goes through the table like every other block."""
    name, x, wrap, _ = next(c for c in lbo.seam_cases() if c[0] == "joined only through the later block, bar at t=2")
    ids, n, _ = lbo.label_blocked(x, 2, wrap, True)
    blk0, n0 = lbo.label_whole(x[:2], wrap, True)
    assert n0 == 4 and n == 5
    assert ids[0, 2, 2] == ids[0, 2, 6] == 1 and blk0[0, 2, 6] == 2
    assert blk0[0, 6, 3] == 3 and ids[0, 6, 3] == 2  # block 0 does NOT map to itself
    assert not np.array_equal(ids[:2], blk0)


def test_memory_need_lists_the_buffers_of_the_peak():
    n = 2072 * 720 * 1440
    need = tracking_memory_need(2072, 720, 1440, 2, 2)
    assert need["2-D labels int32"] == need["2-D areas int32"] == 4 * n
    assert need["mask uint8"] == need["hole-filled mask uint8"] == need["gap-filled mask uint8"] == need["filtered mask uint8"] == n
    assert need["library scratch"] == 4 * (2**31 - 2)
    assert "gap-filled mask uint8" not in tracking_memory_need(2072, 720, 1440, 2, 0)
    assert "mask uint8" not in tracking_memory_need(2072, 720, 1440, 2, 0, resident=True)
    lab = labelling_memory_need(2072, 720 * 1440)
    assert lab["ID field int32"] == 4 * n and lab["areas int32 (one block)"] == 4 * 2071 * 720 * 1440
    small = labelling_memory_need(100, 1000)
    assert small["areas int32 (one block)"] == small["ID field int32"] == 400000   # the single call: areas as large as the IDs
    assert labelling_memory_need(100, 1000, 7 * 1000)["areas int32 (one block)"] == 4 * 7000
    # the labelling never needs more than the pre-processing peak that precedes it
    for T in (10, 2071, 2072, 14610):
        for tf in (0, 2):
            assert sum(labelling_memory_need(T, 720 * 1440, resident=True).values()) + T * 720 * 1440 \
                <= sum(tracking_memory_need(T, 720, 1440, 0, tf, resident=True).values())


def _da(T=4, ny=6, nx=8):
    ev = np.zeros((T, ny, nx), dtype=bool)
    ev[1, 2, 3] = True
    return DataArray(ev, dims=("time", "lat", "lon"),
                     coords={"time": np.arange(T), "lat": np.linspace(-80, 80, ny), "lon": np.linspace(0, 360, nx, endpoint=False)})


def test_tracker_accepts_label_block_steps_without_touching_the_gpu(monkeypatch):
    import marex_amd.detect as det

    monkeypatch.setattr(det, "get_engine", lambda *a, **k: (_ for _ in ()).throw(AssertionError("GPU touched")))
    mask = DataArray(np.ones((6, 8), dtype=bool), dims=("lat", "lon"))
    t = marex_amd.tracker(_da(), mask, R_fill=2, allow_merging=False, label_block_steps=3)
    assert t.label_block_steps == 3
    assert marex_amd.tracker(_da(), mask, R_fill=2, allow_merging=False).label_block_steps is None
    for bad in (0, -2, 1.5, True, "3"):
        with pytest.raises(ConfigurationError, match="label_block_steps must be a positive number of timesteps"):
            marex_amd.tracker(_da(), mask, R_fill=2, allow_merging=False, label_block_steps=bad)


def test_only_merge_tracking_still_refuses_by_total_size(monkeypatch):
    """``_check_size`` is the merge tracker's refusal now: run() with merging raises it before any device work, and its
    message says so."""
    import marex_amd.detect as det

    monkeypatch.setattr(det, "get_engine", lambda *a, **k: (_ for _ in ()).throw(AssertionError("GPU touched")))
    with pytest.raises(TrackingError, match="merge tracking"):
        marex_amd.tracker._check_size((2072, 720, 1440))
    mask = DataArray(np.ones((6, 8), dtype=bool), dims=("lat", "lon"))
    t = marex_amd.tracker(_da(), mask, R_fill=2, allow_merging=True, timechunks=2, coordinate_units="degrees")

    class Huge:  # only the shape is looked at before the refusal
        shape = (2072, 720, 1440)

    t.data_bin = Huge()
    with pytest.raises(TrackingError, match="merge tracking"):
        t.run()
    with pytest.raises(TrackingError, match="merge tracking"):
        t.track_objects(Huge())
