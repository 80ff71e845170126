"""Merge tracking in time blocks, host side (no GPU): the tracker's ``merge_block_steps`` keyword, the memory estimate
and the helper that merges the overlap lists of the blocks."""
import numpy as np
import pytest

import marex_amd
from marex_amd.exceptions import ConfigurationError, ProcessingError, TrackingError
from marex_amd.track import merge_block_pairs, merge_memory_need, plan_merge_blocks
from marex_amd.xr_compat import DataArray


def _da(T=4, ny=6, nx=8):
    ev = np.zeros((T, ny, nx), dtype=bool)
    ev[1, 2, 3] = True
    return DataArray(ev, dims=("time", "lat", "lon"),
                     coords={"time": np.arange(T), "lat": np.linspace(-80, 80, ny), "lon": np.linspace(0, 360, nx, endpoint=False)})


def test_tracker_accepts_merge_block_steps_without_touching_the_gpu(monkeypatch):
    import marex_amd.detect as det

    monkeypatch.setattr(det, "get_engine", lambda *a, **k: (_ for _ in ()).throw(AssertionError("GPU touched")))
    mask = DataArray(np.ones((6, 8), dtype=bool), dims=("lat", "lon"))
    kw = dict(R_fill=2, allow_merging=True, timechunks=2, coordinate_units="degrees")
    assert marex_amd.tracker(_da(), mask, merge_block_steps=3, **kw).merge_block_steps == 3
    assert marex_amd.tracker(_da(), mask, merge_block_steps=np.int64(3), **kw).merge_block_steps == 3
    assert marex_amd.tracker(_da(), mask, merge_block_steps="auto", **kw).merge_block_steps == "auto"
    assert marex_amd.tracker(_da(), mask, **kw).merge_block_steps is None
    for bad in (0, -2, 1.5, True, "3"):
        with pytest.raises(ConfigurationError, match="merge_block_steps must be a positive number of timesteps, 'auto' or None"):
            marex_amd.tracker(_da(), mask, merge_block_steps=bad, **kw)
    with pytest.raises(ConfigurationError, match="merge_block_steps is for merge tracking on grids"):
        marex_amd.tracker(_da(), mask, R_fill=2, allow_merging=False, merge_block_steps=3)


def test_a_single_slice_of_2_31_cells_stays_refused_and_none_keeps_the_refusal(monkeypatch):
    import marex_amd.detect as det

    monkeypatch.setattr(det, "get_engine", lambda *a, **k: object())  # an engine nothing is asked of
    mask = DataArray(np.ones((6, 8), dtype=bool), dims=("lat", "lon"))
    t = marex_amd.tracker(_da(), mask, R_fill=2, timechunks=2, coordinate_units="degrees", merge_block_steps=1)

    class Wide:  # only the shape is looked at before the refusal
        shape = (3, 46341, 46341)  # 46341^2 >= 2^31 - 1

    t.data_bin = Wide()
    with pytest.raises(TrackingError, match="one timestep of 2147488281 cells"):
        t.run()
    with pytest.raises(TrackingError, match="one timestep of 2147488281 cells"):
        t.track_objects(Wide())


def test_merge_memory_need_on_the_forty_year_record():
    T, ny, nx, B = 14610, 720, 1440, 2071
    C = ny * nx
    n = T * C
    need = merge_memory_need(T, ny, nx, B)
    assert need["pre-processed mask uint8"] == n
    assert need["ID field int32"] == 4 * n
    assert need["labelling scratch int32 (areas and ranks of one block)"] == 8 * 2071 * C
    assert sum(need.values()) == 5 * n + 8 * 2071 * C < 8 * n
    assert "cell areas float32 (one slice)" not in need
    assert merge_memory_need(T, ny, nx, B, weights=True)["cell areas float32 (one slice)"] == 4 * C
    assert "pre-processed mask uint8" not in merge_memory_need(T, ny, nx, B, resident=True)
    # a block is never more than 2^31 - 2 cells, whatever is asked for
    assert merge_memory_need(T, ny, nx, 10**6) == need
    # a small field: B >= T gives the sizes of the unblocked run (areas and ranks as large as the ID field)
    small = merge_memory_need(100, 10, 100, 100)
    assert small == merge_memory_need(100, 10, 100, 5000)
    assert small["ID field int32"] == 400000 and small["labelling scratch int32 (areas and ranks of one block)"] == 800000
    assert merge_memory_need(100, 10, 100, 7)["labelling scratch int32 (areas and ranks of one block)"] == 8 * 7000


def test_the_block_planner_takes_the_largest_block_that_fits():
    T, ny, nx = 14610, 720, 1440
    C = ny * nx
    n = T * C
    assert plan_merge_blocks(T, ny, nx, 10**13) == 2071                       # the cell limit of a block
    assert plan_merge_blocks(T, ny, nx, 5 * n + 8 * 100 * C) == 100           # the memory limit
    assert plan_merge_blocks(T, ny, nx, 5 * n + 8 * 100 * C - 1) == 99
    assert plan_merge_blocks(T, ny, nx, 4 * n + 8 * C, resident=True) == 1
    assert plan_merge_blocks(5, 10, 10, 10**9) == 5                           # never more than T
    with pytest.raises(TrackingError, match="one step per block needs"):
        plan_merge_blocks(T, ny, nx, 5 * n + 8 * C - 1)
    with pytest.raises(TrackingError, match="exceeds the labelling block"):
        plan_merge_blocks(3, 46341, 46341, 10**15)


def test_block_pair_lists_merge_by_key_in_lexicographic_order():
    a = np.array([[1, 2, 10], [1, 5, 3], [7, 2, 4]], np.int32)
    b = np.array([[1, 2, 5], [3, 9, 1], [1, 4, 2]], np.int32)
    c = np.zeros((0, 3), np.int32)
    got = merge_block_pairs([a, c, b])
    assert got.dtype == np.int32
    assert got.tolist() == [[1, 2, 15], [1, 4, 2], [1, 5, 3], [3, 9, 1], [7, 2, 4]]
    assert merge_block_pairs([a]).tolist() == a.tolist()
    assert merge_block_pairs([]).shape == (0, 3) and merge_block_pairs([c, c]).dtype == np.int32
    # IDs up to int32's largest keep their order and their value
    big = np.array([[2**31 - 1, 1, 1], [2, 2**31 - 1, 1]], np.int32)
    assert merge_block_pairs([big, big]).tolist() == [[2, 2**31 - 1, 2], [2**31 - 1, 1, 2]]
    # counts are summed before the int32 check: two blocks that fit on their own, a sum that does not
    half = np.array([[4, 6, 2**30]], np.int32)
    assert merge_block_pairs([half]).tolist() == half.tolist()
    with pytest.raises(ProcessingError, match="int32 cannot hold"):
        merge_block_pairs([half, np.array([[4, 6, 2**30]], np.int32)])
    assert merge_block_pairs([half, np.array([[4, 6, 2**30 - 1]], np.int32)]).tolist() == [[4, 6, 2**31 - 1]]
