"""Host side of the time-blocked pre-processing: the memory model and the block planner, the
tracker's ``preprocess_block_steps`` keyword and the compaction entry point's refusal of a null context -- no GPU."""
import numpy as np
import pytest

import marex_amd
import marex_amd.track as trk_mod
from marex_amd import _lib
from marex_amd.exceptions import ConfigurationError, TrackingError
from marex_amd.xr_compat import DataArray

HEADLINE = (36500, 720, 1440)


def _alloc(T, C, Tf, B, **kw):
    return trk_mod.preprocess_alloc_bytes(trk_mod.preprocess_memory_need(T, kw.pop("ny", None), C, kw.pop("R_fill", 0), Tf, B, **kw))


@pytest.mark.parametrize("T,ny,nx,Tf,R,free", [(100, 48, 96, 2, 2, 3_000_000), (100, 48, 96, 0, 0, 1_200_000),
                                              (37, 5, 35, 4, 1, 60_000), (500, None, 4100, 2, 3, 9_000_000),
                                              (12, 48, 96, 2, 2, 10**9)])
def test_plan_returns_the_largest_block_that_fits(T, ny, nx, Tf, R, free):
    C = nx if ny is None else ny * nx
    for kw in (dict(resident=True), dict(host_input=True), dict()):
        B = trk_mod.plan_preprocess_blocks(T, C, Tf, free, ny=ny, R_fill=R, **kw)
        assert 1 <= B <= T
        assert _alloc(T, C, Tf, B, ny=ny, R_fill=R, **kw) <= free
        if B < T:
            assert _alloc(T, C, Tf, B + 1, ny=ny, R_fill=R, **kw) > free
    assert trk_mod.plan_preprocess_blocks(12, 48 * 96, 2, 10**9, ny=48, R_fill=2) == 12   # never more than T


def test_plan_raises_with_need_and_free_when_one_step_does_not_fit():
    T, ny, nx = 100, 48, 96
    need = _alloc(T, ny * nx, 2, 1, ny=ny, R_fill=2, host_input=True)
    with pytest.raises(TrackingError, match=rf"needs {need / 1e9:.3f} GB of device memory, {(need - 1) / 1e9:.3f} GB are free"):
        trk_mod.plan_preprocess_blocks(T, ny * nx, 2, need - 1, ny=ny, R_fill=2, host_input=True)
    assert trk_mod.plan_preprocess_blocks(T, ny * nx, 2, need, ny=ny, R_fill=2, host_input=True) == 1
    with pytest.raises(TrackingError):
        trk_mod.plan_preprocess_blocks(0, 10, 2, 10**9)


def test_headline_field_needs_two_bytes_per_cell_blocked_and_eleven_whole():
    T, ny, nx = HEADLINE
    n = T * ny * nx
    need = trk_mod.preprocess_memory_need(T, ny, ny * nx, 8, 2, 64, resident=True)
    assert 2.0 <= sum(need.values()) / n < 2.1
    assert trk_mod.preprocess_alloc_bytes(need) / n < 1.1      # the resident input is allocated already
    assert sum(trk_mod.tracking_memory_need(T, ny, nx, 8, 2, resident=True).values()) / n > 11
    # window entries: three uint8 of B + 2 T_fill rows, int32 labels and areas of B rows
    C = ny * nx
    assert need["window buffers 3 x uint8"] == 3 * 68 * C
    assert need["block labels int32"] == need["block areas int32"] == 4 * 64 * C
    assert need["library scratch"] >= 4 * 64 * C


def test_a_host_input_is_not_part_of_the_need():
    T, ny, nx = 100, 48, 96
    n = T * ny * nx
    host = trk_mod.preprocess_memory_need(T, ny, ny * nx, 2, 2, 8, host_input=True)
    dev = trk_mod.preprocess_memory_need(T, ny, ny * nx, 2, 2, 8, resident=True)
    assert not any("input" in k for k in host) and sum(k.startswith("input") for k in dev) == 1
    assert sum(dev.values()) - sum(host.values()) == n
    mesh = trk_mod.preprocess_memory_need(T, None, 4100, 3, 2, 8, host_input=True)
    assert mesh["library scratch"] == max(2 * 12 * 4100, 4 * 8 * 4100) and mesh["pre-processed mask uint8"] == T * 4100


def test_tracking_memory_need_is_unchanged():
    need = trk_mod.tracking_memory_need(14, 48, 96, 2, 2)
    n = 14 * 48 * 96
    assert sum(need.values()) == 3 * n + 8 * n + n + 4 * n + max(16 * 14 * 56 * 2, 4 * n)


def _field():
    T, ny, nx = 4, 6, 8
    da = DataArray(np.zeros((T, ny, nx), bool), dims=("time", "lat", "lon"),
                   coords={"time": np.arange(T), "lat": np.linspace(-10, 10, ny), "lon": np.linspace(0, 70, nx)})
    return da, DataArray(np.ones((ny, nx), bool), dims=("lat", "lon"))


@pytest.mark.parametrize("bad", [0, -1, 2.5, "yes", True])
def test_bad_preprocess_block_steps_is_a_configuration_error(bad):
    da, mk = _field()
    with pytest.raises(ConfigurationError, match="preprocess_block_steps"):
        marex_amd.tracker(da, mk, R_fill=1, allow_merging=False, preprocess_block_steps=bad)


@pytest.mark.parametrize("good", [None, 1, 7, np.int64(3), "auto"])
def test_good_preprocess_block_steps_is_kept(good):
    da, mk = _field()
    t = marex_amd.tracker(da, mk, R_fill=1, allow_merging=False, preprocess_block_steps=good)
    assert t.preprocess_block_steps == good


def test_compaction_refuses_a_null_context_without_a_device():
    lib = _lib.load()
    assert lib.marex_compact_positive_i32(None, None, 10, None, 10, None, None) != 0
    buf = np.zeros(16, np.int64)
    assert lib.marex_compact_positive_i32(None, buf.ctypes.data, 4, buf.ctypes.data, 4, buf.ctypes.data, buf.ctypes.data) != 0
    assert not buf.any()
