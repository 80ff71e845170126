"""GPU parity: the merge tracker with ``merge_block_steps`` -- per-timestep labelling and the final overlap pass in time
blocks, the cluster renaming by the fused pass -- against the host oracle of tests/merge_oracle.py (and so against the run
without the keyword), the memory check, and a field of 2^31 cells on device tensors."""
import os
import sys
import time

import numpy as np
import pytest
import torch

import marex_amd
from marex_amd.exceptions import TrackingError
from marex_amd.xr_compat import DataArray
from marex_amd.zarr_io import DeviceDataArray

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import merge_oracle as mo  # noqa: E402
from test_gpu_merge_track import _blobs, _check, _da, _fixture_time, _oracle  # noqa: E402
from test_track_host import load_fixture  # noqa: E402

pytestmark = pytest.mark.gpu

_cache = {}


def _fixture_case(**kw):
    """The reference fixture and its oracle result, computed once per set of oracle arguments."""
    key = tuple(sorted(kw.items()))
    if key not in _cache:
        ev, mask, lat, lon, _ = load_fixture(True)
        tv = _fixture_time()
        tc = kw.pop("tc")
        _cache[key] = (ev, mask, lat, lon, tv, _oracle(ev, mask, tv, lat, lon, mo.chunk_layout(32, tc), 4, 2, **kw))
    return _cache[key]


@pytest.mark.parametrize("nn", [False, True])
@pytest.mark.parametrize("B", [1, 3, 7, 32, "auto"])
def test_fixture_matches_oracle_for_every_block_length(hot, nn, B):
    ev, mask, lat, lon, tv, (exp, attrs, mds) = _fixture_case(tc=2, nn=nn)
    trk = marex_amd.tracker(_da(ev, tv, lat, lon), DataArray(mask, dims=("lat", "lon")), R_fill=4, T_fill=2,
                            area_filter_quartile=0.5, allow_merging=True, nn_partitioning=nn, timechunks=2, merge_block_steps=B)
    ds, merges = trk.run(return_merges=True)
    _check(ds, merges, exp, attrs, mds, tv, lat, lon)
    assert set(trk._stage_times) == {"objects", "split_and_merge", "cluster_rename"}


def _blob_case(seed):
    if ("blobs", seed) not in _cache:
        nn, regional, tc = {1: (False, False, 4), 2: (True, False, 3), 3: (False, True, 1), 4: (True, True, 7)}[seed]
        T, ny, nx = 24, 60, 240
        ev = _blobs(T, ny, nx, 40, seed)
        mask = np.ones((ny, nx), bool)
        lat = np.linspace(-59.5, 59.5, ny).astype(np.float32)
        lon = np.linspace(0.75, 359.25, nx).astype(np.float32)
        tv = np.arange(T).astype("datetime64[D]").astype("datetime64[ns]")
        orc = _oracle(ev, mask, tv, lat, lon, mo.chunk_layout(T, tc), 1, 2, q=0.2, nn=nn, regional=regional)
        _cache["blobs", seed] = (ev, mask, lat, lon, tv, nn, regional, tc, orc)
    return _cache["blobs", seed]


@pytest.mark.parametrize("B", [1, 5])
@pytest.mark.parametrize("seed", [1, 2, 3, 4])
def test_fuzz_colliding_blobs_in_blocks(hot, seed, B):
    """Seams at every step (B = 1), inside and across the time chunks (B = 5 against chunks of 4, 3, 1 and 7), with and
    without the periodic boundary."""
    ev, mask, lat, lon, tv, nn, regional, tc, (exp, attrs, mds) = _blob_case(seed)
    assert attrs["total_merges"] > 0
    trk = marex_amd.tracker(_da(ev, tv, lat, lon), DataArray(mask, dims=("lat", "lon")), R_fill=1, T_fill=2,
                            area_filter_quartile=0.2, nn_partitioning=nn, regional_mode=regional, timechunks=tc,
                            coordinate_units="degrees", merge_block_steps=B)
    _check(*trk.run(return_merges=True), exp, attrs, mds, tv, lat, lon)


def test_grid_resolution_in_blocks(hot):
    ev, mask, lat, lon, tv, (exp, attrs, mds) = _fixture_case(tc=3, grid_resolution=1.0)
    trk = marex_amd.tracker(_da(ev, tv, lat, lon), DataArray(mask, dims=("lat", "lon")), R_fill=4, T_fill=2,
                            grid_resolution=1.0, timechunks=3, merge_block_steps=4)
    # rtol 1e-6: the project's own tolerance for the float32 area totals (tests/test_gpu_merge_track.py)
    _check(*trk.run(return_merges=True), exp, attrs, mds, tv, lat, lon, rtol=1e-6)


def test_composes_with_blocked_preprocessing(hot):
    ev, mask, lat, lon, tv, (exp, attrs, mds) = _fixture_case(tc=2, nn=False)
    trk = marex_amd.tracker(_da(ev, tv, lat, lon), DataArray(mask, dims=("lat", "lon")), R_fill=4, T_fill=2, timechunks=2,
                            merge_block_steps=3, preprocess_block_steps=5)
    _check(*trk.run(return_merges=True), exp, attrs, mds, tv, lat, lon)


def test_not_enough_device_memory_is_a_tracking_error_with_both_numbers(hot, monkeypatch):
    ev, mask, lat, lon, tv, _ = _fixture_case(tc=2, nn=False)
    monkeypatch.setattr(torch.cuda, "mem_get_info", lambda *a, **k: (1000, 2000))
    monkeypatch.setattr(torch.cuda, "memory_reserved", lambda *a, **k: 0)
    monkeypatch.setattr(torch.cuda, "memory_allocated", lambda *a, **k: 0)
    for kw in ({"merge_block_steps": 3}, {"merge_block_steps": 3, "preprocess_block_steps": 5}):
        trk = marex_amd.tracker(_da(ev, tv, lat, lon), DataArray(mask, dims=("lat", "lon")), R_fill=4, T_fill=2, timechunks=2, **kw)
        with pytest.raises(TrackingError, match=r"tracker.run: needs \d+\.\d{3} GB of device memory, 0.000 GB are free"):
            trk.run()
    trk = marex_amd.tracker(_da(ev, tv, lat, lon), DataArray(mask, dims=("lat", "lon")), R_fill=4, T_fill=2, timechunks=2,
                            merge_block_steps="auto")
    with pytest.raises(TrackingError, match="merge tracking in time blocks: one step per block needs"):
        trk.run()
    with pytest.raises(TrackingError, match="tracker.track_objects: needs"):
        marex_amd.tracker(_da(ev, tv, lat, lon), DataArray(mask, dims=("lat", "lon")), R_fill=4, T_fill=2, timechunks=2,
                          merge_block_steps=3).track_objects(_da(ev, tv, lat, lon))


def test_a_field_of_2_31_cells_is_merge_tracked_in_two_blocks(hot):
    """130 steps of 2880 x 5760 = 2 156 544 000 cells >= 2^31, on a device tensor: zero but for its last five steps, which
    hold a five-step pattern of colliding blobs built at 360 x 720 and repeated 8 times in y and x.  The plan is 129 + 1
    steps, so the labelling seam and the seam of the final overlap pass lie between pattern steps 3 and 4.  Expected: the
    tracker without the keyword on the five pattern steps alone."""
    from marex_amd.engine import plan_time_blocks

    T, ny, nx, P, S = 130, 2880, 5760, 5, 8
    C = ny * nx
    assert T * C >= 2**31 and plan_time_blocks(T, C) == [(0, 129), (129, 130)]
    small = _blobs(P, ny // S, nx // S, 40, 4, rmax=20.0)
    tv = np.arange(T).astype("datetime64[D]").astype("datetime64[ns]")
    lat = np.linspace(-89.97, 89.97, ny).astype(np.float32)
    lon = np.linspace(0.03, 359.97, nx).astype(np.float32)
    # the pattern merges, the last time at its last step: checked with the oracle at the 1/8 scale
    _, m8, _ = mo.track(small, tv[:P], lat[::S], lon[::S], mo.chunk_layout(P, P), 0.5, False, True, None, lon_init=lon[::S],
                        units="degrees")
    assert len(m8["n_parents"]) >= 1 and m8["merge_time"].max() == tv[P - 1]
    pat = torch.from_numpy(small).to(hot.device).repeat_interleave(S, dim=1).repeat_interleave(S, dim=2)
    mask = DataArray(np.ones((ny, nx), bool), dims=("lat", "lon"))
    kw = dict(R_fill=1, T_fill=2, timechunks=P, regional_mode=True, coordinate_units="degrees")

    def dev_da(t, times):
        return DeviceDataArray(t, ("time", "lat", "lon"), {"time": times, "lat": lat, "lon": lon})

    ref = marex_amd.tracker(dev_da(pat, tv[:P]), mask, **kw)
    exp, exp_m, exp_n = ref.track_objects(dev_da(pat, tv[:P]))
    assert exp_n > 10 and len(exp_m["n_parents"].values) >= 1
    big = torch.zeros((T, ny, nx), dtype=torch.bool, device=hot.device)
    big[T - P:] = pat
    del pat
    with pytest.raises(TrackingError, match="merge tracking"):  # the parent's behaviour, and still the default
        marex_amd.tracker(dev_da(big, tv), mask, **kw).track_objects(dev_da(big, tv))
    torch.cuda.reset_peak_memory_stats(hot.device)
    t0 = time.perf_counter()
    trk = marex_amd.tracker(dev_da(big, tv), mask, merge_block_steps="auto", **kw)
    ds, merges, n = trk.track_objects(dev_da(big, tv))
    wall = time.perf_counter() - t0
    print(f"\n2^31 field: {T} x {ny} x {nx}, {n} events, {len(merges['n_parents'].values)} merges, {wall:.2f} s, torch peak "
          f"{torch.cuda.max_memory_allocated(hot.device) / 1e9:.2f} GB, stages {trk._stage_times}")
    assert n == exp_n
    ids = np.asarray(ds["ID_field"].values)
    assert ids.dtype == np.int32 and ids.shape == (T, ny, nx)
    assert np.array_equal(ids[T - P:], np.asarray(exp["ID_field"].values))
    assert not ids[:T - P].any()
    del ids
    for k in ("global_ID", "area", "presence", "merge_ledger"):
        got, want = np.asarray(ds[k].values), np.asarray(exp[k].values)
        assert got.dtype == want.dtype and got.shape == (T,) + want.shape[1:], k
        assert np.array_equal(got[T - P:], want, equal_nan=True), k
        blank = got[:T - P]
        assert np.isnan(blank).all() if k == "area" else (blank == {"merge_ledger": -1}.get(k, 0)).all(), k
    cen, want = np.asarray(ds["centroid"].values), np.asarray(exp["centroid"].values)
    assert cen.dtype == want.dtype and np.array_equal(cen[:, T - P:], want, equal_nan=True) and np.isnan(cen[:, :T - P]).all()
    shift = tv[T - P] - tv[0]
    for k in ("time_start", "time_end"):
        assert np.array_equal(np.asarray(ds[k].values), np.asarray(exp[k].values) + shift), k
    assert list(merges.data_vars) == list(exp_m.data_vars)
    for k in exp_m.data_vars:
        got, want = np.asarray(merges[k].values), np.asarray(exp_m[k].values)
        assert got.dtype == want.dtype and np.array_equal(got, want + shift if k == "merge_time" else want), k
