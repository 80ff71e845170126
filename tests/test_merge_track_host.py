"""Merge tracker (marEx.tracker(..., allow_merging=True), gridded data) on the host: the oracle of tests/merge_oracle.py
against the counts the reference's own tests pin, hand-checked partitions, consolidation and ledger cases, and the
constructor's chunking rule -- no GPU needed."""
import os
import sys

import numpy as np
import pytest

import marex_amd
from marex_amd import zarr_io
from marex_amd.exceptions import ConfigurationError
from marex_amd.track import _components, _time_chunk_layout
from marex_amd.xr_compat import DataArray

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import merge_oracle as mo  # noqa: E402
from test_track_host import FIX, load_fixture  # noqa: E402


# ---------------------------------------------------------------------------------------------------- the anchor
@pytest.mark.parametrize("nn,events,merges", [(False, 21, 15), (True, 20, 13)])
def test_oracle_falls_in_the_reference_test_ranges(nn, events, merges):
    """test_tracking_data_consistency / test_advanced_tracking_with_merging of the reference (time chunks of 2)."""
    ev, mask, lat, lon, _ = load_fixture(True)
    tv = zarr_io.read_dataset(FIX)["time"].values
    out, attrs, mds = mo.run(ev, mask, tv, lat, lon, mo.chunk_layout(32, 2), 4, 2, 0.5, nn=nn)
    assert abs(attrs["N_objects_prefiltered"] - 516) <= 2 and abs(attrs["N_objects_filtered"] - 258) <= 2
    assert abs(attrs["N_events_final"] - events) <= 1
    assert abs(attrs["total_merges"] - merges) <= 2
    assert abs(attrs["preprocessed_area_fraction"] - 0.9143) <= 0.02
    pres = out["presence"]
    assert np.array_equal(pres, out["global_ID"] != 0) and (out["area"][pres] > 0).all()
    assert (out["time_start"] <= out["time_end"]).all()
    c = out["centroid"]
    assert np.nanmin(c[0]) >= lat.min() and np.nanmax(c[0]) <= lat.max()
    assert np.nanmin(c[1]) >= lon.min() and np.nanmax(c[1]) <= lon.max()


# ---------------------------------------------------------------------------------------------------- hand cases
def _two(ny=12, nx=240):  # nx >= 200: the seam bands of calculate_centroid do not overlap
    return np.zeros((2, ny, nx), np.int32)


def _sm(ids, chunks=(2,), nn=False, regional=False):
    return mo.split_and_merge(ids, list(chunks), np.arange(ids.shape[0]), 0.5, nn, regional)


def test_two_parents_merge_into_one_child():
    ids = _two()
    ids[0, 5:8, 10:13] = 1  # A, centroid x = 11
    ids[0, 5:8, 20:23] = 2  # B, centroid x = 21
    ids[1, 5:8, 10:23] = 3  # the child
    for regional in (False, True):
        out, props, ov, (mt, mp, mc, ma) = _sm(ids, regional=regional)
        # x <= 16 is nearer A (x = 16 is a tie: the first parent), x >= 17 nearer B
        assert (out[1, 5:8, 10:17] == 3).all() and (out[1, 5:8, 17:23] == 4).all()
        assert [p.tolist() for p in mp] == [[1, 2]] and [c.tolist() for c in mc] == [[3, 4]] and [a.tolist() for a in ma] == [[9, 9]]
        assert sorted(map(tuple, ov.tolist())) == [(1, 3), (2, 4)]
        assert props[3] == [21.0, 6.0, 13.0] and props[4] == [18.0, 6.0, 19.5]


def test_two_parents_across_the_seam():
    ids = _two()
    ids[0, 5:8, 236:239] = 1  # centroid x = 237
    ids[0, 5:8, 2:5] = 2      # centroid x = 3
    ids[1, 5:8, 236:240] = 3
    ids[1, 5:8, 0:5] = 3
    out, props, ov, merges = _sm(ids)
    # x = 0: 3 from both centroids (wrapped) -> the first parent; x = 1 .. 4 nearer B
    assert (out[1, 5:8, 236:240] == 3).all() and (out[1, 5:8, 0] == 3).all() and (out[1, 5:8, 1:5] == 4).all()
    assert props[3] == [15.0, 6.0, 238.0]  # seam rule: (-4 - 3 - 2 - 1 + 0) / 5 + 240
    assert props[4] == [12.0, 6.0, 2.5]


def test_three_parents_and_the_ledger_broadcast():
    ids = _two()
    ids[0, 5:8, 10:13] = 1
    ids[0, 5:8, 20:23] = 2
    ids[0, 5:8, 30:33] = 3
    ids[1, 5:8, 10:33] = 4
    out, props, ov, merges = _sm(ids)
    mds = mo.merges_dataset(merges, np.int64)
    assert mds["parent_IDs"].tolist() == [[1, 2, 3]] and mds["child_IDs"].tolist() == [[4, 5, 6]]
    assert mds["n_parents"].dtype == np.int8 and int((mds["n_parents"] > 2).sum()) == 1
    lat, lon = np.arange(12.0), np.arange(240.0)
    res = mo.cluster_rename(out, ov, mds, np.arange(2), lat, lon, np.ones((12, 240), np.float32))
    assert res["N"] == 3
    led = res["merge_ledger"]
    assert led.shape == (2, 3, 3) and (led[0] == -1).all()
    assert led[1].tolist() == [[1, 1, 1], [2, 2, 2], [3, 3, 3]]  # [t, P, :] = P for every parent event P
    assert res["global_ID"].tolist() == [[1, 2, 3], [4, 5, 6]]


def test_split_rejoined_by_consolidation_unless_alone_in_its_chunk():
    ids = _two()
    ids[0, 5:8, 10:31] = 1
    ids[1, 5:8, 10:16] = 2
    ids[1, 5:8, 25:31] = 3
    out, props, ov, merges = _sm(ids, chunks=(2,))
    assert set(np.unique(out[1]).tolist()) == {0, 2} and 3 not in props and props[2][0] == 36.0
    out, props, ov, merges = _sm(ids, chunks=(1, 1))  # step 1 alone in its chunk: not consolidated
    assert set(np.unique(out[1]).tolist()) == {0, 2, 3}
    lut, n = mo.events(out, ov)
    assert n == 1 and lut[1] == lut[2] == lut[3] == 1


def test_centroid_tie_takes_the_first_parent():
    a = mo.partition_centroid(np.array([2]), np.array([5]), [[2.0, 3.0], [2.0, 7.0]], 11, True)
    assert a.tolist() == [0]
    # distinct squares whose square roots round equal compare equal, as the reference's sqrt values do: parent 0 is at
    # squared distance 4 + 2^-50 (dy = 2^-25, dx = 2), parent 1 at exactly 4; both square roots round to 2.0
    pc = [[-2.0 ** -25, 2.0], [0.0, 2.0]]
    d2 = [(0.0 - y) * (0.0 - y) + (0.0 - x) * (0.0 - x) for y, x in pc]
    assert d2[0] > d2[1] and np.sqrt(d2[0]) == np.sqrt(d2[1])
    a = mo.partition_centroid(np.array([0]), np.array([0]), pc, 100, False)
    assert a.tolist() == [0]  # comparing the squares would pick parent 1


def test_nn_nearest_cell_outside_the_buckets_is_not_seen():
    ny, nx = 60, 200
    ys, xs = np.array([5]), np.array([10])
    p0 = (np.array([5]), np.array([30]))   # distance 20, bucket (0, 3): outside the 3 x 3 buckets of (0, 1)
    p1 = (np.array([19]), np.array([25]))  # distance 20.5, bucket (1, 2): inside
    a = mo.partition_nn(ys, xs, [p0, p1], np.array([[5.0, 30.0], [19.0, 25.0]]), ny, nx, 40, True)
    assert a.tolist() == [1]


def test_nn_without_candidates_falls_back_to_the_centroid():
    ny, nx = 60, 200
    ys, xs = np.array([5]), np.array([10])
    p0 = (np.array([5]), np.array([120]))
    p1 = (np.array([40]), np.array([60]))
    a = mo.partition_nn(ys, xs, [p0, p1], np.array([[5.0, 120.0], [40.0, 60.0]]), ny, nx, 40, True)
    assert a.tolist() == [1]
    assert mo.nn_params([10.0, 400.0]) == (60, 15) and mo.nn_params([4.0]) == (40, 10)


def test_components_number_events_by_smallest_id():
    rng = np.random.default_rng(3)
    from scipy.sparse import csr_matrix
    from scipy.sparse.csgraph import connected_components

    for n in (1, 7, 200):
        m = rng.integers(0, 2 * n)
        a, b = rng.integers(0, n, m), rng.integers(0, n, m)
        _, exp = connected_components(csr_matrix((np.ones(m, bool), (a, b)), shape=(n, n)), directed=False)
        assert np.array_equal(_components(n, a, b), exp)


# ---------------------------------------------------------------------------------------------------- constructor
def _fixture_da():
    ds = zarr_io.read_dataset(FIX)
    ev = ds["extreme_events"]
    m = ds["mask"]
    return (DataArray(ev.values.astype(bool), dims=ev.dims, coords={k: ev.coords[k] for k in ev.coords}),
            DataArray(m.values.astype(bool), dims=m.dims))


def test_merging_needs_a_time_chunking():
    da, mask = _fixture_da()
    with pytest.raises(ConfigurationError) as e:
        marex_amd.tracker(da, mask, R_fill=2)
    assert str(e.value).startswith("allow_merging=True is not supported")
    assert "timechunks" in str(e.value)
    trk = marex_amd.tracker(da, mask, R_fill=2, timechunks=5)
    assert trk._time_chunks == [5] * 6 + [2] and trk.nn_partitioning is False and trk.coordinate_units == "degrees"
    da.encoding["chunks"] = (2, 180, 360)
    assert marex_amd.tracker(da, mask, R_fill=2, nn_partitioning=True)._time_chunks == [2] * 16
    da.chunks = ((3,) * 10 + (2,), (180,), (360,))
    assert marex_amd.tracker(da, mask, R_fill=2, timechunks=7)._time_chunks == [3] * 10 + [2]
    assert _time_chunk_layout(da, None, None) == [3] * 10 + [2]
    with pytest.raises(ConfigurationError):
        marex_amd.tracker(da, mask, R_fill=2, unstructured_grid=True)
    with pytest.raises(ConfigurationError):
        marex_amd.tracker(da, mask, R_fill=2, checkpoint="save")


def test_store_records_its_chunks():
    ds = zarr_io.read_dataset(FIX)
    assert tuple(ds["extreme_events"].encoding["chunks"]) == (2, 180, 360)
    assert mo.chunk_layout(32, 3) == [3] * 10 + [2] and mo.chunk_layout(5, chunks=(1, 4)) == [1, 4]


def test_merge_repeats_until_the_iteration_cap(caplog):
    """nx = 40 < 200: calculate_centroid's seam bands overlap, so B's centroid moves to x = 34.33 and every child cell
    stays nearer A; the child still has two parents after each iteration, so the merge is recorded again (a new ID per
    iteration, which gets no cells) until the cap of 10 iterations warns."""
    ids = np.zeros((2, 12, 40), np.int32)
    ids[0, 5:8, 10:13] = 1
    ids[0, 5:8, 20:23] = 2
    ids[1, 5:8, 10:23] = 3
    with caplog.at_level("WARNING", logger="marex_amd"):
        out, props, ov, (mt, mp, mc, ma) = _sm(ids)
    assert props[2][2] == pytest.approx(34 + 1 / 3)
    assert (out[1][ids[1] > 0] == 3).all()
    assert [c.tolist() for c in mc] == [[3, k] for k in range(4, 14)] and len(mp) == 10
    assert any("did not converge after 10 iterations" in r.message for r in caplog.records)


def second_iteration_case():
    """A merge that resolves on its second iteration.  t = 0: A (1) rows 5..7 x cols 10..19, B (2) rows 5..7 x cols
    40..49, D (3) rows 8..19 x cols 10..19 (120 cells).  t = 1: child 4 = A's and B's cells plus rows 8..11 x cols 10..19
    (100 cells).  D overlaps it in 40 cells: 40 / min(120, 100) = 0.4 < 0.5, so iteration 1 splits 4 between A and B only
    (B's half -> 5).  The piece 4 left near A has 60 cells, so D's 40 now pass (40 / 60), and iteration 2 splits it between
    A (centroid row 6) and D (row 13.5): rows 10..11 are nearer D -> 6."""
    ids = np.zeros((2, 20, 240), np.int32)
    ids[0, 5:8, 10:20] = 1
    ids[0, 5:8, 40:50] = 2
    ids[0, 8:20, 10:20] = 3
    ids[1, 5:12, 10:20] = 4
    ids[1, 5:8, 40:50] = 4
    return ids


def test_merge_resolved_on_the_second_iteration(caplog):
    ids = second_iteration_case()
    with caplog.at_level("WARNING", logger="marex_amd"):
        out, props, ov, (mt, mp, mc, ma) = _sm(ids)
    assert not any("did not converge" in r.message for r in caplog.records)
    assert [p.tolist() for p in mp] == [[1, 2], [1, 3]] and [c.tolist() for c in mc] == [[4, 5], [4, 6]]
    assert [a.tolist() for a in ma] == [[30, 30], [30, 40]] and mt == [1, 1]
    assert (out[1, 5:10, 10:20] == 4).all() and (out[1, 10:12, 10:20] == 6).all() and (out[1, 5:8, 40:50] == 5).all()
    assert props[4][0] == 50.0 and props[5][0] == 30.0 and props[6][0] == 20.0
    assert sorted(map(tuple, ov.tolist())) == [(1, 4), (2, 5), (3, 6)]


def test_explicit_timechunks_that_disagree_with_the_data_warn(caplog):
    da, mask = _fixture_da()
    da.encoding["chunks"] = (2, 180, 360)
    with caplog.at_level("WARNING", logger="marex_amd"):
        trk = marex_amd.tracker(da, mask, R_fill=2, timechunks=7)
    assert trk._time_chunks == [2] * 16
    assert any("timechunks=7 is ignored" in r.message for r in caplog.records)
    caplog.clear()
    with caplog.at_level("WARNING", logger="marex_amd"):
        marex_amd.tracker(da, mask, R_fill=2, timechunks=2)
    assert not any("is ignored" in r.message for r in caplog.records)
