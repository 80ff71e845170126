"""The event matching on the device: ``marex_event_matching_count_i32`` / ``marex_event_matching_i32`` through
``HotPath.event_matching`` against the NumPy oracle at the edges of the kernel's layout, of its run-time key and of its table --
exact integers throughout -- the cross-checks against the statistics that exist already, and the public path on a grid, a mesh
and the trackers' own fields."""
import os
import sys

import numpy as np
import pytest

import marex_amd
from marex_amd.engine import HotPath
from marex_amd.exceptions import DataValidationError, ProcessingError
from marex_amd.xr_compat import DataArray

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import event_matching_cases as mc  # noqa: E402
import event_matching_oracle as mo  # noqa: E402

pytestmark = pytest.mark.gpu
F = np.float32
I31 = mc.I31


def layout():
    from marex_amd.csrc import build as _build

    _build.build(verbose=False)
    return HotPath.matching_layout()


L = layout()
PIECE, WAVE, WG, STRIDE = L["piece"], L["wave"], L["wg"], L["row_stride"]
SHAPES = sorted({1, 63, 64, 65, 255, 257, WAVE - 1, WAVE, WAVE + 1, WG - 1, WG, WG + 1})
FIELDS = ("t", "a", "b", "cells", "area")


def run(hot, a, b, q=None, cap=None, windows=None):
    """``HotPath.event_matching`` over the windows between the cuts (one call by default), joined as the public path does."""
    import torch

    T = a.shape[0]
    xa, xb = (torch.from_numpy(np.ascontiguousarray(v, dtype=np.int32)).to(hot.device) for v in (a, b))
    w = sorted(set(windows or (0, T)))
    parts = [hot.event_matching(xa[s:e], xb[s:e], t0=s, q=q, cap=cap) for s, e in zip(w[:-1], w[1:])]
    r = {k: np.concatenate([p[k] for p in parts]) for k in FIELDS}
    order = np.lexsort((r["b"], r["a"]))
    return {k: v[order] for k, v in r.items()}, parts


def check(hot, a, b, q=None, **kw):
    r, parts = run(hot, a, b, q, **kw)
    mc.assert_same(r, mo.step_records(a, b, q))
    return r, parts


def pairs_of(rng, T, C):
    a, b = mc.blob_pair(rng, T, C, n_ids=max(3, C // 40), width=min(C, 23))
    a[:, 0] = 7  # a cell of an event throughout
    return (a, b), mc.random_pair(rng, T, C)


@pytest.mark.parametrize("C", SHAPES)
def test_at_the_layout_edges(hot, C):
    rng = np.random.default_rng(C)
    q = rng.integers(0, 2**40, C).astype(np.int64)
    for a, b in pairs_of(rng, 2, C):
        check(hot, a, b)
        check(hot, a, b, q=q)


@pytest.mark.parametrize("T", [1, 2, STRIDE - 1, STRIDE, STRIDE + 1])
def test_rows_around_the_row_stride(hot, T):
    rng = np.random.default_rng(100 + T)
    C = WG + 70
    (a, b), _ = pairs_of(rng, T, C)
    r, _ = check(hot, a, b, q=rng.integers(0, 2**40, C).astype(np.int64))
    assert set(r["t"].tolist()) == set(range(T))


@pytest.mark.parametrize("name", ["one_event", "own_ids", "a_only", "b_only", "alternating", "empty_step"])
def test_field_shapes(hot, name):
    rng = np.random.default_rng(8)
    T, C = 3, WAVE + 130
    q = rng.integers(0, 2**40, C).astype(np.int64)
    if name == "one_event":
        a, b = np.full((T, C), 5, np.int32), np.full((T, C), 9, np.int32)
    elif name == "own_ids":
        a = (1 + np.arange(T * C, dtype=np.int32)).reshape(T, C)
        b = a[:, ::-1].copy()
    elif name in ("a_only", "b_only"):
        a, b = np.full((T, C), 3, np.int32), np.zeros((T, C), np.int32)
        if name == "b_only":
            a, b = b, a
    elif name == "alternating":
        a = np.tile(1 + (np.arange(C, dtype=np.int32) % 2), (T, 1))
        b = np.tile(1 + (np.arange(C, dtype=np.int32) % 3), (T, 1))
    else:  # a step in which neither field holds an event, between steps that do
        a, b = mc.blob_pair(rng, T, C)
        a[0, 3], a[1], a[2, 5] = 2, 0, 4
        b[1] = 0
    r, _ = check(hot, a, b, q=q)
    if name == "one_event":
        assert r["cells"].tolist() == [C] * T and r["area"].tolist() == [int(q.sum())] * T
    if name == "own_ids":
        assert (r["cells"] == 1).all() and r["t"].size == T * C  # nothing folds
    if name == "a_only":
        assert (r["b"] == 0).all() and (r["a"] == 3).all() and r["t"].tolist() == [0, 1, 2]
    if name == "b_only":
        assert (r["a"] == 0).all() and (r["b"] == 3).all()
    if name == "empty_step":
        assert 1 not in r["t"]


def test_key_corners_split_the_window(hot):
    T, C = 9, 70
    a, b = np.zeros((T, C), np.int32), np.zeros((T, C), np.int32)
    a[:, [0, 4, 9]], a[:, [1, 5, 10]] = 1, I31
    b[:, [0, 1, 20]], b[:, [4, 5, 21]] = 1, I31
    r, parts = check(hot, a, b, q=np.arange(1, C + 1, dtype=np.int64))
    w = parts[0]["widths"]
    assert w == (31, 31, 2) and (1 << w[2]) < T  # sub-windows of 4 steps: a split happened
    assert sorted(set(zip(r["a"].tolist(), r["b"].tolist()))) == [(0, 1), (0, I31), (1, 0), (1, 1), (1, I31), (I31, 0), (I31, 1), (I31, I31)]
    assert set(r["t"].tolist()) == set(range(T))


def test_widths_that_sum_to_64_run_whole_and_one_more_step_is_split(hot):
    rng = np.random.default_rng(21)
    C = 300
    a, b = mc.random_pair(rng, 9, C)
    a[:, 7], b[:, 11] = I31, 2**30 - 1  # 31 and 30 bits: 3 remain for the step
    r8, p8 = check(hot, a[:8], b[:8])
    assert p8[0]["widths"] == (31, 30, 3) and sum(p8[0]["widths"]) == 64 and 8 <= 1 << p8[0]["widths"][2]  # one launch
    r9, p9 = check(hot, a, b)
    assert p9[0]["widths"] == (31, 30, 3) and 9 > 1 << p9[0]["widths"][2]  # split
    first = r9["t"] < 8
    for k in FIELDS:
        assert np.array_equal(r9[k][first], r8[k]), k


def test_the_table_at_load_one_half_at_its_end_and_too_small(hot):
    import torch

    # cap = 64 with exactly 32 distinct keys
    a = (1 + np.arange(32, dtype=np.int32)).reshape(1, 32)
    b = a[:, ::-1].copy()
    r, parts = check(hot, a, b, cap=64)
    assert r["a"].size == 32 and parts[0]["cap"] == 64 and parts[0]["runs"] == 32 and HotPath.exposure_cap(32) == 64
    # keys that the hash sends to the last two entries: the probes wrap around the table's end.  An anchor cell holds 511 in
    # both fields, so that the widths are (9, 9, 2) whatever else is placed
    T, C, cap = 4, 64, 64
    widths = HotPath.matching_widths(511, 511, T)
    assert widths == (9, 9, 2)
    t, i, j = np.meshgrid(np.arange(T), np.arange(0, 512), np.arange(0, 512), indexing="ij")
    home = HotPath.exposure_home(HotPath.matching_key(t, i, j, widths), cap)
    a, b = np.zeros((T, C), np.int32), np.zeros((T, C), np.int32)
    a[0, 0] = b[0, 0] = 511
    cell = np.ones(T, int)
    sel = (home >= cap - 2) & ((i > 0) | (j > 0))
    for tt, ii, jj in list(zip(t[sel], i[sel], j[sel]))[::97][:14]:
        a[tt, cell[tt]], b[tt, cell[tt]] = ii, jj
        cell[tt] += 1
    assert cell.sum() - T == 14
    r, parts = check(hot, a, b, cap=cap)
    assert parts[0]["widths"] == widths
    at_end = HotPath.exposure_home(HotPath.matching_key(r["t"], r["a"], r["b"], widths), cap) >= cap - 2
    assert r["a"].size == 15 and at_end.sum() >= 14
    # a table below the number of distinct keys: a handled status, and the engine goes on
    a = (1 + np.arange(100, dtype=np.int32)).reshape(1, 100)
    b = np.ones((1, 100), np.int32)
    with pytest.raises(ProcessingError, match="the table of 64 entries does not hold the keys of 100 runs"):
        run(hot, a, b, cap=64)
    with pytest.raises(ProcessingError, match="cap=100 is not a power of two"):
        run(hot, a, b, cap=100)
    check(hot, a, b)
    for bad_a, bad_b, name in ((np.where(a == 50, -3, a), b, "ID_field_a"), (a, -b, "ID_field_b")):
        with pytest.raises(DataValidationError, match="Object IDs must be non-negative") as err:
            run(hot, bad_a, bad_b)
        assert name in str(err.value) + str(getattr(err.value, "details", ""))
    check(hot, a, b, cap=256)
    # widths too narrow for the IDs, passed directly to the C entry: the overflow status, nothing written, and the next call
    # succeeds -- a handled status, not a fault
    xa, xb = (torch.from_numpy(v).to(hot.device) for v in (a, b))
    status = torch.zeros(8, dtype=torch.int64, device=hot.device)
    hot.call("marex_event_matching_count_i32", xa, xb, 1, 100, status)
    assert status.cpu().numpy().tolist()[:5] == [0, 0, 100, 100, 1]
    tab = [torch.full((256,), 7, dtype=torch.int64, device=hot.device) for _ in range(2)]
    out = [torch.full((100,), -5, dtype=torch.int64, device=hot.device) for _ in range(2)]
    hot.call("marex_event_matching_i32", xa, xb, 1, 100, None, 3, 1, 1, 256, tab[0], tab[1], None, status, 100, out[0], out[1], None)
    s = status.cpu().numpy().tolist()
    assert s[5] == 0 and s[6] == 100 - 7 and s[7] == 7  # the IDs 1 .. 7 fit 3 bits, the other 93 cells are counted and dropped
    kept = np.sort(out[0][:7].cpu().numpy().view(np.uint64))
    assert np.array_equal(kept, HotPath.matching_key(0, np.arange(1, 8), 1, (3, 1, 1))) and (out[0][7:] == -5).all()
    assert int((tab[0] != 0).sum()) == 7 and int(tab[1].sum()) == 7
    hot.call("marex_event_matching_i32", xa, xb, 1, 100, None, 1, 1, 1, 256, tab[0], tab[1], None, status, 100, out[0], out[1], None)
    s = status.cpu().numpy().tolist()
    assert s[5] == 0 and s[6] == 99 and s[7] == 1
    hot.call("marex_event_matching_i32", xa + 1, xb, 1, 100, None, 1, 1, 1, 256, tab[0], tab[1], None, status, 100, out[0], out[1], None)
    s = status.cpu().numpy().tolist()  # the IDs 2 .. 101 under one bit: every cell is counted, nothing is written
    assert s[5] == 0 and s[6] == 100 and s[7] == 0 and int((tab[0] != 0).sum()) == 0 and int((tab[1] != 0).sum()) == 0
    with pytest.raises(ProcessingError, match=r"marex_event_matching_i32 failed \(code -1\)"):
        hot.call("marex_event_matching_i32", xa, xb, 1, 100, None, 31, 31, 3, 256, tab[0], tab[1], None, status, 100, out[0], out[1], None)
    with pytest.raises(ProcessingError, match=r"marex_event_matching_i32 failed \(code -1\)"):
        hot.call("marex_event_matching_i32", xa, xb, 1, 100, None, 8, 0, 4, 256, tab[0], tab[1], None, status, 100, out[0], out[1], None)
    check(hot, a, b)


def test_windows_and_residency_give_the_same_records(hot):
    import torch

    rng = np.random.default_rng(10)
    T, C = 7, 700
    (a, b), _ = pairs_of(rng, T, C)
    q = rng.integers(0, 2**40, C).astype(np.int64)
    whole, _ = check(hot, a, b, q=q)
    for w in ([0, 1, 2, 3, 4, 5, 6, 7], [0, 2, 4, 6, 7], [0, 7]):
        r, _ = run(hot, a, b, q=q, windows=w)
        for k in whole:
            assert r[k].tobytes() == whole[k].tobytes(), (k, w)
    r, _ = run(hot, a, b, q=torch.from_numpy(q).to(hot.device))  # the table as a device tensor
    assert all(r[k].tobytes() == whole[k].tobytes() for k in whole)
    # the public path: host and resident fields and their mixes, block_steps in {1, 2, 3, T}
    areas = rng.integers(1, 2**10, C).astype(np.float64)
    ds = marex_amd.event_matching(a, b, cell_areas=areas, per_timestep=True)
    mc.assert_dataset(ds, mo.matching(a, b, areas, per_timestep=True))
    ta, tb = torch.from_numpy(a).to(hot.device), torch.from_numpy(b).to(hot.device)
    for fa, fb, s in ((a, b, 1), (a, b, 2), (a, b, T), (ta, tb, 3), (ta, b, 2), (a, tb, 3), (ta, tb, None)):
        mc.same_bytes(ds, marex_amd.event_matching(fa, fb, cell_areas=areas, per_timestep=True, block_steps=s))


def test_cross_checks_against_event_exposure_and_event_intensity(hot):
    from event_exposure_cases import dyadic_anomalies, dyadic_weights

    rng = np.random.default_rng(11)
    T, ny, nx = 6, 40, 64
    C = ny * nx
    ids = mc.blob_field(rng, T, C, n_ids=9, width=300)
    regions = (np.arange(C) // 900).astype(np.int64) * 4  # three regions ...
    regions[regions > 8] = -1
    regions[np.arange(C) % 11 == 5] = -1  # ... plus holes
    w = dyadic_weights(rng, C) + F(1)
    ex = marex_amd.event_exposure(ids, regions, cell_areas=w)
    rvals = np.asarray(ex["region_events"].coords["region"].values)
    rank = np.where(regions >= 0, np.searchsorted(rvals, regions), -1)
    field_b = np.broadcast_to((rank + 1).astype(np.int32), (T, C)).copy()  # region rank + 1 as an "event" at every step
    field_b[ids <= 0] = 0  # the exposure sees a region only under an event
    ds = marex_amd.event_matching(ids, field_b, cell_areas=w)
    v, x = ({k: np.asarray(d[k].values) for k in d.data_vars} for d in (ds, ex))
    assert v["pair_ID_a"].size > 9 and np.array_equal(v["pair_ID_a"], x["pair_ID"]) and np.array_equal(rvals[v["pair_ID_b"] - 1], x["pair_region"])
    for k in ("pair_steps", "pair_cell_steps", "pair_area_steps", "pair_cells_max", "pair_time_start", "pair_time_end",
              "pair_time_of_max_area", "pair_area_max"):
        assert np.array_equal(v[k], x[k]) and v[k].dtype == x[k].dtype, k
    assert np.array_equal(v["pair_share_of_a"], x["pair_share_of_event"])
    # matched = whole - outside as exact integers, each share one division: fl(m / A) and 1 - fl(o / A) each lie within
    # 2^-53 of m / A = 1 - o / A for the division (a quotient in 0 .. 1) plus 2^-53 for the subtraction: 3 * 2^-53 apart
    out = x["event_outside_share"]
    assert 0 < out.max() and out.min() < 1 and np.abs(v["a_matched_share"] - (1 - out)).max() <= 3 * 2.0**-53
    assert np.array_equal(v["a_matched_share"] == 1, out == 0) and np.array_equal(v["a_matched_share"] == 0, out == 1)
    ei = marex_amd.event_intensity(ids, dyadic_anomalies(rng, (T, C)), cell_areas=w)
    assert np.array_equal(v["a_steps"], np.asarray(ei["event_duration"].values)) and v["a_steps"].min() > 0


def test_public_path_on_a_grid_and_a_mesh(hot):
    rng = np.random.default_rng(12)
    T, ny, nx = 12, 9, 44
    C = ny * nx
    tv = (np.datetime64("2003-12-25") + np.arange(T)).astype("datetime64[ns]")
    a, b = mc.blob_pair(rng, T, C, n_ids=10, width=30)
    area_y = np.array([1.0, 2.5, 4.0, 6.0, 8.0, 6.0, 4.0, 2.5, 1.0])
    dims = ("time", "lat", "lon")
    fa = DataArray(a.reshape(T, ny, nx), dims=dims, coords={"time": ("time", tv)})
    fb = DataArray(b.reshape(T, ny, nx), dims=dims, coords={"time": ("time", tv)})
    for per in (False, True):
        ds = marex_amd.event_matching(fa, fb, cell_areas=area_y, min_share=0.3, per_timestep=per)
        mc.assert_dataset(ds, mo.matching(a, b, np.repeat(area_y, nx), min_share=0.3, per_timestep=per, tv=tv))
    mc.assert_dataset(marex_amd.event_matching(fa, fb), mo.matching(a, b, tv=tv))
    # a mesh: areas orders of magnitude apart
    T, C = 9, 3001
    a, b = mc.blob_pair(rng, T, C, n_ids=20, width=60)
    areas = rng.integers(1, 2**10, C) * 2.0 ** rng.integers(-20, 30, C)
    ds = marex_amd.event_matching(DataArray(a, dims=("time", "ncells")), DataArray(b, dims=("time", "ncells")), cell_areas=areas,
                                  per_timestep=True, block_steps=4)
    mc.assert_dataset(ds, mo.matching(a, b, areas, per_timestep=True))
    assert np.asarray(ds["pair_ID_a"].values).size > 5


def test_merge_tracker_against_basic_tracker_of_the_same_mask(hot):
    from intensity_cases import blobs

    ev = blobs()
    T, ny, nx = ev.shape
    tv = np.arange(T).astype("datetime64[D]").astype("datetime64[ns]")
    lat, lon = np.linspace(-57.5, 57.5, ny).astype(F), np.linspace(3.75, 356.25, nx).astype(F)
    valid = np.ones((ny, nx), bool)
    valid[5:9, 6:12] = False
    ev = ev & valid[None]
    dims = ("time", "lat", "lon")
    coords = {"time": ("time", tv), "lat": ("lat", lat), "lon": ("lon", lon)}
    trk, events = {}, {}
    for merging in (True, False):
        trk[merging] = marex_amd.tracker(DataArray(ev, dims=dims, coords=coords, name="extreme_events"), DataArray(valid, dims=("lat", "lon")),
                                         R_fill=1, T_fill=2, area_filter_quartile=0.2, timechunks=4, coordinate_units="degrees",
                                         allow_merging=merging, grid_resolution=7.5)
        events[merging] = trk[merging].run()
    a, b = (np.asarray(events[m]["ID_field"].values).reshape(T, -1) for m in (True, False))
    assert a.max() >= 2 and b.max() >= 1
    n = [int(np.asarray(events[m]["ID"].values).size) if "ID" in events[m] else None for m in (True, False)]
    wy = np.arange(1.0, ny + 1)
    ds = trk[True].event_matching(events[True], events[False], per_timestep=True, cell_areas=wy, block_steps=5)
    mc.assert_dataset(ds, mo.matching(a, b, np.repeat(wy, nx), per_timestep=True, tv=tv, n_a=n[0], n_b=n[1]))
    mc.same_bytes(ds, trk[True].event_matching(events[True], events[False]["ID_field"], per_timestep=True, cell_areas=wy))
    v = {k: np.asarray(ds[k].values) for k in ds.data_vars}
    # the merge tracker splits what the basic tracker keeps as one event: one event of one tracking has two partners
    assert max(v["a_matches"].max(), v["b_matches"].max()) >= 2 and float(v["pod"]) > 0 and int(v["cell_steps_both"]) > 0
    # the tracker's own areas are the default
    own = trk[True].event_matching(events[True], events[False])
    mc.assert_dataset(own, mo.matching(a, b, trk[True]._cell_weights.reshape(-1), tv=tv, n_a=n[0], n_b=n[1]))
    if n[0] is not None and n[0] > 1:
        bad = marex_amd.Dataset({"ID_field": events[True]["ID_field"], "ID": DataArray(np.arange(1, 2), dims=("ID",))})
        with pytest.raises(ProcessingError, match="the ID field holds event"):
            trk[True].event_matching(bad, events[False])
        shifted_ids = marex_amd.Dataset({"ID_field": events[True]["ID_field"], "ID": DataArray(np.arange(2, n[0] + 2), dims=("ID",))})
        with pytest.raises(ProcessingError, match="the ID axis of the other Dataset is not 1 .. N"):
            trk[True].event_matching(events[True], shifted_ids)
    with pytest.raises(TypeError, match="unexpected keyword argument 'by'"):
        trk[True].event_matching(events[True], events[False], by="year")


def test_mesh_tracker_field_against_itself_one_step_later(hot):
    from test_mesh_merge_host import THRESHOLD, load_merging_fixture

    f = load_merging_fixture()  # the fixture and the tracker of tests/test_gpu_mesh_events.py
    mask = DataArray(f["ev"], dims=("time", "ncells"),
                     coords={"time": ("time", f["time"]), "lat": ("ncells", f["lat"]), "lon": ("ncells", f["lon"])})
    trk = marex_amd.tracker(mask, DataArray(f["mask"], dims=("ncells",)), R_fill=1, area_filter_quartile=None, area_filter_absolute=5,
                            T_fill=2, overlap_threshold=THRESHOLD, nn_partitioning=True, unstructured_grid=True,
                            dimensions={"x": "ncells"}, coordinates={"x": "lon", "y": "lat"}, coordinate_units="degrees",
                            neighbours=DataArray(f["nb"], dims=("nv", "ncells")), cell_areas=DataArray(f["areas"], dims=("ncells",)),
                            timechunks=5)
    events = trk.run()
    ids = np.asarray(events["ID_field"].values)
    assert ids.max() >= 2
    later = mc.shifted(ids, 1)
    n = int(np.asarray(events["ID"].values).size) if "ID" in events else None
    ds = trk.event_matching(events, later, per_timestep=True)  # the tracker's areas and time values are the defaults
    mc.assert_dataset(ds, mo.matching(ids, later, np.asarray(f["areas"]), per_timestep=True, tv=np.asarray(f["time"]), n_a=n))
    v = {k: np.asarray(ds[k].values) for k in ds.data_vars}
    own = v["pair_ID_a"] == v["pair_ID_b"]
    assert own.sum() >= 2 and (v["pair_onset_lag"][own] == 1).all()
