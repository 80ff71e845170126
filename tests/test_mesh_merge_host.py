"""The split-and-merge stage on unstructured meshes, on the host: the reference's merging fixture through the NumPy oracle
(tests/mesh_merge_oracle.py) against the ranges the reference's own test accepts, the margin of every threshold decision,
the chord rule against a float64 haversine, the error paths that need no device, the limits on hand-built inputs, and the
host side of ``tracker.split_and_merge_objects_parallel`` over a NumPy stand-in for the engine -- no GPU needed."""
import os
import sys

import numpy as np
import pytest

import marex_amd
from marex_amd import zarr_io
from marex_amd.exceptions import ConfigurationError, TrackingError
from marex_amd.track_mesh import (check_temporary_id_ranges, mesh_nn_hop_cap, mesh_unit_vectors, plan_merge_step)
from marex_amd.xr_compat import DataArray, Dataset

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import mesh_merge_oracle as mm  # noqa: E402
import mesh_objects_oracle as mo  # noqa: E402
from mesh_merge_host_engine import use_host_engine  # noqa: E402
from test_mesh_tracker_host import mesh_tracker  # noqa: E402

FIX = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "ref_fixtures", "extremes_unstructured_merging.zarr")
THRESHOLD = 0.8  # the reference test's overlap_threshold (tests/test_unstructured_tracking.py)
# (nn_partitioning, timechunks) -> iterations; merges and events are the same in every configuration
CONFIGS = {(True, 100): 1, (True, 5): 3, (True, 2): 6, (False, 100): 1, (False, 5): 3, (False, 2): 6}
MERGES, EVENTS = 9, 11

_cache = {}


def load_merging_fixture():
    if "fix" not in _cache:
        rd = lambda v: zarr_io.read_array(os.path.join(FIX, v))  # noqa: E731
        f = {"ev": rd("extreme_events").astype(bool), "mask": rd("mask").astype(bool), "nb": rd("neighbours"),
             "areas": rd("cell_areas"), "lat": rd("lat"), "lon": rd("lon"), "time": rd("time")}
        f["nb0"] = np.maximum(f["nb"].astype(np.int64) - 1, -1).astype(np.int32)
        f["e"], f["q"] = mo.weight_tables(f["areas"], f["lat"], f["lon"])
        f["pre"], f["stats"] = mo.run_preprocess(f["ev"], f["mask"], f["nb0"], f["q"], f["e"], 1, 2, 0.5, 5)
        f["ids"] = mo.unique_ids_in_time(mo.identify_objects(f["pre"], f["mask"], f["nb0"])).astype(np.int32)
        _cache["fix"] = f
    return _cache["fix"]


def fixture_oracle(nn: bool, chunk: int):
    """The oracle's result on the fixture, computed once per configuration and shared (read only)."""
    key = ("oracle", nn, chunk)
    if key not in _cache:
        f = load_merging_fixture()
        _cache[key] = mm.split_and_merge(f["ids"], f["q"], f["e"], f["nb0"], f["areas"], f["lat"], f["lon"], THRESHOLD,
                                         [chunk] * (100 // chunk), nn)
    return _cache[key]


def props_dataset(ids, q, e):
    _, pid, _, area, cen = mo.object_properties(ids, q, e)
    coord = {"ID": ("ID", pid)}
    return Dataset({"area": DataArray(area, dims=("ID",), coords=coord),
                    "centroid": DataArray(cen, dims=("component", "ID"), coords=coord)}, coords=coord)


def assert_stage_equals_oracle(got, exp, time_values, what=""):
    """ID field, props (bitwise), pair list and every merge_events variable."""
    field, props, pairs, ev = got
    same = lambda a, b: a.dtype == b.dtype and a.shape == b.shape and a.tobytes() == b.tobytes()  # noqa: E731
    fv = np.asarray(field.values)
    assert fv.dtype == np.int32 and np.array_equal(fv, exp["field"]), what
    assert np.array_equal(np.asarray(props["ID"].values), exp["props"]["ID"]), what
    assert same(np.asarray(props["area"].values), exp["props"]["area"]), what
    assert same(np.asarray(props["centroid"].values), exp["props"]["centroid"]), what
    assert pairs.dtype == np.int32 and np.array_equal(pairs, exp["pairs"]), what
    for k in ("parent_IDs", "child_IDs", "overlap_areas", "n_parents", "n_children"):
        assert same(np.asarray(ev[k].values), exp["events"][k]), (what, k)
    assert np.array_equal(np.asarray(ev["merge_time"].values), np.asarray(time_values)[exp["events"]["merge_tidx"]]), what
    assert ev.attrs["fill_value"] == -1


# ------------------------------------------------------------------ 1-3: the reference's fixture through the oracle
def test_fixture_preprocessing_counts():
    f = load_merging_fixture()
    assert f["ev"].shape == (100, 405) and int(f["ev"].sum()) == 3426 and f["nb"].shape == (3, 405)
    st = f["stats"]
    assert (st[1], st[2], int(f["pre"].sum())) == (98, 98, 3408)
    assert abs(st[1] - 98) <= 2 and abs(st[2] - 97) <= 2  # the reference's ranges, tests/test_unstructured_tracking.py:257-258


@pytest.mark.parametrize("nn,chunk", list(CONFIGS), ids=[f"{'nn' if n else 'centroid'}-{c}" for n, c in CONFIGS])
def test_fixture_merging_counts(nn, chunk):
    r = fixture_oracle(nn, chunk)
    n_merges, n_events = len(r["merges"]), mm.count_events(r["pairs"], r["props"]["ID"])
    assert abs(n_merges - 9) <= 1 and abs(n_events - 12) <= 2  # the reference's ranges, tests/test_unstructured_tracking.py:259-260
    assert (n_merges, n_events, r["iterations"]) == (MERGES, EVENTS, CONFIGS[(nn, chunk)])
    assert r["field"].dtype == np.int32 and np.array_equal(r["field"] > 0, load_merging_fixture()["ids"] > 0)
    ids = r["props"]["ID"]
    assert np.array_equal(np.sort(ids), np.arange(1, ids.size + 1))  # the new IDs continue the old ones without a gap
    assert [m[0] for m in r["merges"]] == sorted(m[0] for m in r["merges"])
    if chunk < 100:  # the cross-chunk path: merges in later iterations come from the chunks' final lists
        assert max(m[0] for m in r["merges"]) >= 1


def test_no_decision_on_the_fixture_is_near_the_threshold():
    """The contract's areas differ from the reference's float32 sums by at most n 2^-24 relative (n cells), far less than
    the distance of any compared fraction from the threshold: no decision can flip."""
    r = fixture_oracle(True, 100)
    fr = r["fractions"][np.isfinite(r["fractions"])]
    gap = np.abs(fr - THRESHOLD).min()
    print(f"{fr.size} decisions, nearest {gap:.6f} from the threshold")
    assert fr.size == 235 and gap > 1e-3
    assert abs(gap - 0.0106) < 1e-4
    for key in CONFIGS:
        f2 = fixture_oracle(*key)["fractions"]
        assert np.abs(f2[np.isfinite(f2)] - THRESHOLD).min() > 1e-3


# ------------------------------------------------------------------ 4: the chord rule against a float64 haversine
def test_chord_rule_agrees_with_haversine_argmin():
    f = load_merging_fixture()
    lat, lon = f["lat"].astype(np.float64), f["lon"].astype(np.float64)
    u = mesh_unit_vectors(lat, lon)
    assert np.array_equal(u, mm.unit_vectors(lat, lon))
    la, lo = np.radians(lat)[:, None], np.radians(lon)[:, None]
    rng = np.random.default_rng(0)
    excluded = mismatches = compared = 0
    smallest = np.inf
    for _ in range(2000):
        k = int(rng.integers(2, 11))
        cen = np.stack([rng.uniform(lat.min(), lat.max(), k), rng.uniform(lon.min(), lon.max(), k)], axis=1).astype(np.float32)
        pla, plo = np.radians(cen[:, 0].astype(np.float64))[None, :], np.radians(cen[:, 1].astype(np.float64))[None, :]
        a = np.sin((pla - la) / 2) ** 2 + np.cos(la) * np.cos(pla) * np.sin((plo - lo) / 2) ** 2
        d = 2 * np.arctan2(np.sqrt(a), np.sqrt(1 - a))
        two = np.sort(d, axis=1)[:, :2]
        gap = two[:, 1] - two[:, 0]
        smallest = min(smallest, gap.min())
        keep = gap >= 1e-9
        excluded += int((~keep).sum())
        got = mm.nearest_centroid(u, mm.unit_vectors(cen[:, 0], cen[:, 1]))
        mismatches += int((got[keep] != np.argmin(d, axis=1)[keep]).sum())
        compared += int(keep.sum())
    print(f"{compared} cell-draws, {mismatches} mismatches, {excluded} excluded, smallest gap {smallest:.3g} rad")
    assert compared == 2000 * 405 and mismatches == 0 and excluded == 0


# ------------------------------------------------------------------ 5: error paths without a GPU
def _no_engine(monkeypatch, trk):
    def no_gpu():
        raise AssertionError("the stage touched the GPU engine")

    monkeypatch.setattr(trk, "_engine", no_gpu)


def _ring(C, seed=3):
    """A ring mesh with chords: ``(mask, nb 1-based, areas, lat, lon)``."""
    rng = np.random.default_rng(seed)
    nb = np.stack([(np.arange(C) + 1) % C + 1, (np.arange(C) - 1) % C + 1, rng.integers(0, C + 1, C)]).astype(np.int32)
    return dict(mask=np.ones(C, bool), nb=nb, areas=rng.uniform(1.0, 2.0, C).astype(np.float32),
                lat=20.0 * np.sin(2 * np.pi * np.arange(C) / C), lon=np.linspace(-170, 170, C))


def _mesh_stage_tracker(ids, mesh, **kw):
    return mesh_tracker(ids > 0, mesh["mask"], mesh["nb"], mesh["areas"], mesh["lat"], mesh["lon"], **kw)


def test_the_method_on_a_grid_points_to_the_gridded_algorithm(monkeypatch):
    ev = np.zeros((4, 6, 8), dtype=bool)
    da = DataArray(ev, dims=("time", "lat", "lon"),
                   coords={"time": np.arange(4), "lat": np.linspace(-80, 80, 6), "lon": np.linspace(0, 360, 8, endpoint=False)})
    trk = marex_amd.tracker(da, DataArray(np.ones((6, 8), bool), dims=("lat", "lon")), R_fill=1, area_filter_quartile=0.5,
                            allow_merging=False)
    _no_engine(monkeypatch, trk)
    with pytest.raises(ConfigurationError) as ei:
        trk.split_and_merge_objects_parallel(DataArray(np.zeros((4, 6, 8), np.int32), dims=("time", "lat", "lon")), None)
    assert "split_and_merge_objects" in " ".join(ei.value.suggestions)


def test_no_known_chunking_and_a_chunk_of_one_step_raise_before_any_device_work(monkeypatch):
    mesh = _ring(12)
    ids = np.zeros((5, 12), np.int32)
    ids[:, 3] = np.arange(1, 6)
    e, q = mo.weight_tables(mesh["areas"], mesh["lat"], mesh["lon"])
    trk = _mesh_stage_tracker(ids, mesh)  # constructs without any chunking, as before
    assert trk._time_chunks is None
    _no_engine(monkeypatch, trk)
    with pytest.raises(ConfigurationError) as ei:
        trk.split_and_merge_objects_parallel(DataArray(ids, dims=("time", "ncells")), props_dataset(ids, q, e))
    assert str(ei.value).startswith("split_and_merge_objects_parallel is not supported without a time chunking")
    for tc in (1, 2, 4):  # 5 steps: chunks of 1; 2 + 2 + 1; 4 + 1
        trk = _mesh_stage_tracker(ids, mesh, timechunks=tc)
        _no_engine(monkeypatch, trk)
        with pytest.raises(ConfigurationError) as ei:
            trk.split_and_merge_objects_parallel(DataArray(ids, dims=("time", "ncells")), props_dataset(ids, q, e))
        assert str(ei.value).startswith("split_and_merge_objects_parallel is not supported with a time chunk of one step")
        with pytest.raises(mm.OracleConfigurationError):
            mm.split_and_merge(ids, q, e, mesh["nb"] - 1, mesh["areas"], mesh["lat"], mesh["lon"], 0.5,
                               trk._time_chunks, True)


def test_the_six_methods_that_need_cluster_renaming_still_raise_and_name_the_new_stage():
    from marex_amd.track_mesh import _not_built

    err = _not_built("tracker.run")
    assert str(err).startswith("tracker.run is not built for unstructured grids: the split-and-merge stage is missing")
    assert "split_and_merge_objects_parallel" in err.details.split("; the reference's")[0]


# ------------------------------------------------------------------ 6: the limits, on hand-built inputs
def _run_both(monkeypatch, ids, mesh, chunks, thr, nn, max_iteration=40):
    """``(product over the host engine, oracle)``: each either a result or the exception it raised."""
    e, q = mo.weight_tables(mesh["areas"], mesh["lat"], mesh["lon"])
    assert len(set(chunks)) == 1 or (len(set(chunks[:-1])) == 1 and chunks[-1] <= chunks[0])
    trk = _mesh_stage_tracker(ids, mesh, timechunks=chunks[0], overlap_threshold=thr, nn_partitioning=nn,
                              max_iteration=max_iteration)
    assert trk._time_chunks == list(chunks)
    use_host_engine(monkeypatch, trk)
    out = []
    for run in (lambda: trk.split_and_merge_objects_parallel(DataArray(ids, dims=("time", "ncells")), props_dataset(ids, q, e)),
                lambda: mm.split_and_merge(ids, q, e, mesh["nb"] - 1, mesh["areas"], mesh["lat"], mesh["lon"], thr, chunks, nn,
                                           max_iteration)):
        try:
            out.append(run())
        except (TrackingError, mm.OracleTrackingError) as err:
            out.append(err)
    return trk, out[0], out[1]


def _eleven_parents(n_par):
    ids = np.zeros((2, 40), np.int32)
    for k in range(n_par):
        ids[0, 2 * k:2 * k + 2] = k + 1
    ids[1, :2 * n_par] = n_par + 1
    return ids


@pytest.mark.parametrize("nn", [True, False])
def test_an_eleventh_parent_raises(monkeypatch, nn):
    mesh = _ring(40)
    trk, got, exp = _run_both(monkeypatch, _eleven_parents(11), mesh, [2], 0.05, nn)
    assert isinstance(got, TrackingError) and str(got).startswith("Too many parent objects for tracking")
    assert isinstance(exp, mm.OracleTrackingError) and str(exp) == "Too many parent objects for tracking"
    trk, got, exp = _run_both(monkeypatch, _eleven_parents(10), mesh, [2], 0.05, nn)  # ten are the limit, not beyond it
    assert_stage_equals_oracle(got, exp, np.arange(2))
    assert len(exp["merges"]) == 1 and len(exp["merges"][0][3]) == 10 and exp["props"]["ID"].size == 20


def _many_merges(n):
    ids = np.zeros((2, 87), np.int32)
    for k in range(n):
        ids[0, 4 * k:4 * k + 2], ids[0, 4 * k + 2:4 * k + 4] = 2 * k + 1, 2 * k + 2
        ids[1, 4 * k:4 * k + 4] = 2 * n + k + 1
    return ids


def test_a_twenty_first_merge_in_one_timestep_raises(monkeypatch):
    mesh = _ring(87)
    trk, got, exp = _run_both(monkeypatch, _many_merges(21), mesh, [2], 0.3, True)
    assert isinstance(got, TrackingError) and str(got).startswith("Too many merge operations")
    assert isinstance(exp, mm.OracleTrackingError) and str(exp) == "Too many merge operations"
    trk, got, exp = _run_both(monkeypatch, _many_merges(20), mesh, [2], 0.3, True)
    assert_stage_equals_oracle(got, exp, np.arange(2))
    assert len(exp["merges"]) == 20


def _collision_field(n_par):
    """t = 1: a child of ``n_par`` parents; t = 2: a child of two parents elsewhere.  With one merging object per timestep
    and one chunk of 4 steps the temporary IDs of consecutive timesteps lie 4 apart."""
    ids = np.zeros((4, 40), np.int32)
    for k in range(n_par):
        ids[0, 2 * k:2 * k + 2] = k + 1
    ids[1, :2 * n_par] = 20
    ids[1, 20:24], ids[1, 24:28] = 21, 22
    ids[2, 20:28] = 23
    return ids


@pytest.mark.parametrize("nn", [True, False])
def test_two_timesteps_drawing_the_same_temporary_id_raise(monkeypatch, nn):
    mesh = _ring(40)
    trk, got, exp = _run_both(monkeypatch, _collision_field(6), mesh, [4], 0.3, nn)  # 5 new IDs at t = 1 reach the base of t = 2
    assert isinstance(got, TrackingError) and str(got).startswith("Temporary object IDs of two timesteps collide")
    assert isinstance(exp, mm.OracleTrackingError) and str(exp) == "Temporary IDs of two timesteps collide"
    trk, got, exp = _run_both(monkeypatch, _collision_field(5), mesh, [4], 0.3, nn)  # 4 new IDs end where t = 2 begins
    assert_stage_equals_oracle(got, exp, np.arange(4))
    assert [len(m[3]) for m in exp["merges"]] == [5, 2] and exp["props"]["ID"].max() == 23 + 5
    with pytest.raises(TrackingError):
        check_temporary_id_ranges({1: (30, 35), 2: (34, 35)})
    check_temporary_id_ranges({1: (30, 34), 2: (34, 35), 3: (38, 38)})


def test_max_iteration_is_no_longer_ignored_on_meshes(monkeypatch):
    mesh = _ring(40)
    ids = _collision_field(2)
    for max_iteration, fails in ((1, True), (2, False)):  # one iteration is needed; reaching max_iteration raises (track.py:4732)
        trk, got, exp = _run_both(monkeypatch, ids, mesh, [4], 0.3, True, max_iteration=max_iteration)
        if fails:
            assert isinstance(got, TrackingError) and str(got).startswith("Maximum iterations reached in tracking algorithm")
            assert isinstance(exp, mm.OracleTrackingError) and str(exp) == "Maximum iterations reached in tracking algorithm"
        else:
            assert_stage_equals_oracle(got, exp, np.arange(4))
            assert exp["iterations"] == 1
    f = load_merging_fixture()  # chunks of 2 need six iterations
    with pytest.raises(mm.OracleTrackingError):
        mm.split_and_merge(f["ids"], f["q"], f["e"], f["nb0"], f["areas"], f["lat"], f["lon"], THRESHOLD, [2] * 50, True, 6)


def test_plan_merge_step_reads_the_tables_as_the_oracle_reads_the_slices():
    ov = np.array([[1, 9, 2.0], [2, 9, 0.5], [3, 9, 2.0], [4, 8, 1.0]], np.float32)
    area_prev = {1: np.float32(2.0), 2: np.float32(2.0), 3: np.float32(4.0), 4: np.float32(1.0)}
    area_cur = {8: np.float32(1.0), 9: np.float32(6.0)}
    plan, nxt = plan_merge_step(3, [9, 8, 7], ov, area_prev, area_cur, 0.5, 100)
    assert nxt == 101 and len(plan) == 1  # parent 2 (0.25) is skipped; 0.5 >= 0.5 keeps parent 3; child 8 has one parent
    assert plan[0]["child_ids"] == [9, 100] and plan[0]["parents"] == [1, 3] and plan[0]["areas"] == [2.0, 2.0]
    assert mesh_nn_hop_cap([np.float32(4.0), np.float32(900.0)], 1.0) == 120 and mesh_nn_hop_cap([np.float32(4.0)], 1.0) == 40
    assert mesh_nn_hop_cap([np.float32(900.0)], 1.0) == mm.hop_cap(np.array([900.0], np.float32), 1.0)


# ------------------------------------------------------------------ the stage's host side over the NumPy engine
@pytest.mark.parametrize("nn,chunk", list(CONFIGS), ids=[f"{'nn' if n else 'centroid'}-{c}" for n, c in CONFIGS])
def test_host_side_of_the_stage_equals_the_oracle_on_the_fixture(monkeypatch, nn, chunk):
    f = load_merging_fixture()
    trk = mesh_tracker(f["pre"], f["mask"], f["nb"], f["areas"], f["lat"], f["lon"], tm=f["time"], R_fill=1, T_fill=2,
                       area_filter_quartile=None, area_filter_absolute=5, overlap_threshold=THRESHOLD, nn_partitioning=nn,
                       timechunks=chunk)
    eng = use_host_engine(monkeypatch, trk)
    got = trk.split_and_merge_objects_parallel(DataArray(f["ids"], dims=("time", "ncells")), props_dataset(f["ids"], f["q"], f["e"]))
    exp = fixture_oracle(nn, chunk)
    assert_stage_equals_oracle(got, exp, f["time"], (nn, chunk))
    assert trk._merge_stats["iterations"] == CONFIGS[(nn, chunk)] and trk._merge_stats["partitions"] == MERGES
    if nn:
        assert [(i["hops"], i["leftover"]) for i in eng.nn_calls] == [(i["hops"], i["leftover"]) for i in exp["nn"]]


@pytest.mark.parametrize("nn", [True, False])
def test_host_side_of_the_stage_equals_the_oracle_on_drifting_runs(monkeypatch, nn):
    """Three parents, several iterations, merges in several chunks of 3 + 3 + 2 steps (the scenario of the GPU tests)."""
    from mesh_merge_scenarios import drifting_runs

    mesh, ids = drifting_runs(1, 200)
    e, q = mo.weight_tables(mesh["areas"], mesh["lat"], mesh["lon"])
    exp = mm.split_and_merge(ids, q, e, mesh["nb0"], mesh["areas"], mesh["lat"], mesh["lon"], 0.3, [3, 3, 2], nn)
    assert max(len(m[3]) for m in exp["merges"]) >= 3 and exp["iterations"] >= 2
    assert len({min(m[1] // 3, 2) for m in exp["merges"]}) >= 2
    trk = mesh_tracker(ids > 0, mesh["mask"], mesh["nb0"] + 1, mesh["areas"], mesh["lat"], mesh["lon"], overlap_threshold=0.3,
                       nn_partitioning=nn, timechunks=3)
    use_host_engine(monkeypatch, trk)
    got = trk.split_and_merge_objects_parallel(DataArray(ids, dims=("time", "ncells")), props_dataset(ids, q, e))
    assert_stage_equals_oracle(got, exp, np.arange(8), nn)
