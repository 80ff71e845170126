"""Cluster renaming and ``track_objects`` on unstructured meshes, on the host: the stage and the whole chain over a NumPy
stand-in for the engine (tests/mesh_events_host_engine.py) against the events oracle (tests/mesh_events_oracle.py) on the
reference's two mesh fixtures, on drifting runs and on hand-built fields; the guard of the four methods that need a time
chunking; and the distance of the event areas and coordinate sums from the reference's float32 sums -- no GPU needed.  The
stand-in answers the rename pass with the oracle's own function: what is compared here is the host side of the stage, the
device pass itself is compared with NumPy in tests/test_gpu_mesh_events.py."""
import os
import sys

import numpy as np
import pytest

from marex_amd.exceptions import ConfigurationError
from marex_amd.xr_compat import DataArray, Dataset

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import mesh_events_oracle as me  # noqa: E402
import mesh_merge_oracle as mm  # noqa: E402
import mesh_objects_oracle as mo  # noqa: E402
from mesh_events_host_engine import use_events_host_engine  # noqa: E402
from mesh_merge_scenarios import drifting_runs  # noqa: E402
from test_mesh_merge_host import EVENTS, MERGES, THRESHOLD, fixture_oracle, load_merging_fixture  # noqa: E402
from test_mesh_tracker_host import _contract_distance, load_mesh_fixture, mesh_tracker  # noqa: E402

EVENT_VARS = ("ID_field", "global_ID", "area", "centroid", "presence", "merge_ledger")
_cache = {}


def same(a, b):
    a, b = np.asarray(a), np.asarray(b)
    return a.dtype == b.dtype and a.shape == b.shape and a.tobytes() == b.tobytes()


def assert_events_equal(ds, exp, what=""):
    """Every variable of the events Dataset against the oracle's, floats bit for bit; dims and the ID coordinate."""
    for k in EVENT_VARS:
        assert same(ds[k].values, exp[k]), (what, k)
    for k in ("time_start", "time_end"):
        assert np.array_equal(np.asarray(ds[k].values), exp[k]), (what, k)
    N = exp["N"]
    assert tuple(ds["ID_field"].dims) == ("time", "ncells") and tuple(ds["centroid"].dims) == ("component", "time", "ID")
    assert tuple(ds["merge_ledger"].dims) == ("time", "ID", "sibling_ID") and tuple(ds["area"].dims) == ("time", "ID")
    assert np.array_equal(np.asarray(ds["ID"].values), np.arange(1, N + 1)) and np.asarray(ds["global_ID"].values).shape[1] == N


def merges_dataset(events, time_values):
    """The merge_events Dataset of the oracle's records (what split_and_merge_objects_parallel hands on)."""
    tm = np.asarray(time_values)[events["merge_tidx"]]
    return Dataset({"parent_IDs": DataArray(events["parent_IDs"], dims=("merge_ID", "parent_idx")),
                    "child_IDs": DataArray(events["child_IDs"], dims=("merge_ID", "child_idx")),
                    "merge_time": DataArray(tm, dims=("merge_ID",)),
                    "n_parents": DataArray(events["n_parents"], dims=("merge_ID",))})


def assert_merges_equal(ds, events, time_values, what=""):
    for k in ("parent_IDs", "child_IDs", "overlap_areas", "n_parents", "n_children"):
        assert same(ds[k].values, events[k]), (what, k)
    assert np.array_equal(np.asarray(ds["merge_time"].values), np.asarray(time_values)[events["merge_tidx"]]), what


def fixture_tracker(f, nn, chunk, **kw):
    args = dict(tm=f["time"], R_fill=1, T_fill=2, area_filter_quartile=None, area_filter_absolute=5, overlap_threshold=THRESHOLD,
                nn_partitioning=nn, timechunks=chunk)
    args.update(kw)
    return mesh_tracker(f["pre"], f["mask"], f["nb"], f["areas"], f["lat"], f["lon"], **args)


def fixture_events(nn, chunk):
    """The events oracle over the split-and-merge oracle on the merging fixture, computed once and shared (read only)."""
    key = ("events", nn, chunk)
    if key not in _cache:
        f, r = load_merging_fixture(), fixture_oracle(nn, chunk)
        _cache[key] = me.cluster_rename(r["field"], r["pairs"], r["events"], f["q"], f["e"], f["time"])
    return _cache[key]


def run_stage(monkeypatch, trk, field, pairs, events, time_values):
    eng = use_events_host_engine(monkeypatch, trk)
    before = field.copy()
    ds = trk.cluster_rename_objects_and_props(DataArray(field, dims=("time", "ncells")), None, pairs,
                                              merges_dataset(events, time_values))
    assert np.array_equal(field, before) and eng.calls == ["mesh_event_rename"] * (1 if np.any(field > 0) else 0)
    return ds


# ------------------------------------------------------------------ the stage and the chain on the merging fixture
@pytest.mark.parametrize("nn,chunk", [(True, 100), (True, 5), (False, 2)], ids=["nn-100", "nn-5", "centroid-2"])
def test_stage_equals_the_oracle_on_the_merging_fixture(monkeypatch, nn, chunk):
    f, r = load_merging_fixture(), fixture_oracle(nn, chunk)
    exp = fixture_events(nn, chunk)
    ds = run_stage(monkeypatch, fixture_tracker(f, nn, chunk), r["field"], r["pairs"], r["events"], f["time"])
    assert_events_equal(ds, exp, (nn, chunk))
    assert ds.sizes["ID"] == EVENTS == exp["N"]
    led = np.asarray(ds["merge_ledger"].values)
    assert led.shape[2] == r["events"]["parent_IDs"].shape[1] and (led > 0).any()  # merges are on the ledger


def test_track_objects_equals_the_oracle_chain_on_the_merging_fixture(monkeypatch):
    f, r, exp = load_merging_fixture(), fixture_oracle(True, 5), fixture_events(True, 5)
    trk = fixture_tracker(f, True, 5)
    eng = use_events_host_engine(monkeypatch, trk)
    events_ds, merges_ds, N = trk.track_objects(trk.data_bin)
    assert eng.calls == ["label_objects_mesh", "unique_ids_in_time", "mesh_event_rename"]
    assert_events_equal(events_ds, exp, "track_objects")
    assert_merges_equal(merges_ds, r["events"], f["time"], "track_objects")
    n_merges = len(np.asarray(merges_ds["n_parents"].values))
    assert (N, n_merges) == (EVENTS, MERGES) == (11, 9)
    assert abs(N - 12) <= 2 and abs(n_merges - 9) <= 1  # the reference's ranges, tests/test_unstructured_tracking.py:259-260
    assert set(trk._stage_times) == {"objects", "split_and_merge", "cluster_rename"}
    ds2, merges2, N2 = trk.run_tracking(trk.data_bin)  # run_tracking on a mesh is track_objects
    assert N2 == N and same(ds2["ID_field"].values, exp["ID_field"])


# ------------------------------------------------------------------ drifting runs
@pytest.mark.parametrize("seed,C", [(1, 200), (7, 4097)])
@pytest.mark.parametrize("nn", [True, False], ids=["nn", "centroid"])
def test_stage_equals_the_oracle_on_drifting_runs(monkeypatch, nn, seed, C):
    mesh, ids = drifting_runs(seed, C)
    e, q = mo.weight_tables(mesh["areas"], mesh["lat"], mesh["lon"])
    r = mm.split_and_merge(ids, q, e, mesh["nb0"], mesh["areas"], mesh["lat"], mesh["lon"], 0.3, [3, 3, 2], nn)
    exp = me.cluster_rename(r["field"], r["pairs"], r["events"], q, e, np.arange(8))
    assert len(r["merges"]) >= 1 and 1 <= exp["N"] < r["props"]["ID"].size
    trk = mesh_tracker(ids > 0, mesh["mask"], mesh["nb0"] + 1, mesh["areas"], mesh["lat"], mesh["lon"], overlap_threshold=0.3,
                       nn_partitioning=nn, timechunks=3)
    ds = run_stage(monkeypatch, trk, r["field"], r["pairs"], r["events"], np.arange(8))
    assert_events_equal(ds, exp, (nn, seed, C))


# ------------------------------------------------------------------ the second fixture
def second_fixture():
    if "second" not in _cache:
        f = load_mesh_fixture()
        f["nb0"] = np.maximum(f["nb"].astype(np.int64) - 1, -1).astype(np.int32)
        f["e"], f["q"] = mo.weight_tables(f["areas"], f["lat"], f["lon"])
        f["pre"], f["stats"] = mo.run_preprocess(f["ev"], f["mask"], f["nb0"], f["q"], f["e"], 3, 2, 0.5)
        f["ids"] = mo.unique_ids_in_time(mo.identify_objects(f["pre"], f["mask"], f["nb0"])).astype(np.int32)
        _cache["second"] = f
    return _cache["second"]


def second_fixture_chain(nn, chunk):
    """Split-and-merge oracle -> events oracle on extremes_unstructured.zarr (R_fill=3, T_fill=2, quartile 0.5, overlap
    threshold 0.5), once per configuration."""
    key = ("second", nn, chunk)
    if key not in _cache:
        f = second_fixture()
        T = f["ids"].shape[0]
        chunks = [min(chunk, T - s) for s in range(0, T, chunk)]
        r = mm.split_and_merge(f["ids"], f["q"], f["e"], f["nb0"], f["areas"], f["lat"], f["lon"], 0.5, chunks, nn)
        _cache[key] = (r, me.cluster_rename(r["field"], r["pairs"], r["events"], f["q"], f["e"], f["time"]))
    return _cache[key]


@pytest.mark.parametrize("chunk", [100, 5, 2])
@pytest.mark.parametrize("nn", [True, False], ids=["nn", "centroid"])
def test_second_fixture_has_three_events_and_no_merges(monkeypatch, nn, chunk):
    f = second_fixture()
    r, exp = second_fixture_chain(nn, chunk)
    assert len(r["merges"]) == 0 and exp["N"] == 3 and abs(exp["N"] - 3) <= 1  # the reference accepts 3 +- 1
    assert exp["merge_ledger"].shape[2] == 1 and (exp["merge_ledger"] == -1).all()
    trk = mesh_tracker(f["ev"], f["mask"], f["nb"], f["areas"], f["lat"], f["lon"], tm=f["time"], R_fill=3, T_fill=2,
                       area_filter_quartile=0.5, nn_partitioning=nn, timechunks=chunk)
    use_events_host_engine(monkeypatch, trk)
    events_ds, merges_ds, N = trk.track_objects(DataArray(f["pre"], dims=("time", "ncells")))
    assert N == 3 and events_ds.sizes["ID"] == 3 and len(np.asarray(merges_ds["n_parents"].values)) == 0
    led = np.asarray(events_ds["merge_ledger"].values)
    assert led.shape == (f["ids"].shape[0], 3, 1) and (led == -1).all()
    assert_events_equal(events_ds, exp, (nn, chunk))


# ------------------------------------------------------------------ hand-built fields
def _hand_mesh(C=24):
    rng = np.random.default_rng(5)
    nb = np.stack([(np.arange(C) + 1) % C + 1, (np.arange(C) - 1) % C + 1, np.zeros(C, np.int64)]).astype(np.int32)
    return dict(mask=np.ones(C, bool), nb=nb, areas=rng.uniform(1.0, 3.0, C).astype(np.float32),
                lat=np.linspace(-50, 50, C), lon=np.linspace(-170, 170, C))


NO_MERGES = mm.merge_events([])


def _hand_stage(monkeypatch, field, pairs, events=NO_MERGES, **kw):
    mesh = _hand_mesh(field.shape[1])
    e, q = mo.weight_tables(mesh["areas"], mesh["lat"], mesh["lon"])
    tm = 10 * np.arange(field.shape[0]) + 3
    exp = me.cluster_rename(field, pairs, events, q, e, tm)
    trk = mesh_tracker(field > 0, mesh["mask"], mesh["nb"], mesh["areas"], mesh["lat"], mesh["lon"], tm=tm, timechunks=2, **kw)
    ds = run_stage(monkeypatch, trk, field, np.asarray(pairs, np.int32).reshape(-1, 2), events, tm)
    assert_events_equal(ds, exp)
    return ds, exp, (mesh, q, e, tm)


def test_an_event_of_two_disjoint_objects_in_one_timestep(monkeypatch):
    field = np.zeros((2, 24), np.int32)
    field[0, 2:5] = 1
    field[1, 1:4], field[1, 15:19] = 2, 3      # both follow object 1: one event, disjoint at t = 1
    ds, exp, (mesh, q, e, tm) = _hand_stage(monkeypatch, field, [[1, 2], [1, 3]])
    assert exp["N"] == 1 and np.asarray(ds["global_ID"].values).tolist() == [[1], [3]]  # the larger of 2 and 3
    both = (field[1] == 2) | (field[1] == 3)
    S = np.array([[q[k][both].sum(dtype=np.int64)] for k in range(4)])
    area, cen = mo._finish(S, e)
    assert same(np.asarray(ds["area"].values)[1], area) and same(np.asarray(ds["centroid"].values)[:, 1, :], cen)
    assert abs(float(area[0]) - float(mesh["areas"][both].astype(np.float64).sum())) < 1e-5 * float(area[0])
    assert np.asarray(ds["ID_field"].values)[1][both].tolist() == [1] * 7


def test_an_event_absent_in_a_middle_timestep(monkeypatch):
    field = np.zeros((4, 24), np.int32)
    field[0, 3:6], field[1, 3:6], field[3, 4:7] = 1, 2, 4     # nothing at t = 2
    field[1, 12:14], field[2, 12:14] = 3, 5                   # a second event, present at t = 1, 2
    ds, exp, (_, _, _, tm) = _hand_stage(monkeypatch, field, [[1, 2], [2, 4], [3, 5]])
    assert exp["N"] == 2
    pres = np.asarray(ds["presence"].values)
    assert pres[:, 0].tolist() == [True, True, False, True] and pres[:, 1].tolist() == [False, True, True, False]
    area, cen = np.asarray(ds["area"].values), np.asarray(ds["centroid"].values)
    assert np.isnan(area[2, 0]) and np.isnan(cen[:, 2, 0]).all() and np.isfinite(area[[0, 1, 3], 0]).all()
    assert np.array_equal(np.isnan(area), ~pres) and np.array_equal(np.isnan(cen[0]), ~pres) and np.array_equal(np.isnan(cen[1]), ~pres)
    assert np.asarray(ds["time_start"].values).tolist() == [tm[0], tm[1]] and np.asarray(ds["time_end"].values).tolist() == [tm[3], tm[2]]


def test_an_id_in_the_pairs_but_not_in_the_field(monkeypatch):
    field = np.zeros((3, 24), np.int32)
    field[0, 2:5], field[2, 2:5], field[1, 10:12] = 1, 4, 5   # ID 3 was at t = 1 once; the pairs still name it
    ds, exp, _ = _hand_stage(monkeypatch, field, [[1, 3], [3, 4]])
    assert exp["N"] == 2 and np.asarray(ds["global_ID"].values).tolist() == [[1, 0], [0, 5], [4, 0]]
    ds, exp, _ = _hand_stage(monkeypatch, field, [[1, 2]])    # ID 2 on its own side: 1 and 2 form an event, 4 and 5 their own
    assert exp["N"] == 3 and np.asarray(ds["global_ID"].values).tolist() == [[1, 0, 0], [0, 0, 5], [0, 4, 0]]


def test_an_all_zero_field_gives_the_empty_dataset(monkeypatch):
    ds, exp, _ = _hand_stage(monkeypatch, np.zeros((3, 24), np.int32), np.zeros((0, 2), np.int32))
    assert exp["N"] == 0 and ds.sizes["ID"] == 0 and np.asarray(ds["ID"].values).size == 0
    assert np.asarray(ds["area"].values).shape == (3, 0) and np.asarray(ds["centroid"].values).shape == (2, 3, 0)
    assert np.asarray(ds["merge_ledger"].values).shape == (3, 0, 1) and not np.asarray(ds["ID_field"].values).any()


def test_merges_land_on_the_ledger_of_their_timestep(monkeypatch):
    field = np.zeros((3, 24), np.int32)
    field[0, 2:4], field[0, 6:8], field[1, 2:5], field[1, 5:8], field[2, 3:7] = 1, 2, 3, 4, 5
    merges = [(0, 1, [3, 4], [1, 2], [np.float32(1.0), np.float32(1.0)])]  # (iteration, t, children, parents, overlaps)
    ds, exp, _ = _hand_stage(monkeypatch, field, [[1, 3], [2, 4], [3, 5]], mm.merge_events(merges))
    assert exp["N"] == 2
    led = np.asarray(ds["merge_ledger"].values)
    assert led.shape == (3, 2, 2) and led[1].tolist() == [[1, 1], [2, 2]] and (led[[0, 2]] == -1).all()


# ------------------------------------------------------------------ the guard
def test_the_four_methods_need_a_time_chunking_and_say_so_before_the_engine_is_touched(monkeypatch):
    mesh = _hand_mesh()
    field = np.zeros((4, 24), np.int32)
    field[:, 3:6] = np.arange(1, 5)[:, None]

    def touched():
        raise AssertionError("the method touched the engine")

    def calls(t):
        x = DataArray(field > 0, dims=("time", "ncells"))
        return {"tracker.run": lambda: t.run(), "tracker.run_tracking": lambda: t.run_tracking(x),
                "tracker.track_objects": lambda: t.track_objects(x),
                "tracker.cluster_rename_objects_and_props":
                    lambda: t.cluster_rename_objects_and_props(DataArray(field, dims=("time", "ncells")), None, None, None)}

    trk = mesh_tracker(field > 0, mesh["mask"], mesh["nb"], mesh["areas"], mesh["lat"], mesh["lon"])
    assert trk._time_chunks is None
    monkeypatch.setattr(trk, "_engine", touched)
    for what, call in calls(trk).items():
        with pytest.raises(ConfigurationError) as ei:
            call()
        assert str(ei.value).startswith(f"{what} is not built for unstructured grids: the split-and-merge stage has no time "
                                        "chunking to walk")
        assert ei.value.suggestions == ["Pass timechunks=<steps per chunk>", "Chunk data_bin in time"]
    with pytest.raises(ConfigurationError, match="tracker.run is not built for unstructured grids"):
        trk.run(return_merges=True)
    trk = mesh_tracker(field > 0, mesh["mask"], mesh["nb"], mesh["areas"], mesh["lat"], mesh["lon"], timechunks=2)
    monkeypatch.setattr(trk, "_engine", touched)
    for what, call in calls(trk).items():  # past the guard: the first thing they meet is the engine
        with pytest.raises(AssertionError, match="the method touched the engine"):
            call()


# ------------------------------------------------------------------ the arithmetic contract on events
def test_event_sums_lie_inside_the_rounding_bound_of_the_reference_sums():
    """An event's area and weighted coordinate sums are integer sums of the same fixed-point weights as an object's, over
    the cells of all its objects of the timestep: the bounds objects are held to (n 2^-24 relative for the area,
    (n + 4) 2^-24 sum |a x| for the coordinates, tests/test_mesh_tracker_host.py) hold with n the cells of the event."""
    f = load_merging_fixture()
    field = fixture_events(True, 100)["ID_field"]
    wa, wc, big = _contract_distance(field, f["areas"], f["lat"], f["lon"])
    print(f"events of the merging fixture: area {wa:.3f} of its bound, coordinates {wc:.3f}, largest event-step {big} cells")
    assert wa <= 1.0 and wc <= 1.0
