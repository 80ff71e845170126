"""The event matching on the host: the oracle against hand-computed values, the validation errors (raised before any device
work), the empty cases, the widths and the key at their corners, and the public path -- the area table, windows, the sort and
the host finish -- on a NumPy stand-in for the engine call.  No GPU needed."""
import os
import sys

import numpy as np
import pytest

import marex_amd
import marex_amd._stream as mi
import marex_amd.matching as mm
from marex_amd.engine import HotPath
from marex_amd.exceptions import ConfigurationError, DataValidationError, ProcessingError
from marex_amd.xr_compat import DataArray

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import event_matching_cases as mc  # noqa: E402
import event_matching_oracle as mo  # noqa: E402
from event_matching_host_engine import HostEngine  # noqa: E402

NAN = np.nan


def test_oracle_on_a_hand_computed_pair_of_fields():
    #             cell 0  1  2  3  4  5
    a = np.array([[1, 1, 1, 1, 0, 2],
                  [0, 1, 1, 0, 0, 2],
                  [0, 0, 0, 0, 0, 0],
                  [3, 0, 0, 0, 0, 0]], np.int32)
    b = np.array([[0, 0, 0, 0, 0, 0],
                  [0, 5, 5, 5, 0, 1],
                  [0, 5, 0, 0, 0, 1],
                  [0, 0, 0, 0, 4, 0]], np.int32)
    areas = np.array([1.0, 2.0, 1.0, 0.5, 4.0, 1.0])
    recs = mo.step_records(a, b)
    assert [(d["a"], d["b"], d["t"], d["cells"]) for d in recs] == [
        (0, 1, 2, 1), (0, 4, 3, 1), (0, 5, 1, 1), (0, 5, 2, 1), (1, 0, 0, 4), (1, 5, 1, 2), (2, 0, 0, 1), (2, 1, 1, 1), (3, 0, 3, 1)]
    o, c = mo.matching(a, b, areas, per_timestep=True)
    assert c["ID_a"].tolist() == [1, 2, 3] and c["ID_b"].tolist() == [1, 2, 3, 4, 5]
    assert o["pair_ID_a"].tolist() == [1, 2] and o["pair_ID_b"].tolist() == [5, 1]
    assert o["pair_steps"].tolist() == [1, 1] and o["pair_time_start"].tolist() == [1, 1] and o["pair_cell_steps"].tolist() == [2, 1]
    assert o["pair_area_steps"].tolist() == [3.0, 1.0] and o["pair_area_max"].tolist() == [3.0, 1.0]
    # event 1 of A: 4.5 + 3 area-steps; event 5 of B: 3.5 + 2; event 2 of A: 1 + 1; event 1 of B: 1 + 1
    assert o["pair_share_of_a"].tolist() == [3.0 / 7.5, 0.5] and o["pair_share_of_b"].tolist() == [3.0 / 5.5, 0.5]
    assert o["pair_iou"].tolist() == [3.0 / 10.0, 1.0 / 3.0]
    assert o["pair_onset_lag"].tolist() == [1, 1] and o["pair_end_lag"].tolist() == [1, 1]
    assert o["a_steps"].tolist() == [2, 2, 1] and o["a_cell_steps"].tolist() == [6, 2, 1] and o["a_area_steps"].tolist() == [7.5, 2.0, 1.0]
    assert o["a_matches"].tolist() == [1, 1, 0] and o["a_best_match"].tolist() == [5, 1, 0]
    assert o["a_best_share"].tolist() == [0.4, 0.5, 0.0] and o["a_matched_share"].tolist() == [0.4, 0.5, 0.0]
    assert o["b_steps"].tolist() == [2, 0, 0, 1, 2] and o["b_matches"].tolist() == [1, 0, 0, 0, 1] and o["b_best_match"].tolist() == [2, 0, 0, 0, 1]
    assert np.array_equal(o["b_matched_share"], [0.5, NAN, NAN, 0.0, 3.0 / 5.5], equal_nan=True)
    assert (int(o["n_a"]), int(o["n_b"]), int(o["matched_a"]), int(o["matched_b"])) == (3, 3, 2, 2)
    assert float(o["pod"]) == 2 / 3 and float(o["far"]) == 1 - 2 / 3 and float(o["csi"]) == 2 / 4
    assert (int(o["cell_steps_both"]), int(o["cell_steps_only_a"]), int(o["cell_steps_only_b"])) == (3, 6, 4)
    assert (float(o["area_steps_both"]), float(o["area_steps_only_a"]), float(o["area_steps_only_b"])) == (4.0, 6.5, 7.5)
    assert o["step_cells_both"].tolist() == [0, 3, 0, 0] and o["step_cells_only_a"].tolist() == [5, 0, 0, 1]
    assert o["step_cells_only_b"].tolist() == [0, 1, 2, 1]
    assert o["pair_record_offsets"].tolist() == [0, 1, 2] and o["record_time"].tolist() == [1, 1] and o["record_area"].tolist() == [3.0, 1.0]
    o, _ = mo.matching(a, b)  # without areas: cells
    assert o["pair_area_steps"].tolist() == [2.0, 1.0] and "record_time" not in o


def _no_gpu(monkeypatch):
    import marex_amd.detect as det

    def no_gpu(*a, **k):
        raise AssertionError("the call touched the GPU engine")

    monkeypatch.setattr(det, "get_engine", no_gpu)


def test_every_refusal_comes_before_the_device(monkeypatch):
    _no_gpu(monkeypatch)
    x = np.zeros((3, 4, 5), np.int32)
    V, Cf = DataValidationError, ConfigurationError
    dims = ("time", "y", "x")
    tx = DataArray(x, dims=dims, coords={"time": ("time", np.arange(3))})
    cases = [
        (dict(ID_field_b=x[:2]), V, "ID_field_a and ID_field_b differ in shape"),
        (dict(ID_field_b=x.reshape(3, 20)), V, "ID_field_a and ID_field_b differ in shape"),
        (dict(ID_field_a=DataArray(x[:, :4, :4], dims=dims), ID_field_b=DataArray(x[:, :4, :4], dims=("time", "x", "y"))), V,
         "ID_field_a and ID_field_b differ in their dimensions"),
        (dict(ID_field_a=tx, ID_field_b=DataArray(x, dims=dims, coords={"time": ("time", np.arange(1, 4))})), V,
         "ID_field_a and ID_field_b differ in their time coordinate"),
        (dict(ID_field_a=x.astype(bool)), V, "event_matching needs ID fields, not masks"),
        (dict(ID_field_b=x.astype(np.uint8)), V, "event_matching needs ID fields, not masks"),
        (dict(ID_field_b=x.astype(np.float32)), V, "field must be a mask .* or an integer ID field"),
        (dict(ID_field_b=None), V, "event_matching needs two ID fields"),
        (dict(ID_field_a=x[0, 0], ID_field_b=x[0, 0]), V, r"field must be \(time, y, x\) or \(time, cells\)"),
        (dict(cell_areas=np.ones(5)), V, "cell_areas does not match the spatial shape"),
        (dict(cell_areas=np.array([1.0, NAN, 1.0, 1.0])), V, "cell_areas must be finite and non-negative"),
        (dict(cell_areas=np.zeros((4, 5))), V, "cell_areas must have a positive, finite sum"),
    ]
    cases += [(dict(min_share=m), Cf, "min_share must be a number in 0 .. 1") for m in (-0.1, 1.5, NAN, "half", True)]
    cases += [(dict(block_steps=s), Cf, "block_steps must be a positive number of timesteps, 'auto' or None") for s in (0, 2.5, "all")]
    for kw, cls, msg in cases:
        args = dict(ID_field_a=x, ID_field_b=x)
        args.update(kw)
        with pytest.raises(cls, match=msg):
            marex_amd.event_matching(**args)
    with pytest.raises(TypeError):
        marex_amd.event_matching(x)  # the second field is required


def decode(key, widths):
    ba, bb, bs = widths
    k = int(key)
    return k & ((1 << bs) - 1), k >> (bb + bs), (k >> bs) & ((1 << bb) - 1)


def test_event_matching_is_public_and_the_key_round_trips_at_its_corners():
    assert "event_matching" in marex_amd.__all__ and marex_amd.event_matching is mm.event_matching
    assert hasattr(marex_amd.tracker, "event_matching") and hasattr(HotPath, "event_matching")
    from marex_amd import _lib
    from marex_amd.csrc import build

    for name in ("marex_event_matching_count_i32", "marex_event_matching_i32", "marex_event_matching_layout"):
        assert name in _lib.PROTOTYPES
    assert "marex_event_matching" in build.UNITS and "event_matching" in marex_amd.__doc__
    build.build(verbose=False)  # hipcc cross-compiles without a GPU
    L = HotPath.matching_layout()
    assert L["piece"] == 64 and L["wave"] % 64 == 0 and L["wg"] == 4 * L["wave"] and L["row_stride"] >= 1
    assert L["id_bits"] == 31 and L["min_step_bits"] == 64 - 2 * L["id_bits"] == 2
    assert HotPath.matching_entry_bytes(False) == 16 and HotPath.matching_entry_bytes(True) == 24
    W, K = HotPath.matching_widths, HotPath.matching_key
    I31 = mc.I31
    # the smallest key
    assert W(1, 1, 1) == (1, 1, 1) and W(0, 0, 1) == (1, 1, 1) and int(K(0, 1, 1, (1, 1, 1))) == 0b110
    assert int(K(0, 0, 1, (1, 1, 1))) == 0b010 and int(K(1, 1, 0, (1, 1, 1))) == 0b101
    # two 31-bit IDs leave 2 step bits: a window of 9 steps is split into pieces of 4
    w = W(I31, I31, 9)
    assert w == (31, 31, 2) and int(K(3, I31, I31, w)) == 2**64 - 1 and int(K(0, 1, 0, w)) == 1 << 33
    # the largest widths that fit one window without a split, and one more step, which forces it
    w = W(I31, 2**16 - 1, 2**17)
    assert w == (31, 16, 17) and sum(w) == 64 and 2**17 <= 1 << w[2]
    w1 = W(I31, 2**16 - 1, 2**17 + 1)
    assert w1 == (31, 16, 17) and 2**17 + 1 > 1 << w1[2]
    assert W(2**17 - 1, 2**17 - 1, 1826) == (17, 17, 11)  # the IDs of a real tracking: nothing is split
    assert W(I31, 2**30 - 1, 8) == (31, 30, 3) and W(I31, 2**30 - 1, 9) == (31, 30, 3) and W(I31, 2**30, 9) == (31, 31, 2)
    rng = np.random.default_rng(0)
    for ma, mb, Tb in ((1, 1, 1), (I31, I31, 9), (I31, 2**16 - 1, 2**17), (5, I31, 1000), (2**17 - 1, 2**17 - 1, 1826), (0, 7, 3)):
        w = W(ma, mb, Tb)
        assert min(w) >= 1 and sum(w) <= 64 and (w[2] >= 2 or Tb <= 2)
        steps = min(Tb, 1 << w[2])
        for s, a, b in [(0, ma, mb), (steps - 1, ma, mb), (steps - 1, 0, mb), (0, ma, 0), (steps - 1, max(ma, 1), 0)] + \
                [(int(rng.integers(0, steps)), int(rng.integers(0, ma + 1)), int(rng.integers(0, mb + 1))) for _ in range(20)]:
            k = K(s, a, b, w)
            assert k.dtype == np.uint64 and decode(k, w) == (s, a, b)
            assert (a == 0 and b == 0) or int(k) >> w[2] != 0  # no present pair gives the key 0
    ks = K([0, 1, 0, 1, 0], [1, 1, 2, 2, 2], [3, 0, 0, 0, 1], (2, 2, 1))
    assert np.argsort(ks).tolist() == [1, 0, 2, 3, 4]  # as integers the keys sort by (a, b, step)
    for bad in ((-1, 1, 1), (2**31, 1, 1), (1, 2**31, 1), (1, 1, 0)):
        with pytest.raises(ProcessingError, match="matching_widths"):
            W(*bad)


@pytest.fixture
def host_engine(monkeypatch):
    import marex_amd.detect as det

    eng = HostEngine()
    monkeypatch.setattr(det, "get_engine", lambda device=0: eng)
    monkeypatch.setattr(mi, "_free_bytes", lambda e: 1 << 30)
    return eng


TIMES = np.array(["2001-12-30", "2001-12-31", "2002-01-01", "2002-02-28", "2002-03-01", "2002-06-01", "2002-12-01"],
                 dtype="datetime64[D]").astype("datetime64[ns]")


@pytest.mark.parametrize("areas", [False, True])
def test_grid_against_the_oracle_with_windows(host_engine, areas):
    rng = np.random.default_rng(1)
    T, ny, nx = TIMES.size, 5, 8
    C = ny * nx
    a, b = mc.blob_pair(rng, T, C, n_ids=6, width=9)
    a[a == 3] = 0  # an ID that no cell holds
    b[2] = 0  # a step without an event of B
    area_y = np.array([1.0, 2.5, 4.0, 2.5, 1.0])
    dims = ("time", "lat", "lon")
    coords = {"time": ("time", TIMES), "lat": ("lat", np.linspace(-30, 30, ny)), "lon": ("lon", np.linspace(0, 70, nx))}
    fa = DataArray(a.reshape(T, ny, nx), dims=dims, coords=coords)
    fb = b.reshape(T, ny, nx)  # a bare array beside a DataArray
    kw, okw = {}, dict(tv=TIMES)
    if areas:
        kw["cell_areas"], okw["cell_areas"] = area_y, np.repeat(area_y, nx)
    for per in (False, True):
        whole = marex_amd.event_matching(fa, fb, per_timestep=per, **kw)
        mc.assert_dataset(whole, mo.matching(a, b, per_timestep=per, **okw))
        assert host_engine.calls[-1] == ("event_matching", 0, T, areas)
        for s in (1, 2, T, "auto"):  # window plans: the same bytes
            host_engine.calls.clear()
            mc.same_bytes(whole, marex_amd.event_matching(fa, fb, per_timestep=per, block_steps=s, **kw))
            if s == 2:
                assert [c[1:3] for c in host_engine.calls] == [(t, min(2, T - t)) for t in range(0, T, 2)]
    v = {k: np.asarray(whole[k].values) for k in whole.data_vars}
    key = v["pair_ID_a"] * 1000 + v["pair_ID_b"]
    assert key.size > 2 and (np.diff(key) > 0).all() and np.array_equal(np.diff(v["pair_record_offsets"]), v["pair_steps"])
    assert v["a_steps"][2] == 0 and np.isnan(v["a_matched_share"][2]) and v["a_best_match"][2] == 0
    assert v["step_cells_both"][2] == 0 and v["step_cells_only_b"][2] == 0
    assert v["pair_time_start"].dtype == TIMES.dtype and np.array_equal(np.asarray(whole["step_cells_both"].coords["time"].values), TIMES)
    assert v["cell_steps_both"] == v["pair_cell_steps"].sum() == v["step_cells_both"].sum()
    # another integer type, the [y, x] areas written out: the same bytes
    kw2 = dict(kw, cell_areas=np.repeat(area_y[:, None], nx, axis=1)) if areas else kw
    mc.same_bytes(whole, marex_amd.event_matching(DataArray(a.reshape(T, ny, nx).astype(np.int64), dims=dims, coords=coords),
                                                 fb.astype(np.int16), per_timestep=True, **kw2))


def test_mesh_with_areas_orders_of_magnitude_apart(host_engine):
    rng = np.random.default_rng(5)
    T, C = 9, 61
    a, b = mc.blob_pair(rng, T, C, n_ids=7, width=8)
    areas = rng.integers(1, 2**10, C) * 2.0 ** rng.integers(-20, 30, C)
    fa, fb = DataArray(a, dims=("time", "ncells")), DataArray(b, dims=("time", "ncells"))
    ds = marex_amd.event_matching(fa, fb, cell_areas=areas, per_timestep=True, block_steps=4)
    mc.assert_dataset(ds, mo.matching(a, b, areas, per_timestep=True))
    assert [c[1:3] for c in host_engine.calls[-3:]] == [(0, 4), (4, 4), (8, 1)]
    assert np.asarray(ds["pair_ID_a"].values).size > 3 and 0 < float(ds["pod"].values) <= 1
    for name, bad_a, bad_b in (("ID_field_a", np.where(a == 3, -1, a), b), ("ID_field_b", a, np.where(b == 2, -7, b))):
        with pytest.raises(DataValidationError, match="Object IDs must be non-negative") as err:
            marex_amd.event_matching(bad_a, bad_b, block_steps=2)
        assert name in str(err.value) + str(getattr(err.value, "details", ""))
    with pytest.raises(marex_amd.TrackingError, match=r"event_matching: needs .* GB of device memory, .* GB are free"):
        marex_amd.event_matching(np.ones((64, 1 << 25), np.int32), np.ones((64, 1 << 25), np.int32))


SWAP = {"pair_ID_a": "pair_ID_b", "pair_share_of_a": "pair_share_of_b", "n_a": "n_b", "matched_a": "matched_b",
        "cell_steps_only_a": "cell_steps_only_b", "area_steps_only_a": "area_steps_only_b", "step_cells_only_a": "step_cells_only_b"}


def test_swapping_the_fields_transposes_the_result(host_engine):
    rng = np.random.default_rng(6)
    T, C = 8, 90
    a, b = mc.blob_pair(rng, T, C, n_ids=8, width=11)
    areas = rng.integers(1, 50, C).astype(np.float64)
    ab = {k: np.asarray(v.values) for k, v in marex_amd.event_matching(a, b, cell_areas=areas).data_vars.items()}
    ba = {k: np.asarray(v.values) for k, v in marex_amd.event_matching(b, a, cell_areas=areas).data_vars.items()}
    order = np.lexsort((ba["pair_ID_a"], ba["pair_ID_b"]))  # the pairs of (b, a) in the order of (a, b)
    assert order.size > 3 and not np.array_equal(order, np.arange(order.size))
    swap = dict(SWAP, **{v: k for k, v in SWAP.items()})
    for k, v in ab.items():
        other = swap.get(k, "b_" + k[2:] if k.startswith("a_") else "a_" + k[2:] if k.startswith("b_") else k)
        w = ba[other][order] if k.startswith("pair_") else ba[other]
        if k in ("pair_onset_lag", "pair_end_lag"):
            w = -w
        if k in ("pod", "far", "csi"):  # the scores are not symmetric: the hits are counted in the first field
            continue
        assert np.array_equal(v, w, equal_nan=v.dtype.kind == "f"), (k, other)
    assert float(ab["pod"]) == int(ba["matched_b"]) / int(ba["n_b"]) and float(ab["far"]) == 1 - int(ba["matched_a"]) / int(ba["n_a"])


def test_a_field_against_itself(host_engine):
    rng = np.random.default_rng(7)
    a = mc.blob_field(rng, 6, 80, n_ids=7, width=9)
    ds = marex_amd.event_matching(a, a.copy(), cell_areas=rng.uniform(0.5, 2.0, 80))
    v = {k: np.asarray(ds[k].values) for k in ds.data_vars}
    present = np.unique(a[a > 0])
    assert v["pair_ID_a"].tolist() == present.tolist() == v["pair_ID_b"].tolist()
    assert (v["pair_iou"] == 1).all() and (v["pair_share_of_a"] == 1).all() and (v["pair_onset_lag"] == 0).all() and (v["pair_end_lag"] == 0).all()
    assert float(v["pod"]) == 1 and float(v["csi"]) == 1 and float(v["far"]) == 0
    assert int(v["cell_steps_only_a"]) == 0 == int(v["cell_steps_only_b"]) and int(v["cell_steps_both"]) == int((a > 0).sum())
    assert np.array_equal(v["a_best_match"][present - 1], present) and (v["a_matched_share"][present - 1] == 1).all()


def test_min_share_at_a_threshold_placed_on_a_share(host_engine):
    a = np.zeros((2, 12), np.int32)
    b = np.zeros((2, 12), np.int32)
    a[0, 0:4], b[0, 3:5] = 1, 1      # event 1 of A: one of four cells covered, 0.25; event 1 of B: one of two, 0.5
    a[1, 6:9], b[1, 6:9] = 2, 2      # event 2 of both: covered whole
    a[1, 10] = 3                     # event 3 of A: not covered at all
    cases = [(0.0, 2, 2), (0.25, 2, 2), (float(np.nextafter(0.25, 1)), 1, 2), (0.5, 1, 2), (float(np.nextafter(0.5, 1)), 1, 1),
             (1.0, 1, 1)]
    for m, ma, mb in cases:
        ds = marex_amd.event_matching(a, b, min_share=m)
        mc.assert_dataset(ds, mo.matching(a, b, min_share=m))
        assert (int(ds["matched_a"].values), int(ds["matched_b"].values)) == (ma, mb), m
        assert float(ds["pod"].values) == ma / 3 and float(ds["far"].values) == 1 - mb / 2 and float(ds["csi"].values) == ma / (3 + 2 - mb)
    assert np.asarray(ds["a_matched_share"].values).tolist() == [0.25, 1.0, 0.0]  # an uncovered event is never matched


def test_the_empty_cases_need_no_device(monkeypatch):
    _no_gpu(monkeypatch)
    for x in (np.zeros((0, 5), np.int32), np.zeros((4, 0), np.int32), np.zeros((0, 2, 3), np.int32), np.zeros((3, 5), np.int32),
              np.zeros((3, 2, 4), np.int64)):
        C = int(np.prod(x.shape[1:]))
        for areas in (None, np.ones(x.shape[1:]) if C else None):
            ds = marex_amd.event_matching(x, x.copy(), cell_areas=areas, per_timestep=True)
            mc.assert_dataset(ds, mo.matching(x.reshape(x.shape[0], C), x.reshape(x.shape[0], C), None if areas is None else np.ones(C),
                                              per_timestep=True))
            assert np.asarray(ds["pair_ID_a"].values).size == 0 and np.asarray(ds["a_steps"].values).size == 0
            assert int(ds["n_a"].values) == 0 and np.isnan(float(ds["pod"].values)) and np.isnan(float(ds["csi"].values))
            assert np.asarray(ds["step_cells_both"].values).shape == (x.shape[0],)


def test_n_events_pad_and_refuse(host_engine):
    a = np.array([[1, 0, 2, 0]], np.int32)
    b = np.array([[1, 1, 0, 0]], np.int32)
    with pytest.raises(ProcessingError, match=r"event_matching \(ID_field_a\): the ID field holds event 2, the events Dataset ends at 1"):
        mm._event_matching(a, b, None, 0.0, False, None, None, n_events_a=1)
    ds = mm._event_matching(a, b, None, 0.0, False, None, None, n_events_a=4, n_events_b=3, time=("step", "date", np.array([7])))
    mc.assert_dataset(ds, mo.matching(a, b, n_a=4, n_b=3, tv=np.array([7])), tname="step")
    assert np.asarray(ds["a_steps"].values).tolist() == [1, 1, 0, 0] and int(ds["n_a"].values) == 2
