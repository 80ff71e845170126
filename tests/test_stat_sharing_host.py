"""What the event-slot and region statistics share (``marex_amd._stream``, ``HotPath._area_q_check``): the spatial parser, the
slot index, the padding to the events Dataset, the guarded mean and the exact-sum test of the fixed-point areas -- and that
every front end that takes ``cell_areas`` hands the engine the bits it handed it before the parser was shared.  No GPU needed.

``tests/golden/stat_sharing_areas.npz`` holds those bits: what reached the host engines when every front end still parsed
``cell_areas`` itself, written by tests/record_stat_sharing_areas.py on that code.  Nothing here writes it."""
import inspect
import os
import re
import sys

import numpy as np
import pytest
import torch

import marex_amd
from marex_amd.exceptions import DataValidationError, ProcessingError
from marex_amd.xr_compat import DataArray

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import event_categories_host_engine  # noqa: E402
import event_exposure_host_engine  # noqa: E402
import event_shapes_host_engine  # noqa: E402
import intensity_host_engine  # noqa: E402
import regional_series_host_engine  # noqa: E402

GOLDEN = os.path.join(HERE, "golden", "stat_sharing_areas.npz")
GRIDS = {"4x5": (4, 5), "1x1": (1, 1), "1x7": (1, 7), "mesh7": (7,)}
T = 3


def _case(grid):
    """``(ids, anom, areas)`` of a grid: three events over three steps, and areas that are constant along x (so that the
    ``[ny]`` row vector says the same as the other forms) with all 53 bits of their mantissas in use."""
    sp = GRIDS[grid]
    rng = np.random.default_rng(sorted(GRIDS).index(grid) + 11)
    ids = rng.integers(0, 4, (T,) + sp).astype(np.int32)
    ids.reshape(T, -1)[:, 0] = (1, 1, 3)
    anom = rng.normal(1.0, 2.0, (T,) + sp).astype(np.float32)
    rows = rng.uniform(0.5, 2.0, sp[0]) * 12345.678
    return ids, anom, (np.ascontiguousarray(np.broadcast_to(rows[:, None], sp)) if len(sp) == 2 else rows)


def _forms(grid, areas):
    sp = GRIDS[grid]
    forms = {"flat": areas.reshape(-1), "spatial": areas}
    if len(sp) == 2:
        forms["transposed"] = DataArray(np.ascontiguousarray(areas.T), dims=("lon", "lat"))
        forms["row"] = areas[:, 0].copy()
    return forms


def _labelled(a):
    dims = ("time", "lat", "lon") if a.ndim == 3 else ("time", "cell")
    return DataArray(a, dims=dims, coords={"time": ("time", np.arange(a.shape[0]))})


def _spy(cls, method, names):
    """An instance of the host engine ``cls`` whose ``method`` notes its arguments ``names`` in ``seen`` before it runs."""
    inner = getattr(cls, method)
    sig = inspect.signature(inner)

    def noting(self, *args, **kw):
        given = sig.bind(self, *args, **kw).arguments
        for n in names:
            v = given.get(n)
            self.seen[n] = None if v is None else np.array(v.numpy() if isinstance(v, torch.Tensor) else v)
        return inner(self, *args, **kw)

    eng = type("Spy", (cls,), {method: noting})()
    eng.seen = {}
    return eng


FRONT_ENDS = ("event_intensity", "event_categories", "event_shapes", "regional_series", "event_exposure")


def _reaches_engine(front, grid, areas_form):
    """``{name: bits}`` of what the engine is handed for the areas, and of the one result that shows ``e``."""
    import marex_amd._stream as ms
    import marex_amd.detect as det

    ids, anom, _ = _case(grid)
    fi, fa = _labelled(ids), _labelled(anom)
    sp = GRIDS[grid]
    with pytest.MonkeyPatch.context() as mp:
        mp.setattr(ms, "_free_bytes", lambda e: 1 << 30)

        def run(cls, method, names, call):
            eng = _spy(cls, method, names)
            mp.setattr(det, "get_engine", lambda device=0: eng)
            return eng.seen, call()

        if front == "event_intensity":
            seen, _ = run(intensity_host_engine.HostEngine, front, ("weights",), lambda: marex_amd.event_intensity(fi, fa, areas_form))
            return {"weights": seen["weights"]}
        if front == "event_categories":
            seen, _ = run(event_categories_host_engine.HostEngine, front, ("weights",),
                          lambda: marex_amd.event_categories(fi, fa, np.ones(sp, np.float32), areas_form))
            return {"weights": seen["weights"]}
        if front == "event_shapes":
            seen, ds = run(event_shapes_host_engine.HostEngine, front, ("area_q",), lambda: marex_amd.event_shapes(fi, cell_areas=areas_form))
            return {"q": seen["area_q"], "shows_e": np.asarray(ds["area"].values)}
        if front == "regional_series":
            seen, ds = run(regional_series_host_engine.HostEngine, front, ("q", "wf"),
                           lambda: marex_amd.regional_series(fi, None, areas_form, fa))
        else:
            seen, ds = run(event_exposure_host_engine.HostEngine, front, ("q", "wf"),
                           lambda: marex_amd.event_exposure(fi, np.zeros(sp, np.int32), areas_form, fa))
        return {"q": seen["q"], "wf": seen["wf"], "shows_e": np.asarray(ds["region_area"].values)}


def _pairs():
    return [(f, g) for f in FRONT_ENDS for g in GRIDS if not (f == "event_shapes" and g == "mesh7")]


@pytest.mark.parametrize("front,grid", _pairs())
def test_the_engine_gets_the_bits_it_got_before(front, grid):
    golden = np.load(GOLDEN)
    want = {k.split("/")[2]: golden[k] for k in golden.files if k.startswith(f"{front}/{grid}/")}
    assert want and want[next(iter(want))].size
    dtypes = {"weights": np.float32, "wf": np.float32, "q": np.int64, "shows_e": np.float64}
    for form, a in _forms(grid, _case(grid)[2]).items():
        got = _reaches_engine(front, grid, a)
        assert sorted(got) == sorted(want), form
        for k, v in got.items():
            assert v.dtype == dtypes[k] == want[k].dtype and v.shape == want[k].shape, (form, k)
            assert v.tobytes() == want[k].tobytes(), (form, k)


# ------------------------------------------------------------------ the spatial parser
def _plan(grid, labelled=True):
    from marex_amd._stream import plan_field

    ids = _case(grid)[0]
    return plan_field(_labelled(ids) if labelled else ids, "test")


@pytest.mark.parametrize("grid", sorted(GRIDS))
def test_every_accepted_form_gives_the_same_flat_vector(grid):
    from marex_amd._stream import spatial

    areas = _case(grid)[2]
    p = _plan(grid)
    for form, a in _forms(grid, areas).items():
        v = spatial(a, p, "cell_areas", row_vector=True)
        assert v.dtype == np.float64 and v.flags.c_contiguous and v.tobytes() == areas.reshape(-1).tobytes(), form
    if len(GRIDS[grid]) == 2 and GRIDS[grid][0] > 1:  # a row vector is taken only where the caller allows it
        with pytest.raises(DataValidationError, match="cell_areas does not match the spatial shape of the field"):
            spatial(areas[:, 0].copy(), p, "cell_areas")
    # the names decide: the same transposed array without them, or under a field without them, is no spatial shape
    if len(GRIDS[grid]) == 2 and GRIDS[grid][0] != GRIDS[grid][1]:
        with pytest.raises(DataValidationError, match="cell_areas does not match"):
            spatial(np.ascontiguousarray(areas.T), p, "cell_areas", row_vector=True)
        with pytest.raises(DataValidationError, match="cell_areas does not match"):
            spatial(_forms(grid, areas)["transposed"], _plan(grid, labelled=False), "cell_areas", row_vector=True)


WORDINGS = (None, "cell_areas do not match the spatial shape of ID_field")
PINNED = ("cell_areas does not match the spatial shape of the field", "cell_areas do not match the spatial shape of ID_field")


@pytest.mark.parametrize("grid", sorted(GRIDS))
def test_rejected_forms_are_refused_in_both_wordings(grid):
    from marex_amd._stream import spatial

    sp = GRIDS[grid]
    C = int(np.prod(sp))
    bad = {"wrong length": np.ones(C + 2), "3-D": np.ones((2,) + sp) if len(sp) == 2 else np.ones((1, 1, C))}
    if len(sp) == 2 and sp[1] not in (sp[0], C):  # on a square grid [nx] is the row vector, on one row the flat form
        bad["[nx]"] = np.ones(sp[1])
    assert grid != "4x5" or sorted(bad) == ["3-D", "[nx]", "wrong length"]
    p = _plan(grid)
    for what, a in bad.items():
        for wording, text in zip(WORDINGS, PINNED):
            with pytest.raises(DataValidationError) as ei:
                spatial(a, p, "cell_areas", row_vector=True, mismatch=wording)
            assert ei.value.message == text and ei.value.details == f"cell_areas {a.shape}, a timestep {sp}", (what, wording)


def test_the_front_ends_keep_their_wordings():
    ids, anom, _ = _case("4x5")
    for a in (np.ones(5), np.ones(21), np.ones((2, 4, 5))):
        for call in (lambda: marex_amd.event_intensity(ids, anom, a), lambda: marex_amd.event_shapes(ids, cell_areas=a),
                     lambda: marex_amd.event_categories(ids, anom, np.ones((4, 5), np.float32), a)):
            with pytest.raises(DataValidationError, match="cell_areas do not match the spatial shape of ID_field"):
                call()
        for call in (lambda: marex_amd.regional_series(ids, None, a), lambda: marex_amd.event_exposure(ids, np.zeros((4, 5), np.int32), a)):
            with pytest.raises(DataValidationError, match="cell_areas does not match the spatial shape of the field"):
                call()
    for call in (lambda a: marex_amd.event_intensity(ids, anom, a), lambda a: marex_amd.event_shapes(ids, cell_areas=a),
                 lambda a: marex_amd.regional_series(ids, None, a), lambda a: marex_amd.event_exposure(ids, np.zeros((4, 5), np.int32), a)):
        with pytest.raises(DataValidationError, match="cell_areas must be numbers"):
            call(np.full((4, 5), "1.0"))
        with pytest.raises(DataValidationError, match="cell_areas must be finite and non-negative"):
            call(np.full((4, 5), -1.0))
    with pytest.raises(DataValidationError, match="mask does not match the spatial shape of ID_field"):
        marex_amd.event_shapes(ids, mask=np.ones((5, 4), bool))


# ------------------------------------------------------------------ slots
def _slots_by_loops(tmin, tmax):
    """``(off, e_of, t_of)`` by a plain double loop over the events 1..N and their steps."""
    off, e_of, t_of = [0, 0], [], []
    for e in range(1, len(tmin)):
        for t in range(int(tmin[e]), int(tmax[e]) + 1):
            e_of.append(e)
            t_of.append(t)
        off.append(len(e_of))
    return np.array(off, np.int64), np.array(e_of, np.int64), np.array(t_of, np.int64)


I32_MAX = 2**31 - 1
SPANS = {"no event": ([I32_MAX], [-1]),
         "one event of one step": ([I32_MAX, 4], [-1, 4]),
         "an event without a slot between two with": ([I32_MAX, 2, I32_MAX, 0], [-1, 4, -1, 1])}


@pytest.mark.parametrize("case", sorted(SPANS))
def test_slot_index_against_a_double_loop(case):
    from marex_amd._stream import slot_index
    from marex_amd.engine import HotPath

    tmin, tmax = (np.array(v, np.int64) for v in SPANS[case])
    N = tmin.size - 1
    off, e_want, t_want = _slots_by_loops(tmin, tmax)
    assert HotPath.event_slot_plan(tmin, tmax).tolist() == off.tolist()
    e_of, t_of = slot_index(off, tmin, N)
    assert e_of.tolist() == e_want.tolist() and t_of.tolist() == t_want.tolist()
    assert e_of.shape == t_of.shape == (int(off[-1]),)


@pytest.mark.parametrize("case", sorted(SPANS))
@pytest.mark.parametrize("more", [0, 1, 3])
def test_pad_events_adds_events_without_a_slot(case, more):
    from marex_amd._stream import pad_events, slot_index

    tmin, tmax = (np.array(v, np.int64) for v in SPANS[case])
    N = tmin.size - 1
    off = _slots_by_loops(tmin, tmax)[0]
    N2, tmin2, off2 = pad_events("event_intensity", N, N + more, tmin, off)
    want = _slots_by_loops(np.concatenate([tmin, np.full(more, I32_MAX)]), np.concatenate([tmax, np.full(more, -1)]))
    assert N2 == N + more and tmin2.tolist() == tmin.tolist() + [I32_MAX] * more and off2.tolist() == want[0].tolist()
    assert tmin2.dtype == off2.dtype == np.int64
    e_of, t_of = slot_index(off2, tmin2, N2)
    assert e_of.tolist() == want[1].tolist() and t_of.tolist() == want[2].tolist()
    assert pad_events("event_intensity", N, None, tmin, off) == (N, tmin, off)  # no events Dataset: as found


def test_pad_events_refuses_a_field_beyond_the_dataset():
    from marex_amd._stream import pad_events

    tmin, tmax = (np.array(v, np.int64) for v in SPANS["an event without a slot between two with"])
    off = _slots_by_loops(tmin, tmax)[0]
    for what in ("event_intensity", "event_categories", "event_shapes", "event_exposure"):
        with pytest.raises(ProcessingError) as ei:
            pad_events(what, 3, 2, tmin, off)
        assert ei.value.message == f"{what}: the ID field holds event 3, the events Dataset ends at 2"
    with pytest.raises(ProcessingError, match="event_exposure: the ID field holds event 3, the events Dataset ends at 2"):
        pad_events("event_exposure", 3, 2)
    assert pad_events("event_exposure", 3, 5) == (5, None, None) and pad_events("event_exposure", 3, None) == (3, None, None)


# ------------------------------------------------------------------ the guarded mean
def test_weighted_mean_is_the_expression_it_replaces():
    from marex_amd._stream import weighted_mean

    some = np.array([True, False, True, True, False, True])
    W = np.array([0.0, 2.0, 3.0, 0.1, 0.0, -0.0])  # cells with W = 0, no cell with W > 0, ordinary ones, -0.0 is 0 too
    SA = np.array([5.0, 4.0, 1.0, -0.7, np.nan, 1.0])
    with np.errstate(invalid="ignore", divide="ignore"):
        want = np.where(some & (W != 0), SA / np.where(W != 0, W, 1.0), np.nan)
    got = weighted_mean(some, W, SA)
    assert got.dtype == np.float64 and got.tobytes() == want.tobytes()
    assert np.isnan(got[0]) and np.isnan(got[1]) and got[2] == 1.0 / 3.0 and got[3] == -0.7 / 0.1 and np.isnan(got[5])
    got2 = weighted_mean(some.reshape(2, 3), W.reshape(2, 3), SA.reshape(2, 3))
    assert got2.shape == (2, 3) and got2.tobytes() == want.tobytes()


# ------------------------------------------------------------------ the exact sum of the fixed-point areas
def test_area_q_check_sums_exactly():
    from marex_amd.engine import HotPath

    wraps = np.full(8, 2**61, np.int64)  # 2^64: an int64 sum wraps to 0
    with np.errstate(over="ignore"):
        assert int(wraps.sum()) == 0
    refusal = "q must be 8 non-negative int64 areas whose sum stays below 2^62"
    for what in ("regional_series", "event_exposure"):
        with pytest.raises(ProcessingError) as ei:
            HotPath._area_q_check(what, wraps, 8)
        assert ei.value.message == f"{what}: {refusal}"
    at = np.array([2**61, 2**61 - 1, 0, 0, 0, 0, 0, 0], np.int64)  # 2^62 - 1
    HotPath._area_q_check("regional_series", at, 8)
    for q in (at + np.eye(8, dtype=np.int64)[7], np.where(np.arange(8) == 3, -1, 1).astype(np.int64), np.full(8, 2**62, np.int64),
              at.astype(np.int32), at[:7]):
        with pytest.raises(ProcessingError, match="regional_series: q must be 8 non-negative int64 areas"):
            HotPath._area_q_check("regional_series", q, 8)
    # through the engine call of the host: refused before anything is allocated
    eng = HotPath.__new__(HotPath)
    eng.device = torch.device("cpu")
    x = torch.zeros((1, 8), dtype=torch.uint8)
    with pytest.raises(ProcessingError, match=re.escape("regional_series: " + refusal)):
        eng.regional_series(x, np.zeros(8, np.int32), 1, 1, q=wraps)
    with pytest.raises(ProcessingError, match=re.escape("event_exposure: " + refusal)):
        eng.event_exposure(x.to(torch.int32), np.zeros(8, np.int32), 1, q=wraps)
