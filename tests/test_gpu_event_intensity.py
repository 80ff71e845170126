"""GPU parity: per-event intensity (``marex_event_intensity_f32`` through ``HotPath.event_intensity``,
``marex_amd.event_intensity`` and ``tracker.event_intensity``) against the NumPy oracle of tests/intensity_oracle.py --
bit for bit where every float64 partial sum is exact, within the derived bound of the sums otherwise; time blocks, the
span guard, the return codes, and the trackers end to end on a grid (merging and not) and on a mesh."""
import os
import sys

import numpy as np
import pytest
import torch

import marex_amd
from marex_amd.engine import HotPath
from marex_amd.exceptions import ProcessingError
from marex_amd.xr_compat import DataArray

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import intensity_oracle as io  # noqa: E402
from intensity_cases import N_EV, SHAPES, blob_anomalies, blobs, exact_field, public_field, spans, weights  # noqa: E402
from test_event_intensity_host import DTYPES, VARS_E, VARS_T, assert_equals_oracle  # noqa: E402

pytestmark = pytest.mark.gpu

U = 2.0 ** -53


def _dev(hot, a):
    return torch.from_numpy(np.array(a, order="C")).to(hot.device)  # np.array copies: the input stays as it is


_exp = {}


def _compact(ids, anom, w, tmin, off, tag="exact"):
    """The oracle's slots laid out as the device lays them out: ``cnt``, ``sums``, ``vmax`` and the sums of |w a|."""
    key = (ids.shape, w is not None, tag)
    if key not in _exp:
        n = int(off[-1])
        cnt, sums, vmax, ab = np.zeros((n, 2), np.int64), np.zeros((n, 2)), np.full(n, np.nan, np.float32), np.zeros(n)
        for (t, e), (nf, nb, W, S, A, mx) in io.slots(ids, anom, w, N_EV).items():
            s = int(off[e] + t - tmin[e])
            assert off[e] <= s < off[e + 1]
            cnt[s], sums[s], ab[s] = (nf, nb), (W, S), A
            if mx is not None:
                vmax[s] = mx
        _exp[key] = (cnt, sums, vmax, ab)
    return _exp[key]


@pytest.mark.parametrize("weighted", [False, True], ids=["cells", "weights"])
@pytest.mark.parametrize("shape", SHAPES, ids=["6x335", "6x693", "5x4200"])
def test_kernel_equals_oracle_bit_for_bit(hot, shape, weighted):
    T, C = shape
    ids, anom = exact_field(T, C)
    tmin, tmax = spans(ids)
    assert HotPath.POISON                                                      # fresh buffers are 0xCD bytes: the zeroing shows
    assert (ids < 0).any() and (ids > N_EV).any() and (tmax >= 0)[1:].all()
    assert tmin[2] == 0 and tmax[2] == T - 1 and not (ids[2] == 2).any()       # event 2 is absent inside its span
    assert (ids == 5).sum() == 1                                               # a single cell
    assert (ids[4] == 6).any() and not np.isfinite(anom[4][ids[4] == 6]).any()  # a slot with non-finite cells only
    a14 = anom[1][ids[1] == 4]
    assert np.isfinite(a14).any() and (a14[np.isfinite(a14)] < 0).all()         # a slot with negative anomalies only
    inside = anom[(ids > 0) & (ids <= N_EV)]
    assert np.isnan(inside).any() and (inside == np.inf).any() and (inside == -np.inf).any()
    w = weights(C) if weighted else None
    wd = None if w is None else _dev(hot, w)
    outs = []
    for _ in range(2):  # a second call on the same input: the same bytes
        d, a = _dev(hot, ids), _dev(hot, anom)
        r = hot.event_intensity(d, a, tmin, tmax, wd)
        off = r["off"]
        assert off.tolist() == HotPath.event_slot_plan(tmin, tmax, T).tolist()
        cnt, sums, vmax, _ = _compact(ids, anom, w, tmin, off)
        assert r["cnt"].dtype == np.int64 and np.array_equal(r["cnt"], cnt), np.argwhere(r["cnt"] != cnt)[:8]
        assert r["sums"].dtype == np.float64 and np.array_equal(r["sums"], sums), np.argwhere(r["sums"] != sums)[:8]
        assert r["vmax"].dtype == np.float32 and np.array_equal(r["vmax"], vmax, equal_nan=True)
        assert np.array_equal(d.cpu().numpy(), ids) and a.cpu().numpy().tobytes() == anom.tobytes()  # inputs are read only
        outs.append((r["cnt"].tobytes(), r["sums"].tobytes(), r["vmax"].tobytes()))
    assert outs[0] == outs[1]
    s2, s6, s4 = int(off[2] + 2 - tmin[2]), int(off[6] + 4 - tmin[6]), int(off[4] + 1 - tmin[4])
    assert not r["cnt"][s2].any() and not r["sums"][s2].any() and np.isnan(r["vmax"][s2])
    assert r["cnt"][s6, 0] == 0 and r["cnt"][s6, 1] > 0 and not r["sums"][s6].any() and np.isnan(r["vmax"][s6])
    assert r["vmax"][s4] < 0 and r["cnt"][:, 0].sum() == np.isfinite(inside).sum() and r["cnt"][:, 1].sum() == (~np.isfinite(inside)).sum()
    if not weighted:
        assert np.array_equal(r["sums"][:, 0], r["cnt"][:, 0].astype(np.float64))
    if shape == SHAPES[1]:  # the same slots as the rename pass plans for these spans
        lut = np.arange(N_EV + 1, dtype=np.int32)
        clean = np.where((ids > 0) & (ids <= N_EV), ids, 0).astype(np.int32)
        assert hot.event_rename(_dev(hot, clean), 21, 33, lut, tmin, tmax)["off"].tolist() == off.tolist()


def test_time_blocks_host_and_device_inputs_give_the_same_bytes(hot):
    T, C = SHAPES[1]
    ids, anom = public_field(T, C)
    w = weights(C)
    exp = io.intensity(ids, anom, w, N_EV)
    whole = marex_amd.event_intensity(ids, anom, w)
    assert_equals_oracle(whole, exp, np.arange(T))
    for b in (1, 4, 6, "auto"):
        for dev in (False, True):
            i, a = (_dev(hot, ids), _dev(hot, anom)) if dev else (ids, anom)
            ds = marex_amd.event_intensity(i, a, w, block_steps=b)
            for k in VARS_T + VARS_E:
                assert np.asarray(ds[k].values).tobytes() == np.asarray(whole[k].values).tobytes(), (b, dev, k)
    # other types are converted on the way: float64 anomalies, int64 IDs; (time, y, x) with areas along y
    wy = (np.arange(21) + 1).astype(np.float32)
    exp = io.intensity(ids, anom, np.repeat(wy, 33), N_EV)
    ds = marex_amd.event_intensity(_dev(hot, ids.astype(np.int64).reshape(T, 21, 33)), anom.astype(np.float64).reshape(T, 21, 33), wy,
                                   block_steps=4)
    assert_equals_oracle(ds, exp, np.arange(T))
    none = marex_amd.event_intensity(np.zeros((T, C), np.int32), anom)
    assert none["ID"].values.size == 0 and np.asarray(none["intensity_cells"].values).shape == (T, 0)


def test_inexact_inputs_stay_within_the_bound_of_the_sums(hot):
    """Sums: |got - fsum| <= 2 n u sum|w a| (n finite cells of the slot, u = 2^-53), the order-independent bound of
    recursive summation of exact terms; the float32 mean of got and of the oracle within one float32 ulp."""
    T, C = SHAPES[1]
    ids, _ = exact_field(T, C)
    rng = np.random.default_rng(3)
    anom = rng.standard_normal((T, C)).astype(np.float32)
    w = rng.random(C).astype(np.float32)
    tmin, tmax = spans(ids)
    r = hot.event_intensity(_dev(hot, ids), _dev(hot, anom), tmin, tmax, _dev(hot, w))
    cnt, sums, vmax, ab = _compact(ids, anom, w, tmin, r["off"], tag="normal")
    assert np.array_equal(r["cnt"], cnt) and np.array_equal(r["vmax"], vmax, equal_nan=True)
    n = cnt[:, 0]
    err = np.abs(r["sums"] - sums)
    print("largest error of W and S over its bound:", float(np.max(err[:, 0] / np.maximum(2 * n * U * sums[:, 0], 1e-300))),
          float(np.max(err[:, 1] / np.maximum(2 * n * U * ab, 1e-300))))
    assert (err[:, 0] <= 2 * n * U * sums[:, 0]).all() and (err[:, 1] <= 2 * n * U * ab).all()
    live = n > 0
    got = (r["sums"][live, 1] / r["sums"][live, 0]).astype(np.float32)
    want = (sums[live, 1] / sums[live, 0]).astype(np.float32)
    assert (np.abs(got.astype(np.float64) - want.astype(np.float64)) <= np.spacing(np.abs(want)).astype(np.float64)).all()


def test_a_cell_outside_its_events_span_is_counted_not_accumulated(hot):
    """Event 1's span is declared one step short and event 2's slots follow it: a missing guard would add event 1's last
    step to event 2's first slot -- inside the allocation, so nothing can fault."""
    T, C = SHAPES[0]
    ids, anom = exact_field(T, C)
    tmin, tmax = spans(ids)
    assert tmax[1] == T - 1 and tmin[2] == 0
    good = hot.event_intensity(_dev(hot, ids), _dev(hot, anom), tmin, tmax)
    short = tmax.copy()
    short[1] -= 1
    lost = int((ids[T - 1] == 1).sum())
    with pytest.raises(ProcessingError, match=rf"event_intensity: {lost} cells belong to an event outside"):
        hot.event_intensity(_dev(hot, ids), _dev(hot, anom), tmin, short)
    # the same through the library, on buffers of the test's own: the other events' slots hold what they held before
    off = HotPath.event_slot_plan(tmin, short)
    n = int(off[-1])
    cnt = torch.zeros((n, 2), dtype=torch.int64, device=hot.device)
    sums = torch.zeros((n, 2), dtype=torch.float64, device=hot.device)
    vmax = torch.zeros(n, dtype=torch.int32, device=hot.device)
    status = torch.zeros(1, dtype=torch.int64, device=hot.device)
    hot.call("marex_event_intensity_f32", _dev(hot, ids), _dev(hot, anom), 0, T, C, N_EV, _dev(hot, tmin.astype(np.int32)),
             _dev(hot, off), n, None, cnt, sums, vmax, status)
    assert int(status.item()) == lost > 0
    g = int(good["off"][2])
    assert off[2] == g - 1
    assert np.array_equal(cnt.cpu().numpy()[off[2]:], good["cnt"][g:]) and np.array_equal(sums.cpu().numpy()[off[2]:], good["sums"][g:])
    assert np.array_equal(cnt.cpu().numpy()[:off[2]], good["cnt"][:off[2]])
    key = vmax.cpu().numpy().view(np.uint32)
    assert np.array_equal(marex_amd.intensity.key_float(key)[off[2]:], good["vmax"][g:], equal_nan=True)
    # a span that starts late: the earlier step is counted; a block that starts at t0 = 1 meets no such cell
    late = tmin.copy()
    late[1] += 1
    with pytest.raises(ProcessingError, match=rf"event_intensity: {int((ids[0] == 1).sum())} cells"):
        hot.event_intensity(_dev(hot, ids), _dev(hot, anom), late, tmax)
    hot.event_intensity(_dev(hot, ids[1:]), _dev(hot, anom[1:]), late, tmax, t0=1)


def test_engine_and_library_check_their_arguments_before_the_launch(hot):
    T, C = SHAPES[0]
    ids, anom = exact_field(T, C)
    tmin, tmax = spans(ids)
    d, a = _dev(hot, ids), _dev(hot, anom)
    first = hot.event_intensity(d, a, tmin, tmax, finish=False)
    for bad in (lambda: hot.event_intensity(d.to(torch.int64), a, tmin, tmax),
                lambda: hot.event_intensity(d, a.to(torch.float64), tmin, tmax),
                lambda: hot.event_intensity(d, a[:, :-1].contiguous(), tmin, tmax),
                lambda: hot.event_intensity(d, a.t().contiguous().t(), tmin, tmax),
                lambda: hot.event_intensity(d, a.cpu(), tmin, tmax),
                lambda: hot.event_intensity(d, a, tmin, tmax, torch.ones(C + 1, device=hot.device)),
                lambda: hot.event_intensity(d, a, tmin, tmax, torch.ones(C, dtype=torch.float64, device=hot.device)),
                lambda: hot.event_intensity(d, a, tmin[:1], tmax[:1]),
                lambda: hot.event_intensity(d, a, tmin, tmax[:-1]),
                lambda: hot.event_intensity(d, a, tmin, tmax, t0=-1),
                lambda: hot.event_intensity(d, a, tmin, tmax - 1, acc=first["acc"])):    # accumulators of another plan
        with pytest.raises(ProcessingError):
            bad()
    n = N_EV + 1
    tm_d, off_d = _dev(hot, np.zeros(n, np.int32)), _dev(hot, np.arange(N_EV + 2, dtype=np.int64))
    cnt = torch.zeros((n, 2), dtype=torch.int64, device=hot.device)
    sums = torch.zeros((n, 2), dtype=torch.float64, device=hot.device)
    vmax = torch.zeros(n, dtype=torch.int32, device=hot.device)
    st = torch.zeros(1, dtype=torch.int64, device=hot.device)
    ok = (d, a, 0, T, C, N_EV, tm_d, off_d, n, None, cnt, sums, vmax, st)

    def with_(**kw):
        names = ("ids", "anom", "t0", "Tb", "C", "n_ev", "ev_tmin", "ev_off", "n_slots", "w", "cnt", "sums", "vmax", "status")
        return tuple(kw.get(k, v) for k, v in zip(names, ok))

    cases = [(-4, with_(C=2**31 - 1)), (-4, with_(C=2**40)), (-4, with_(Tb=2**31 - 1)), (-4, with_(t0=2**31 - 1 - T)),
             (-4, with_(t0=2**40)), (-1, with_(Tb=0)), (-1, with_(C=0)), (-1, with_(n_ev=0)), (-1, with_(n_slots=0)),
             (-1, with_(t0=-1))]
    cases += [(-1, with_(**{k: None})) for k in ("ids", "anom", "ev_tmin", "ev_off", "cnt", "sums", "vmax", "status")]
    for code, args in cases:  # refused by the library before any launch
        with pytest.raises(ProcessingError, match=rf"marex_event_intensity_f32 failed \(code {code}\)"):
            hot.call("marex_event_intensity_f32", *args)
    hot.sync()
    assert not cnt.any() and not sums.any() and not vmax.any() and not st.any()
    assert np.array_equal(d.cpu().numpy(), ids)


# ------------------------------------------------------------------ the trackers end to end
def assert_within_bound(ds, exp, tv):
    """Arbitrary float32 areas: counts, maxima, durations and times equal; S within 2 n u sum|w a|; the float32 values
    derived from S and W within one float32 ulp."""
    assert list(ds.data_vars)[-len(VARS_T + VARS_E):] == VARS_T + VARS_E
    for k in ("intensity_cells", "intensity_max", "event_duration", "event_intensity_max", "event_invalid_cells"):
        got = np.asarray(ds[k].values)
        assert got.dtype == DTYPES[k] and np.array_equal(got, exp[k], equal_nan=got.dtype.kind == "f"), k
    got, want = np.asarray(ds["intensity_integral"].values), exp["intensity_integral"]
    assert got.dtype == np.float64 and np.array_equal(np.isnan(got), np.isnan(want))
    live = ~np.isnan(want)
    assert (np.abs(got - want)[live] <= (2 * exp["intensity_cells"] * U * exp["abs_integral"])[live]).all()
    for k in ("intensity_mean", "event_intensity_mean", "event_intensity_cumulative"):
        got, want = np.asarray(ds[k].values), exp[k]
        assert got.dtype == np.float32 and np.array_equal(np.isnan(got), np.isnan(want)), k
        live = ~np.isnan(want)
        assert (np.abs(got[live].astype(np.float64) - want[live]) <= np.spacing(np.abs(want[live]))).all(), k
    step = exp["event_step_of_max"]
    assert np.array_equal(np.asarray(ds["event_time_of_max"].values)[step >= 0], np.asarray(tv)[step[step >= 0]])


_grid = {}


def _grid_case():
    if not _grid:
        ev = blobs()
        T, ny, nx = ev.shape
        _grid.update(ev=ev, anom=blob_anomalies(ev.shape), lat=np.linspace(-57.5, 57.5, ny).astype(np.float32),
                     lon=np.linspace(3.75, 356.25, nx).astype(np.float32),
                     tv=np.arange(T).astype("datetime64[D]").astype("datetime64[ns]"))
    return _grid


def _grid_tracker(g, **kw):
    T, ny, nx = g["ev"].shape
    da = DataArray(g["ev"], dims=("time", "lat", "lon"),
                   coords={"time": ("time", g["tv"]), "lat": ("lat", g["lat"]), "lon": ("lon", g["lon"])}, name="extreme_events")
    return marex_amd.tracker(da, DataArray(np.ones((ny, nx), bool), dims=("lat", "lon")), R_fill=1, T_fill=2,
                             area_filter_quartile=0.2, timechunks=4, coordinate_units="degrees", **kw)


@pytest.mark.parametrize("resolution", [None, 7.5], ids=["cells", "grid_resolution"])
def test_merge_tracker_end_to_end(hot, resolution):
    g = _grid_case()
    trk = _grid_tracker(g, allow_merging=True, grid_resolution=resolution)
    events = trk.run()
    before = {k: np.asarray(v.values).copy() for k, v in events.data_vars.items()}
    assert events.attrs["total_merges"] > 0 and events.attrs["N_events_final"] >= 3
    anom = DataArray(g["anom"], dims=("time", "lat", "lon"), coords={"time": ("time", g["tv"])})
    ds = trk.event_intensity(events, anom)
    field = np.asarray(events["ID_field"].values)
    N = int(events["ID"].values.size)
    w = None if resolution is None else trk._cell_weights.reshape(-1)
    exp = io.intensity(field, g["anom"], w, N)
    assert list(ds.data_vars) == list(events.data_vars) + VARS_T + VARS_E and ds.attrs == events.attrs
    for k, v in before.items():  # the tracker's own variables are carried over, the input Dataset is not changed
        assert np.array_equal(np.asarray(ds[k].values), v, equal_nan=v.dtype.kind == "f")
        assert np.array_equal(np.asarray(events[k].values), v, equal_nan=v.dtype.kind == "f")
    if resolution is None:
        assert_equals_oracle(Dataset_view(ds), exp, g["tv"])
    else:
        assert_within_bound(ds, exp, g["tv"])
    pres = np.asarray(events["presence"].values)
    mx, mean = np.asarray(ds["intensity_max"].values), np.asarray(ds["intensity_mean"].values)
    assert np.array_equal(np.isnan(mx), ~pres) and np.array_equal(np.isnan(mean), ~pres)  # every slot here has a finite cell
    assert (mx[pres] >= mean[pres]).all() and np.isnan(g["anom"][field > 0]).any()
    assert np.array_equal(np.asarray(ds["event_duration"].values), pres.sum(0))
    assert np.array_equal(ds["ID"].values, events["ID"].values) and np.array_equal(ds["time"].values, g["tv"])
    assert tuple(ds["intensity_max"].dims) == ("time", "ID") and tuple(ds["event_duration"].dims) == ("ID",)
    if resolution is None:  # blocks, per_timestep off, a resident field
        ev2 = trk.event_intensity(events, _dev(hot, g["anom"]), per_timestep=False, block_steps=5)
        assert list(ev2.data_vars) == list(events.data_vars) + VARS_E
        for k in VARS_E:
            assert np.asarray(ev2[k].values).tobytes() == np.asarray(ds[k].values).tobytes(), k
        # a Dataset that disagrees with its own ID field is refused
        wrong = marex_amd.Dataset({k: v for k, v in events.data_vars.items()})
        wrong["presence"] = DataArray(~pres, dims=tuple(events["presence"].dims))
        with pytest.raises(ProcessingError, match="an event's duration differs from its presence"):
            trk.event_intensity(wrong, anom)


class Dataset_view:
    """The intensity variables of a merged Dataset, in the shape ``assert_equals_oracle`` expects."""

    def __init__(self, ds):
        self.data_vars = {k: ds[k] for k in VARS_T + VARS_E}
        self._ds = ds

    def __getitem__(self, k):
        return self._ds[k]


def test_basic_tracker_through_the_free_function(hot):
    g = _grid_case()
    events = _grid_tracker(g, allow_merging=False).run()
    field = events["ID_field"]
    ids = np.asarray(field.values)
    assert ids.max() >= 2
    anom = DataArray(g["anom"], dims=("time", "lat", "lon"), coords={"time": ("time", g["tv"])})
    exp = io.intensity(ids, g["anom"])
    ds = marex_amd.event_intensity(field, anom)
    assert_equals_oracle(ds, exp, g["tv"])
    wy = np.cos(np.radians(g["lat"])).astype(np.float32)  # arbitrary float32 areas along y
    ds = marex_amd.event_intensity(field, anom, cell_areas=wy, block_steps=7)
    assert_within_bound(ds, io.intensity(ids, g["anom"], np.repeat(wy, ids.shape[2])), g["tv"])
    # the tracker's method on a Dataset without ID / presence: unit weights, the tracker's time name
    both = _grid_tracker(g, allow_merging=False).event_intensity(events, anom)
    assert list(both.data_vars) == ["ID_field"] + VARS_T + VARS_E
    assert_equals_oracle(Dataset_view(both), exp, g["tv"])


def test_mesh_tracker_end_to_end(hot):
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
    field = np.asarray(events["ID_field"].values)
    rng = np.random.default_rng(9)
    anom = (rng.integers(1, 2**13, field.shape) / 1024.0).astype(np.float32)
    anom[rng.random(field.shape) < 0.02] = np.nan
    N = int(events["ID"].values.size)
    ds = trk.event_intensity(events, DataArray(anom, dims=("time", "ncells")), block_steps=32)
    exp = io.intensity(field, anom, np.asarray(f["areas"], np.float32), N)
    assert_within_bound(ds, exp, f["time"])
    pres = np.asarray(events["presence"].values)
    assert np.array_equal(np.asarray(ds["event_duration"].values), pres.sum(0)) and N == 11
    assert np.array_equal(~np.isnan(np.asarray(ds["intensity_integral"].values)), pres & (exp["intensity_cells"] > 0))
    assert tuple(ds["intensity_max"].dims) == ("time", "ID") and "merge_ledger" in ds.data_vars
