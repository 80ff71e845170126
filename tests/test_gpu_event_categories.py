"""GPU parity: severity categories of tracked events (``marex_event_categories_f32`` through ``HotPath.call``,
``HotPath.event_categories``, ``marex_amd.event_categories`` and ``tracker.event_categories``) against the NumPy oracle of
tests/event_categories_oracle.py.  Everything is an exact integer, or a float64 sum of multiples of 2^-10 that is exact in
any order: every comparison is bit for bit."""
import os
import sys

import numpy as np
import pytest
import torch

import marex_amd
from marex_amd import calendar, synth
from marex_amd.engine import HotPath
from marex_amd.exceptions import ProcessingError
from marex_amd.xr_compat import DataArray

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import event_categories_oracle as co  # noqa: E402
from event_categories_cases import N_DOY, N_EV, case, public_case, spans, weights  # noqa: E402
from test_event_categories_host import VARS_E, VARS_T, assert_equals_oracle  # noqa: E402

pytestmark = pytest.mark.gpu

FN = "marex_event_categories_f32"
T = 70  # more rows than the 64 a launch keeps in flight: the row stride wraps
SIZES = [1, 63, 65, 4097]  # 4097: one cell past a workgroup's 4096-cell chunk


def _dev(hot, a):
    return torch.from_numpy(np.array(a, order="C")).to(hot.device)  # np.array copies: the input stays as it is


_exp = {}


def _oracle(C, weighted):
    """The case of C cells and its oracle, once: ``(ids, anom, thr, doy, w, tmin, tmax, off, cnt [n, 7], area [n, 6], exp)``."""
    key = (C, weighted)
    if key not in _exp:
        ids, anom, thr, doy = case(T, C)
        w = weights(C) if weighted else None
        tmin, tmax = spans(ids)
        off = HotPath.event_slot_plan(tmin, tmax, T)
        exp = co.categories(ids, anom, thr, doy, w, N_EV)
        n = int(off[-1])
        cnt, area = np.zeros((n, 7), np.int64), np.zeros((n, 6))
        for e in range(1, N_EV + 1):
            for t in range(int(tmin[e]), int(tmax[e]) + 1):
                s = int(off[e] + t - tmin[e])
                cnt[s], area[s] = exp["slot_cells"][t, e - 1], exp["category_area"][t, e - 1]
        assert cnt.sum() == exp["slot_cells"].sum() == ((ids > 0) & (ids <= N_EV)).sum()
        _exp[key] = (ids, anom, thr, doy, w, tmin, tmax, off, cnt, area, exp)
    return _exp[key]


@pytest.mark.parametrize("weighted", [False, True], ids=["cells", "weights"])
@pytest.mark.parametrize("C", SIZES)
def test_kernel_equals_oracle_whole_and_in_windows(hot, C, weighted):
    ids, anom, thr, doy, w, tmin, tmax, off, cnt, area, exp = _oracle(C, weighted)
    assert HotPath.POISON                                                 # fresh buffers are 0xCD bytes: the zeroing shows
    if C >= 63:
        inside = (ids > 0) & (ids <= N_EV)
        assert (ids < 0).any() and (ids > N_EV).any() and (~np.isfinite(anom[inside])).any()
        assert set(np.unique(exp["category_field"])) == set(range(8))     # no event, the six classes, non-finite
        h = thr[doy]
        for k in (1, 2, 3, 4):                                            # every class boundary is hit exactly, and just missed
            assert (inside & (anom == np.float32(k) * h) & (h > 0)).any()
            assert (inside & (anom == np.nextafter(np.float32(k) * h, np.float32(-np.inf))) & (h > 0) & np.isfinite(h)).any()
        assert len(set(ids[1, :8].tolist()) & set(range(1, 7))) == 5      # several events inside one 64-lane piece
    if C > 4096:
        assert (ids[2, 3000:] == 1).all() and (ids[3, 900:1200] == 4).all()  # one event over pieces, waves and workgroups
    wd = None if w is None else _dev(hot, w)
    thr_d = _dev(hot, thr)
    first = None
    for B in (T, 1, 2, 5, 23):
        d, a = _dev(hot, ids), _dev(hot, anom)
        field = HotPath._buf(None, "t_field", (T, C), torch.uint8, hot.device)
        acc = r = None
        for t0 in range(0, T, B):
            r = hot.event_categories(d[t0:t0 + B], a[t0:t0 + B], tmin, tmax, thr_d, doy, wd, t0=t0, field=field, acc=acc,
                                     finish=t0 + B >= T)
            acc = r["acc"]
        assert r["off"].tolist() == off.tolist()
        assert r["cat_cnt"].dtype == np.int64 and np.array_equal(r["cat_cnt"], cnt), (B, np.argwhere(r["cat_cnt"] != cnt)[:8])
        f = field.cpu().numpy()
        assert np.array_equal(f, exp["category_field"]), (B, np.argwhere(f != exp["category_field"])[:8])
        if weighted:
            assert r["cat_area"].dtype == np.float64 and r["cat_area"].tobytes() == area.tobytes(), B
        else:
            assert r["cat_area"] is None
        assert np.array_equal(d.cpu().numpy(), ids) and a.cpu().numpy().tobytes() == anom.tobytes()  # inputs are read only
        got = (r["cat_cnt"].tobytes(), f.tobytes(), None if not weighted else r["cat_area"].tobytes())
        first = first or got
        assert got == first, B
        # the histogram of the field is the counts, and no cell outside an event is anything but 0
        assert np.bincount(f.reshape(-1), minlength=8)[1:].tolist() == r["cat_cnt"].sum(axis=0).tolist()
        assert not f[~((ids > 0) & (ids <= N_EV))].any()
    # without a field the accumulators are the same
    r = hot.event_categories(_dev(hot, ids), _dev(hot, anom), tmin, tmax, thr_d, doy, wd, finish=True)
    assert r["cat_cnt"].tobytes() == first[0] and (not weighted or r["cat_area"].tobytes() == first[2])


def _own_buffers(hot, n, weighted):
    cnt = torch.zeros((n, 7), dtype=torch.int64, device=hot.device)
    area = torch.zeros((n, 6), dtype=torch.float64, device=hot.device) if weighted else None
    return cnt, area, torch.zeros(2, dtype=torch.int64, device=hot.device)


def test_lost_cells_are_counted_not_accumulated(hot):
    """Event 1's span is declared one step short and event 2's slots follow it: a missing guard would add event 1's last
    step to event 2's first slot -- inside the allocation, so nothing can fault.  A doy label outside 0 .. n_doy - 1 reads
    no threshold: the event cells of its rows are counted in status[1]."""
    C = 65
    ids, anom, thr, doy, w, tmin, tmax, off, cnt, area, exp = _oracle(C, True)
    assert tmax[1] == T - 1 and tmax[2] >= tmin[2] >= 0
    d, a, thr_d, wd = _dev(hot, ids), _dev(hot, anom), _dev(hot, thr), _dev(hot, w)
    short = tmax.copy()
    short[1] -= 1
    lost = int((ids[T - 1] == 1).sum())
    assert lost > 0
    with pytest.raises(ProcessingError, match=rf"event_categories: {lost} cells belong to an event outside"):
        hot.event_categories(d, a, tmin, short, thr_d, doy, wd, finish=True)
    off_s = HotPath.event_slot_plan(tmin, short)
    n = int(off_s[-1])
    exp_s = co.categories(ids, anom, thr, doy, w, N_EV, spans=(tmin, short))
    assert exp_s["status"] == [lost, 0]
    c, ar, st = _own_buffers(hot, n, True)
    field = HotPath._buf(None, "t_field", (T, C), torch.uint8, hot.device)
    hot.call(FN, d, a, 0, T, C, N_EV, _dev(hot, tmin.astype(np.int32)), _dev(hot, off_s), n, thr_d, _dev(hot, doy), N_DOY, wd,
             c, ar, field, st)
    assert st.cpu().tolist() == [lost, 0]
    g = int(off[2])
    assert off_s[2] == g - 1
    assert np.array_equal(c.cpu().numpy()[off_s[2]:], cnt[g:]) and np.array_equal(c.cpu().numpy()[:off_s[2]], cnt[:off_s[2]])
    assert ar.cpu().numpy()[off_s[2]:].tobytes() == area[g:].tobytes()
    assert np.array_equal(field.cpu().numpy(), exp_s["category_field"]) and not field[T - 1][d[T - 1] == 1].any()
    # doy labels out of range, on both sides, in rows 3 and 68 (the second pass of the row stride)
    bad = doy.copy()
    bad[3], bad[68] = N_DOY, -1
    exp_b = co.categories(ids, anom, thr, bad, w, N_EV)
    gone = int(((ids[[3, 68]] > 0) & (ids[[3, 68]] <= N_EV)).sum())
    assert exp_b["status"] == [0, gone] and gone > 0
    with pytest.raises(ProcessingError, match=rf"event_categories: {gone} event cells lie under a step label outside its range"):
        hot.event_categories(d, a, tmin, tmax, thr_d, bad, wd, finish=True)
    n = int(off[-1])
    c, ar, st = _own_buffers(hot, n, True)
    field = HotPath._buf(None, "t_field", (T, C), torch.uint8, hot.device)
    hot.call(FN, d, a, 0, T, C, N_EV, _dev(hot, tmin.astype(np.int32)), _dev(hot, off), n, thr_d, _dev(hot, bad), N_DOY, wd,
             c, ar, field, st)
    assert st.cpu().tolist() == [0, gone]
    assert np.array_equal(field.cpu().numpy(), exp_b["category_field"]) and not field[3].any() and not field[68].any()
    keep = np.ones(n, bool)
    for e in range(1, N_EV + 1):
        for t in (3, 68):
            if tmin[e] <= t <= tmax[e]:
                keep[int(off[e] + t - tmin[e])] = False
    assert np.array_equal(c.cpu().numpy()[keep], cnt[keep]) and not c.cpu().numpy()[~keep].any()
    assert ar.cpu().numpy()[keep].tobytes() == area[keep].tobytes() and not ar.cpu().numpy()[~keep].any()


def test_engine_and_library_check_their_arguments_before_the_launch(hot):
    C = 63
    ids, anom, thr, doy, w, tmin, tmax, off, cnt, area, exp = _oracle(C, True)
    d, a, thr_d, wd = _dev(hot, ids), _dev(hot, anom), _dev(hot, thr), _dev(hot, w)
    first = hot.event_categories(d, a, tmin, tmax, thr_d, doy, wd)
    assert "cat_cnt" not in first  # finish defaults to False: no host read
    field = torch.zeros((T, C), dtype=torch.uint8, device=hot.device)
    for bad in (lambda: hot.event_categories(d.to(torch.int64), a, tmin, tmax, thr_d, doy),
                lambda: hot.event_categories(d, a.to(torch.float64), tmin, tmax, thr_d, doy),
                lambda: hot.event_categories(d, a[:, :-1].contiguous(), tmin, tmax, thr_d, doy),
                lambda: hot.event_categories(d, a.cpu(), tmin, tmax, thr_d, doy),
                lambda: hot.event_categories(d, a, tmin, tmax, thr_d, doy, torch.ones(C + 1, device=hot.device)),
                lambda: hot.event_categories(d, a, tmin, tmax, thr_d.to(torch.float64), doy),
                lambda: hot.event_categories(d, a, tmin, tmax, thr_d[:, :-1].contiguous(), doy),
                lambda: hot.event_categories(d, a, tmin, tmax, thr_d.cpu(), doy),
                lambda: hot.event_categories(d, a, tmin, tmax, None, doy),
                lambda: hot.event_categories(d, a, tmin, tmax, thr_d, None),
                lambda: hot.event_categories(d, a, tmin, tmax, thr_d, doy.astype(np.float32)),
                lambda: hot.event_categories(d, a, tmin, tmax, thr_d, doy[:-1]),                  # does not reach the window
                lambda: hot.event_categories(d, a, tmin[:1], tmax[:1], thr_d, doy),
                lambda: hot.event_categories(d, a, tmin, tmax, thr_d, doy, t0=-1),
                lambda: hot.event_categories(d, a, tmin, tmax, thr_d, doy, field=field[:-1]),      # not the whole output
                lambda: hot.event_categories(d, a, tmin, tmax, thr_d, doy, field=field.to(torch.int32)),
                lambda: hot.event_categories(d, a, tmin, tmax, thr_d, doy, acc=first["acc"]),      # planned with weights
                lambda: hot.event_categories(d, a, tmin, tmax - 1, thr_d, doy, wd, acc=first["acc"])):
        with pytest.raises(ProcessingError):
            bad()
    n = int(off[-1])
    c, ar, st = _own_buffers(hot, n, True)
    ok = (d, a, 0, T, C, N_EV, _dev(hot, tmin.astype(np.int32)), _dev(hot, off), n, thr_d, _dev(hot, doy), N_DOY, wd, c, ar, field, st)
    names = ("ids", "anom", "t0", "Tb", "C", "n_ev", "ev_tmin", "ev_off", "n_slots", "thr", "doy", "n_doy", "w", "cat_cnt", "cat_area",
             "field", "status")

    def with_(**kw):
        return tuple(kw.get(k, v) for k, v in zip(names, ok))

    cases = [(-4, with_(C=2**31 - 1)), (-4, with_(C=2**40)), (-4, with_(Tb=2**31 - 1)), (-4, with_(t0=2**31 - 1 - T)),
             (-4, with_(t0=2**40)), (-1, with_(Tb=0)), (-1, with_(C=0)), (-1, with_(n_ev=0)), (-1, with_(n_slots=0)),
             (-1, with_(t0=-1)), (-1, with_(n_doy=0)), (-1, with_(n_doy=-3))]
    cases += [(-1, with_(**{k: None})) for k in ("ids", "anom", "ev_tmin", "ev_off", "cat_cnt", "status", "thr", "doy", "w", "cat_area")]
    for code, args in cases:  # refused by the library before any launch
        with pytest.raises(ProcessingError, match=rf"{FN} failed \(code {code}\)"):
            hot.call(FN, *args)
    hot.sync()
    assert not c.any() and not ar.any() and not st.any() and not field.any()
    assert np.array_equal(d.cpu().numpy(), ids)
    hot.call(FN, *with_(field=None))  # the field is optional
    assert np.array_equal(c.cpu().numpy(), cnt) and ar.cpu().numpy().tobytes() == area.tobytes() and not field.any()


def _resident(hot, da):
    t = torch.from_numpy(np.ascontiguousarray(da.values)).to(hot.device)
    return DataArray(t, dims=tuple(da.dims), coords={k: (tuple(v.dims), np.asarray(v.values)) for k, v in da.coords.items()})


@pytest.mark.parametrize("mesh", [False, True], ids=["grid", "mesh"])
def test_public_api_resident_and_host_whole_and_in_windows(hot, mesh):
    ny, nx = 17, 241  # 4097 cells
    C = ny * nx
    ids, anom, thr, doy = public_case(T, C)
    w = weights(C)
    exp = co.categories(ids, anom, thr, doy, w, N_EV)
    sp, dims = ((C,), ("time", "ncells")) if mesh else ((ny, nx), ("time", "lat", "lon"))
    # the public layouts need the 366 rows of a year: the three rows of the case go to the days of 70 consecutive dates,
    # every other row would put every cell into another class
    dates = (np.datetime64("2021-03-01", "D") + np.arange(T)).astype("datetime64[ns]")
    day = calendar._to_year_doy(dates)[1].astype(np.int64) - 1
    thr366 = np.full((366, C), 1000.0, np.float32)
    for t in range(T):
        thr366[day[t]] = thr[doy[t]]
    da_i = DataArray(ids.reshape((T,) + sp), dims=dims, coords={"time": ("time", dates)})
    da_a = DataArray(anom.reshape((T,) + sp), dims=dims, coords={"time": ("time", dates)})
    th = thr366.reshape((366,) + sp)
    area = w.reshape(sp)
    whole = marex_amd.event_categories(da_i, da_a, th, area, per_timestep=True, return_field=True)
    assert_equals_oracle(whole, exp, dates, True, True, True)
    assert isinstance(whole["category_field"].values, np.ndarray) and tuple(whole["category_field"].dims) == dims
    ri, ra, rt = _resident(hot, da_i), _resident(hot, da_a), torch.from_numpy(th).to(hot.device)
    for b in (1, 2, 5, 23, None, "auto"):
        for dev in (False, True):
            i, a, h = (ri, ra, rt) if dev else (da_i, da_a, th)
            ds = marex_amd.event_categories(i, a, h, area, per_timestep=True, return_field=True, block_steps=b)
            f = ds["category_field"].data
            assert torch.is_tensor(f) == dev and (not dev or (f.device == hot.device and f.dtype == torch.uint8))
            assert tuple(f.shape) == (T,) + sp
            assert (f.cpu().numpy() if dev else f).tobytes() == np.asarray(whole["category_field"].values).tobytes(), (b, dev)
            for k in VARS_T + VARS_E:
                assert np.asarray(ds[k].values).tobytes() == np.asarray(whole[k].values).tobytes(), (b, dev, k)
    # other types are converted on the way: float64 anomalies, int64 IDs, thresholds with dayofyear last
    last = np.ascontiguousarray(np.moveaxis(th, 0, -1))
    ds = marex_amd.event_categories(DataArray(ids.astype(np.int64).reshape((T,) + sp), dims=dims, coords={"time": ("time", dates)}),
                                    DataArray(anom.astype(np.float64).reshape((T,) + sp), dims=dims), last, block_steps=23)
    assert_equals_oracle(ds, co.categories(ids, anom, thr, doy, None, N_EV), dates)
    none = marex_amd.event_categories(np.zeros((T, C), np.int32), anom, thr[0], return_field=True)
    assert none["ID"].values.size == 0 and not np.asarray(none["category_field"].values).any()


def test_identities_with_event_intensity_and_local_intensity(hot):
    C = 4097
    ids, anom, thr, doy = public_case(T, C)
    tmin, tmax = spans(ids)
    d, a, thr_d = _dev(hot, ids), _dev(hot, anom), _dev(hot, thr)
    cat = hot.event_categories(d, a, tmin, tmax, thr_d, doy, finish=True)
    inten = hot.event_intensity(d, a, tmin, tmax)
    assert cat["off"].tolist() == inten["off"].tolist()
    # slot for slot: the classified cells are the finite ones, class 6 the non-finite ones
    assert np.array_equal(cat["cat_cnt"][:, :6].sum(axis=1), inten["cnt"][:, 0]) and np.array_equal(cat["cat_cnt"][:, 6], inten["cnt"][:, 1])
    assert inten["cnt"][:, 1].sum() > 0
    g = thr[0]  # one threshold per cell: no dates needed
    ds = marex_amd.event_categories(ids, anom, g, per_timestep=True)
    di = marex_amd.event_intensity(ids, anom)
    assert np.array_equal(np.asarray(ds["category_cells"].values).sum(axis=2), np.asarray(di["intensity_cells"].values))
    assert np.array_equal(np.asarray(ds["event_category_steps"].values).sum(axis=1), np.asarray(di["event_duration"].values))
    assert np.array_equal(np.asarray(ds["event_invalid_cells"].values), np.asarray(di["event_invalid_cells"].values))
    # a mask cast to int32 is one event: its per-class totals are local_intensity's category days summed over the cells
    mask = (ids > 0).astype(np.int32)
    one = marex_amd.event_categories(mask, anom, g)
    li = marex_amd.local_intensity(mask, anom, g)
    days = np.asarray(li["category_days"].values).astype(np.int64)
    assert days.shape == (6, C) and days.sum() > 0
    assert np.asarray(one["event_category_cell_steps"].values).tolist() == [days.sum(axis=1).tolist()]
    assert int(np.asarray(one["event_category"].values)[0]) == int(np.asarray(li["category_peak"].values).max())


def test_field_addresses_past_32_bits(hot):
    """A field of 4099 x 2^20 bytes and a window that starts at step 4097 with events only in its last row: t C exceeds 2^32.
    Two rows of the inputs are touched; the field takes 4.3 GB."""
    C, t0, Tf = 2**20, 4097, 4099
    field = torch.empty((Tf, C), dtype=torch.uint8, device=hot.device)
    field[t0 - 1:].fill_(9)
    ids = torch.zeros((2, C), dtype=torch.int32, device=hot.device)
    anom = torch.full((2, C), 2.5, dtype=torch.float32, device=hot.device)
    thr = torch.ones((1, C), dtype=torch.float32, device=hot.device)
    cells = [0, 5, 6, 2**19, C - 1]
    for k, c in enumerate(cells):
        ids[1, c] = 1 + k % 2
        thr[0, c] = [1.0, 2.0, 0.5, 3.0, 1.0][k]
    tmin, tmax = np.array([0, Tf - 1, Tf - 1]), np.array([0, Tf - 1, Tf - 1])
    r = hot.event_categories(ids, anom, tmin, tmax, thr, np.zeros(Tf, np.int32), t0=t0, field=field, finish=True)
    assert (Tf - 1) * C > 2**32
    # 2.5 under 1, 2, 0.5, 3, 1: strong, moderate, extreme, below, strong; events 1, 2, 1, 2, 1
    assert r["cat_cnt"].tolist() == [[0, 0, 2, 0, 1, 0, 0], [1, 1, 0, 0, 0, 0, 0]]
    rows = field[t0:].cpu().numpy()
    assert rows[1, cells].tolist() == [3, 2, 5, 1, 3] and rows.sum() == 14 and not rows[0].any()
    assert bool((field[t0 - 1] == 9).all())
    del field, ids, anom, thr, r
    torch.cuda.empty_cache()


def test_preprocess_track_and_categorise_end_to_end(hot):
    """``preprocess_data`` -> ``tracker.run()`` -> ``tracker.event_categories`` on a small synthetic field, equal to the
    oracle on the host copies of ``ID_field``, ``dat_anomaly`` and ``thresholds``."""
    ny, nx = 16, 32
    tm = calendar.daily_time_axis("2010-01-01", 12 * 365 + 3)
    x = synth.synth_field(synth.make_tables(tm, ny, nx)).reshape(tm.size, ny, nx)
    yy, xx = np.mgrid[0:ny, 0:nx]
    for k in range(8):  # warm discs of 12 days and 2 .. 5.5 degrees over the open rows: events of several categories
        disc = (yy - (4 if k % 2 == 0 else 11)) ** 2 + (xx - (3 + 4 * k)) ** 2 <= 2.2 ** 2
        x[2400 + 200 * k:2412 + 200 * k, disc] += np.float32(2.0 + 0.5 * k)
    da = DataArray(x, dims=("time", "lat", "lon"), coords={"time": tm, "lat": np.linspace(-56.25, 56.25, ny), "lon": np.linspace(0, 348.75, nx)},
                   name="sst")
    extremes = marex_amd.preprocess_data(da, window_year_baseline=5)
    trk = marex_amd.tracker(extremes["extreme_events"], extremes["mask"], R_fill=1, T_fill=2, area_filter_quartile=0.2,
                            allow_merging=False, quiet=True)
    events = trk.run()
    ids = np.asarray(events["ID_field"].values)
    Tn = ids.shape[0]
    N = int(ids.max())
    assert N >= 4
    ds = trk.event_categories(events, extremes, per_timestep=True, return_field=True, block_steps=1000)
    thr = np.moveaxis(np.asarray(extremes["thresholds"].values), -1, 0).reshape(366, ny * nx)
    assert tuple(extremes["thresholds"].dims) == ("lat", "lon", "dayofyear")
    tv = np.asarray(extremes["dat_anomaly"].coords["time"].values)
    doy = calendar._to_year_doy(tv)[1].astype(np.int32) - 1
    exp = co.categories(ids.reshape(Tn, -1), np.asarray(extremes["dat_anomaly"].values).reshape(Tn, -1), thr, doy, None, N)
    assert list(ds.data_vars) == list(events.data_vars) + [v for v in VARS_T if v != "category_area"] + VARS_E + ["category_field"]

    class View:
        data_vars = {k: ds[k] for k in list(ds.data_vars)[len(list(events.data_vars)):]}

        def __getitem__(self, k):
            return ds[k]

    assert_equals_oracle(View(), exp, tv, True, False, True)
    assert ds.attrs == events.attrs and exp["event_category_cell_steps"][:, 1].sum() > 0
    assert (exp["event_category"] >= 2).any() and len(set(exp["event_category"].tolist())) >= 2
    # the filled gaps of the tracker are cells below the threshold; nothing is undefined on this field
    assert exp["event_category_cell_steps"][:, 0].sum() > 0 and exp["event_category_cell_steps"][:, 5].sum() == 0
    whole = marex_amd.event_categories(events["ID_field"], extremes["dat_anomaly"], extremes["thresholds"])
    for k in VARS_E:
        assert np.asarray(whole[k].values).tobytes() == np.asarray(ds[k].values).tobytes(), k
