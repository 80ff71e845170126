"""GPU: the tracker's pre-processing in time blocks gives bit for bit what the whole-field path gives
-- the compaction kernel against NumPy, ``HotPath.preprocess_blocked`` against the three whole-field calls and the host
oracle for every block length, hand-built cases on the seams, the first-object rule, the ``preprocess_block_steps``
keyword of ``tracker`` on grids and meshes, and the peak of torch's allocations against the memory model."""
import os
import sys

import numpy as np
import pytest
import torch

import marex_amd
import marex_amd.track as trk_mod
import marex_amd.track_pre as tp
from marex_amd.exceptions import ProcessingError
from marex_amd.xr_compat import DataArray
from marex_amd.zarr_io import DeviceDataArray

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import label_blocks_oracle as lbo  # noqa: E402
import track_oracle as tor  # noqa: E402
from test_mesh_tracker_host import load_mesh_fixture, mesh_tracker  # noqa: E402
from test_track_host import REFERENCE_ROWS, load_fixture  # noqa: E402

pytestmark = pytest.mark.gpu

TILE = 4096  # CCL_TILE of csrc/marex_morphology.hip: the entries one workgroup of the compaction counts and scatters


# ------------------------------------------------------------------ 1. the compaction kernel
def _compact(hot, v_dev, cap):
    """One raw call: ``(rc, out incl. an 8-entry guard, n_out, first_index)``."""
    GUARD = 8
    out = torch.full((cap + GUARD,), -77, dtype=torch.int32, device=hot.device)
    res = torch.full((2,), -5, dtype=torch.int64, device=hot.device)
    hot._bind_stream()
    rc = hot.lib.marex_compact_positive_i32(hot.ctx.handle, v_dev.data_ptr(), int(v_dev.numel()), out.data_ptr(), cap,
                                            res.data_ptr(), res.data_ptr() + 8)
    hot.sync()
    r = res.cpu().numpy()
    return rc, out.cpu().numpy(), int(r[0]), int(r[1])


def _patterns(rng, n):
    mixed = rng.integers(-3, 4, n).astype(np.int32) * rng.integers(1, 1000, n).astype(np.int32)
    none = -np.abs(mixed)
    allpos = np.abs(mixed) + 1
    last = none.copy()
    last[-1] = 7
    last_tile = none.copy()
    lo = ((n - 1) // TILE) * TILE
    last_tile[lo:] = np.abs(mixed[lo:]) + (np.arange(n - lo) % 3 == 0)
    return {"mixed": mixed, "none": none, "all": allpos, "last element": last, "last tile": last_tile}


@pytest.mark.parametrize("n", [1, 63, 64, 65, 255, 256, 257, TILE - 1, TILE, TILE + 1, 3 * 2**20 + 5])
def test_compaction_equals_numpy(hot, n):
    rng = np.random.default_rng(n)
    for name, v in _patterns(rng, n).items():
        exp = v[v > 0]
        base = torch.from_numpy(np.concatenate([np.full(3, 5, np.int32), v])).to(hot.device)
        for vd in (torch.from_numpy(v).to(hot.device), base[3:]):  # aligned, and an unaligned slice
            rc, out, cnt, first = _compact(hot, vd, max(1, exp.size))
            assert rc == 0 and cnt == exp.size, (name, n, rc, cnt, exp.size)
            assert first == (int(np.flatnonzero(v > 0)[0]) if exp.size else -1), (name, n)
            assert np.array_equal(out[:exp.size], exp), (name, n)
            assert (out[max(1, exp.size):] == -77).all() and (exp.size or out[0] == -77), (name, n)
        lst, cnt, fidx = hot.compact_positive(torch.from_numpy(v).to(hot.device))
        assert cnt == exp.size and np.array_equal(lst[:cnt].cpu().numpy(), exp) and int(fidx.item()) == (
            int(np.flatnonzero(v > 0)[0]) if exp.size else -1)


@pytest.mark.parametrize("n", [65, TILE + 1, 3 * 2**20 + 5])
def test_compaction_with_too_little_room_reports_the_count_and_stays_inside(hot, n):
    rng = np.random.default_rng(n + 1)
    v = _patterns(rng, n)["mixed"]
    v[0], v[-1] = 3, 9
    exp = v[v > 0]
    for cap in (exp.size - 1, 0):
        rc, out, cnt, first = _compact(hot, torch.from_numpy(v).to(hot.device), cap)
        assert rc < 0 and cnt == exp.size and first == 0
        assert np.array_equal(out[:cap], exp[:cap]) and (out[cap:] == -77).all()
    # the engine grows its list and carries the entries before `used` over
    have = torch.arange(10, dtype=torch.int32, device=hot.device)
    lst, cnt, _ = hot.compact_positive(torch.from_numpy(v).to(hot.device), have, 10)
    assert cnt == exp.size and np.array_equal(lst[:10 + cnt].cpu().numpy(), np.concatenate([np.arange(10), exp]))


def test_compaction_refuses_bad_arguments(hot):
    v = torch.ones(8, dtype=torch.int32, device=hot.device)
    res = torch.zeros(2, dtype=torch.int64, device=hot.device)
    f, h = hot.lib.marex_compact_positive_i32, hot.ctx.handle
    p = v.data_ptr()
    assert f(h, None, 8, p, 8, res.data_ptr(), res.data_ptr() + 8) != 0
    assert f(h, p, 8, None, 8, res.data_ptr(), res.data_ptr() + 8) != 0
    assert f(h, p, 8, p, 8, None, res.data_ptr()) != 0 and f(h, p, 8, p, 8, res.data_ptr(), None) != 0
    assert f(h, p, 0, p, 8, res.data_ptr(), res.data_ptr() + 8) != 0 and f(h, p, -1, p, 8, res.data_ptr(), res.data_ptr() + 8) != 0
    assert f(h, p, 2**31 - 1, p, 8, res.data_ptr(), res.data_ptr() + 8) != 0
    assert f(None, p, 8, p, 8, res.data_ptr(), res.data_ptr() + 8) != 0


# ------------------------------------------------------------------ 2. blocked equals whole, on grids
def _dev(hot, x):
    return torch.from_numpy(np.ascontiguousarray(x).reshape(x.shape[0], -1).astype(np.uint8)).to(hot.device)


def _whole(hot, xd, mk, ny, nx, R, Tf, quart, absolute, regional):
    """The existing three-call chain and ``object_stats`` as ``_preprocess_device`` forms them."""
    a = hot.fill_holes(xd, mk, ny, nx, R, regional)
    g = hot.fill_time_gaps(a, mk, ny, nx, R, Tf, regional)
    r = hot.filter_small_objects(g, ny, nx, quart, absolute, regional)
    filtered, stats = tp._preprocess_device(hot, xd, mk, ny, nx, R, Tf, quart, absolute, regional)
    assert torch.equal(filtered, r["filtered"])
    return r, stats


def _blocked(hot, xd, mk, ny, nx, R, Tf, quart, absolute, regional, B):
    r = hot.preprocess_blocked(xd, mk, R, Tf, B, quart, absolute, ny=ny, nx=nx, regional_mode=regional)
    hot.sync()
    return r, tp._blocked_stats(r)


def _same(got, exp, what):
    (rg, sg), (re_, se) = got, exp
    assert "labels" not in rg
    assert torch.equal(rg["filtered"], re_["filtered"]), (what, torch.nonzero(rg["filtered"] != re_["filtered"])[:5])
    assert rg["object_areas"].dtype == re_["object_areas"].dtype and torch.equal(rg["object_areas"], re_["object_areas"]), what
    assert rg["area_threshold"] == re_["area_threshold"] and (rg["n_before"], rg["n_after"]) == (re_["n_before"], re_["n_after"]), what
    assert len(sg) == 6 and np.array_equal(np.float64(sg), np.float64(se), equal_nan=True), (what, sg, se)


def _grid_field(shape):
    rng = np.random.default_rng(sum(shape))
    T, ny, nx = shape
    ev = lbo.blobby(rng, shape, 0.2)
    mask = np.ones((ny, nx), bool)
    mask[0] = False
    mask[ny // 2, nx // 3:nx // 2] = False
    return ev, mask


@pytest.mark.parametrize("absolute", [None, 3.0])
@pytest.mark.parametrize("regional", [False, True])
@pytest.mark.parametrize("shape", [(14, 48, 96), (11, 5, 35)])
def test_blocked_equals_whole_on_grids(hot, shape, regional, absolute):
    ev, mask = _grid_field(shape)
    T, ny, nx = shape
    xd, mk = _dev(hot, ev), torch.from_numpy(mask.reshape(-1).astype(np.uint8)).to(hot.device)
    quart = 0.4
    runs = 0
    for Tf in (0, 2, 4):
        for R in (0, 1, 2):
            try:
                exp = _whole(hot, xd, mk, ny, nx, R, Tf, quart, absolute, regional)
            except ProcessingError:
                for B in (1, T):
                    with pytest.raises(ProcessingError, match="No objects found for area-based filtering"):
                        _blocked(hot, xd, mk, ny, nx, R, Tf, quart, absolute, regional, B)
                continue
            o_f, o_st = tor.preprocess(ev, mask, R, Tf, quart, absolute, regional)
            assert np.array_equal(exp[0]["filtered"].cpu().numpy().reshape(shape).astype(bool), o_f)
            assert np.array_equal(np.float64(exp[1]), np.float64(o_st), equal_nan=True), (exp[1], o_st)
            for B in (1, 2, 3, 5, T - 1, T, T + 3):
                _same(_blocked(hot, xd, mk, ny, nx, R, Tf, quart, absolute, regional, B), exp, (shape, Tf, R, B))
                runs += 1
    assert runs >= 7 * 6  # the small shape may lose all its objects to a large R_fill, not most configurations


def test_blocked_from_a_host_array_uploads_windows_only(hot):
    ev, mask = _grid_field((14, 48, 96))
    T, ny, nx = ev.shape
    for B, Tf in ((3, 2), (1, 4), (14, 2)):
        exp = tp.run_preprocess(ev, mask, R_fill=2, T_fill=Tf, area_filter_quartile=0.4)
        got = tp.run_preprocess(ev, mask, R_fill=2, T_fill=Tf, area_filter_quartile=0.4, block_steps=B)
        assert got[0].dtype == bool and np.array_equal(got[0], exp[0]) and tuple(got[1]) == tuple(exp[1])
    for bad in (0, -2, 1.5, True):
        with pytest.raises(marex_amd.exceptions.ConfigurationError, match="block_steps"):
            tp.run_preprocess(ev, mask, R_fill=2, block_steps=bad)


# ------------------------------------------------------------------ 3. hand-built cases on the seams
def _seam_field(Tf):
    """``(field bool [9, 6, 32], {case name: [(cell, expected column)]})``.  R_fill = 0 and an absolute filter of one cell
    make every cell a column of its own: only the temporal closing acts on it.  Cell 0 is set throughout: it holds the
    first object of the list, which the filter drops at t = 0; its neighbours (cells 1, 32 and 33) stay empty."""
    T, ny, nx = 9, 6, 32
    x = np.zeros((T, ny * nx), bool)
    cases, cell = {}, [2]

    def col(name, present, expected):
        c = cell[0]
        cell[0] += 1
        x[list(present), c] = True
        e = np.zeros(T, bool)
        e[list(expected)] = True
        cases.setdefault(name, []).append((c, e))

    x[:, 0] = True
    for s in range(1, T - 1):  # the gap on row s: the first row of a block for every B that divides s
        col("one-step gap", (s - 1, s + 1), (s - 1, s, s + 1))
    for a in range(1, T - Tf):  # gap rows a .. a + Tf - 1 straddle every seam in between
        col("gap of T_fill: closed", (a - 1, a + Tf), range(a - 1, a + Tf + 1))
    for a in range(1, T - Tf - 1):
        col("gap of T_fill + 1: open", (a - 1, a + Tf + 1), (a - 1, a + Tf + 1))
    col("only t = 0", (0,), (0,))
    col("only t = T - 1", (T - 1,), (T - 1,))
    col("first and last", (0, T - 1), (0, T - 1) if T - 2 > Tf else range(T))
    assert cell[0] <= nx  # all on the first grid row, clear of cell 0's neighbours
    return x.reshape(T, ny, nx), cases


@pytest.mark.parametrize("Tf", [2, 4])
def test_hand_built_seam_cases(hot, Tf):
    x, cases = _seam_field(Tf)
    T, ny, nx = x.shape
    xd = _dev(hot, x)
    mk = torch.ones(ny * nx, dtype=torch.uint8, device=hot.device)
    exp = _whole(hot, xd, mk, ny, nx, 0, Tf, 0.5, 1.0, True)
    for B in range(1, T + 1):
        got = _blocked(hot, xd, mk, ny, nx, 0, Tf, 0.5, 1.0, True, B)
        f = got[0]["filtered"].cpu().numpy().astype(bool)
        for name, cols in cases.items():
            for c, e in cols:
                assert np.array_equal(f[:, c], e), (name, "T_fill", Tf, "B", B, "cell", c, f[:, c].astype(int), e.astype(int))
        assert not f[0, 0] and f[1:, 0].all()  # the first object of the list, dropped at t = 0 only
        _same(got, exp, (Tf, B))


# ------------------------------------------------------------------ 4. the first-object rule
def _first_object_field():
    T, ny, nx = 7, 8, 16
    x = np.zeros((T, ny, nx), bool)
    for t in range(2, T):
        x[t, 0:3, 0:3] = True          # 9 cells: the first object of every step from t = 2 on
        x[t, 5, 5:5 + (t % 3) + 1] = True  # 1..3 cells
        x[t, 6:8, 10:12] = True        # 4 cells
        x[t, 4, 14] = True             # 1 cell
    return x


@pytest.mark.parametrize("absolute", [None, 4.0])
def test_the_first_object_is_dropped_exactly_once_for_every_block_length(hot, absolute):
    x = _first_object_field()
    T, ny, nx = x.shape
    xd = _dev(hot, x)
    mk = torch.ones(ny * nx, dtype=torch.uint8, device=hot.device)
    exp = _whole(hot, xd, mk, ny, nx, 0, 0, 0.5, absolute, True)
    thr = exp[0]["area_threshold"]
    assert thr <= 9 and exp[0]["n_after"] == int((exp[0]["object_areas"].cpu().numpy() >= thr).sum()) - 1
    for B in range(1, T + 2):
        got = _blocked(hot, xd, mk, ny, nx, 0, 0, 0.5, absolute, True, B)
        f = got[0]["filtered"].cpu().numpy().reshape(x.shape).astype(bool)
        assert not f[:2].any() and not f[2, 0:3, 0:3].any(), B      # dropped in the block that holds it ...
        assert all(f[t, 0:3, 0:3].all() for t in range(3, T)), B    # ... and nowhere else
        assert f[2, 6:8, 10:12].all()
        _same(got, exp, B)


def test_a_field_without_objects_raises_for_every_block_length(hot):
    T, ny, nx = 7, 8, 16
    xd = torch.zeros((T, ny * nx), dtype=torch.uint8, device=hot.device)
    mk = torch.ones(ny * nx, dtype=torch.uint8, device=hot.device)
    for absolute in (None, 2.0):
        with pytest.raises(ProcessingError, match="No objects found for area-based filtering"):
            _whole(hot, xd, mk, ny, nx, 1, 2, 0.5, absolute, False)
        for B in range(1, T + 2):
            with pytest.raises(ProcessingError, match="No objects found for area-based filtering"):
                _blocked(hot, xd, mk, ny, nx, 1, 2, 0.5, absolute, False, B)


# ------------------------------------------------------------------ 5. the tracker
def _synthetic():
    rng = np.random.default_rng(77)
    T, ny, nx = 14, 48, 96
    ev = lbo.blobby(rng, (T, ny, nx), 0.15)
    mask = np.ones((ny, nx), bool)
    mask[:3] = False
    mask[20:24, 30:40] = False
    coords = {"time": np.arange(T), "lat": np.linspace(-70, 70, ny), "lon": np.linspace(0, 360, nx, endpoint=False)}
    return ev, mask, coords, dict(R_fill=2, T_fill=2, area_filter_quartile=0.4)


def _fixture():
    R, Tf, q, poles = REFERENCE_ROWS[4][0]
    ev, mask, lat, lon, tm = load_fixture(poles)
    return ev, mask, {"time": tm, "lat": lat, "lon": lon}, dict(R_fill=R, T_fill=Tf, area_filter_quartile=q)


def _run(capsys, da, mk, **kw):
    ds = marex_amd.tracker(da, mk, allow_merging=False, **kw).run()
    return ds, capsys.readouterr().out


def _same_run(a, b, what):
    (da, oa), (db, ob) = a, b
    assert sorted(da.data_vars) == sorted(db.data_vars) and len(da.data_vars) >= 1, what
    for k in da.data_vars:
        va, vb = np.asarray(da[k].values), np.asarray(db[k].values)
        assert va.dtype == vb.dtype and np.array_equal(va, vb), (what, k)
    assert da.attrs == db.attrs and list(da.attrs) == list(db.attrs), what
    assert oa == ob, what


@pytest.mark.parametrize("resident", [False, True])
@pytest.mark.parametrize("field", [_synthetic, _fixture])
def test_tracker_with_preprocess_block_steps(hot, capsys, monkeypatch, field, resident):
    ev, mask, coords, kw = field()
    T = ev.shape[0]
    mk = DataArray(mask, dims=("lat", "lon"))
    if resident:
        da = DeviceDataArray(torch.from_numpy(ev).to(hot.device), ("time", "lat", "lon"), coords)
    else:
        da = DataArray(ev, dims=("time", "lat", "lon"), coords=coords)
    base = _run(capsys, da, mk, **kw)
    assert base[0].attrs["N_events_final"] > 3 and "Total Events Tracked" in base[1]
    base2 = _run(capsys, da, mk, label_block_steps=2, **kw)
    _same_run(base2, base, "label_block_steps=2")

    rows = []
    upload = tp._upload_rows
    monkeypatch.setattr(tp, "_upload_rows", lambda host, t0, t1, buf: (rows.append(t1 - t0), upload(host, t0, t1, buf))[1])
    whole_upload = trk_mod.tracker._device_u8

    def no_whole_upload(self, d, eng):
        assert trk_mod._tensor_of(d) is not None, "a host array was uploaded whole"
        return whole_upload(self, d, eng)

    monkeypatch.setattr(trk_mod.tracker, "_device_u8", no_whole_upload)
    for k in (1, 3, 7, T, "auto"):
        del rows[:]
        _same_run(_run(capsys, da, mk, preprocess_block_steps=k, **kw), base, k)
        if resident:
            assert not rows
        elif k != "auto":
            assert rows and max(rows) <= min(T, k + 2 * kw["T_fill"]) and (k >= T or max(rows) < T), (k, rows)
        _same_run(_run(capsys, da, mk, preprocess_block_steps=k, label_block_steps=2, **kw), base, (k, "label blocks"))


# ------------------------------------------------------------------ 6. meshes
def _mesh_cases():
    f = load_mesh_fixture()
    yield "fixture", f["ev"], f["mask"], f["nb"], f["areas"], f["lat"], f["lon"], f["time"], dict(R_fill=3, area_filter_quartile=0.5)
    from test_gpu_mesh_objects import _mesh

    rng = np.random.default_rng(9)
    C, T = 4100, 9
    m = _mesh(rng, C)
    x = rng.random((T, C)) < 0.35
    x[3] = False
    yield ("synthetic", x, m["mask"], m["nb0"] + 1, m["areas"], m["lat"], m["lon"], None,
           dict(R_fill=1, area_filter_quartile=None, area_filter_absolute=6))
    yield ("synthetic, percentile", x, m["mask"], m["nb0"] + 1, m["areas"], m["lat"], m["lon"], None,
           dict(R_fill=1, area_filter_quartile=0.3))


@pytest.mark.parametrize("Tf", [0, 2])
def test_mesh_run_preprocess_in_blocks(hot, Tf):
    for name, ev, mask, nb, areas, lat, lon, tm, kw in _mesh_cases():
        T = ev.shape[0]
        try:
            pre0, st0 = mesh_tracker(ev, mask, nb, areas, lat, lon, tm=tm, T_fill=Tf, **kw).run_preprocess()
        except ProcessingError:  # no cluster of more than 50 cells with these parameters: the same error in blocks
            for k in (1, T):
                with pytest.raises(ProcessingError, match="No objects found for area-based filtering"):
                    mesh_tracker(ev, mask, nb, areas, lat, lon, tm=tm, T_fill=Tf, preprocess_block_steps=k, **kw).run_preprocess()
            assert name != "synthetic"
            continue
        assert int(pre0.device_tensor.sum().item()) > 0
        for k in (1, 2, T, "auto"):
            pre, st = mesh_tracker(ev, mask, nb, areas, lat, lon, tm=tm, T_fill=Tf, preprocess_block_steps=k, **kw).run_preprocess()
            assert tuple(pre.dims) == tuple(pre0.dims) and torch.equal(pre.device_tensor, pre0.device_tensor), (name, k)
            assert len(st) == 6 and np.array_equal(np.float64(st), np.float64(st0), equal_nan=True), (name, k, st, st0)
        xd = torch.from_numpy(ev).to(hot.device)
        trk = mesh_tracker(ev, mask, nb, areas, lat, lon, tm=tm, T_fill=Tf, preprocess_block_steps=2, **kw)
        trk.data_bin = DeviceDataArray(xd, ("time", "ncells"), {"time": trk.time_values, "lat": lat, "lon": lon})
        pre, st = trk.run_preprocess()
        assert torch.equal(pre.device_tensor, pre0.device_tensor) and np.array_equal(np.float64(st), np.float64(st0), equal_nan=True)


# ------------------------------------------------------------------ 7. memory
def test_peak_memory_stays_within_the_model(hot, capsys):
    T, ny, nx = 40, 96, 192
    rng = np.random.default_rng(5)
    ev = lbo.blobby(rng, (T, ny, nx), 0.15)
    coords = {"time": np.arange(T), "lat": np.linspace(-70, 70, ny), "lon": np.linspace(0, 360, nx, endpoint=False)}
    da = DeviceDataArray(torch.from_numpy(ev).to(hot.device), ("time", "lat", "lon"), coords)
    mk = DataArray(np.ones((ny, nx), bool), dims=("lat", "lon"))
    kw = dict(R_fill=2, T_fill=2, area_filter_quartile=0.5, allow_merging=False)

    def peak(**more):
        trk = marex_amd.tracker(da, mk, **kw, **more)
        hot.sync()
        torch.cuda.synchronize()
        before = torch.cuda.memory_allocated(hot.device)
        torch.cuda.reset_peak_memory_stats(hot.device)
        pre, stats = trk.run_preprocess()
        hot.sync()
        return torch.cuda.max_memory_allocated(hot.device) - before, pre.device_tensor.clone(), stats

    need = trk_mod.preprocess_memory_need(T, ny, ny * nx, 2, 2, 4, resident=True)
    bound = sum(v for k, v in need.items() if k not in ("library scratch", trk_mod._RESIDENT_INPUT))  # torch's own entries
    blocked, f1, s1 = peak(preprocess_block_steps=4)
    whole, f0, s0 = peak()
    print(f"peak of torch allocations over run_preprocess: blocked {blocked} B, model {bound} B, whole field {whole} B")
    assert torch.equal(f0, f1) and tuple(s0) == tuple(s1)
    assert blocked <= bound, (blocked, bound)
    assert whole > bound, (whole, bound)
