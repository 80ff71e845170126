"""GPU: labelling in time blocks with the seams stitched on the device (``HotPath.label_objects_3d(..., max_block_cells=)``,
``tracker(..., label_block_steps=)``) gives, bit for bit, what one labelling call over the whole field gives -- on seeded
fields, on hand-built seam cases, through the tracker, and on a field of 2^31 cells and more that one call cannot take."""
import os
import sys

import numpy as np
import pytest
import torch

import marex_amd
import marex_amd.track as trk_mod
from marex_amd.engine import HotPath
from marex_amd.exceptions import TrackingError
from marex_amd.xr_compat import DataArray

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import label_blocks_oracle as lbo  # noqa: E402
from test_track_host import REFERENCE_ROWS, load_fixture  # noqa: E402

pytestmark = pytest.mark.gpu

NEW_ENTRIES = ("marex_label_seam_union_i32", "marex_label_table_resolve_i32", "marex_label_apply_table_i32")


def _dev(hot, x):
    T = x.shape[0]
    return torch.from_numpy(np.ascontiguousarray(x).reshape(T, -1).astype(np.uint8)).to(hot.device)


def _label(hot, xd, ny, nx, wrap, connect_t, block_steps=None):
    assert HotPath.POISON  # fresh buffers start as 0xCD bytes (tests/conftest.py)
    r = hot.label_objects_3d(xd, ny, nx, wrap_x=wrap, connect_t=connect_t,
                             max_block_cells=None if block_steps is None else block_steps * ny * nx)
    hot.sync()
    n = int(r["n"].item())
    return r["ids"], n, r["areas"][:n]


def _check_all_block_lengths(hot, x, wrap, connect_t, what, lengths=None):
    T, ny, nx = x.shape
    xd = _dev(hot, x)
    exp, n_exp = lbo.label_whole(x, wrap, connect_t)
    ids0, n0, areas0 = _label(hot, xd, ny, nx, wrap, connect_t)
    assert n0 == n_exp, (what, n0, n_exp)
    assert np.array_equal(ids0.cpu().numpy().reshape(T, ny, nx), exp), what
    assert areas0.dtype == torch.int32
    for b in lengths or sorted({b for b in (1, 2, 3, 7, T - 1, T) if b >= 1}):
        ids, n, areas = _label(hot, xd, ny, nx, wrap, connect_t, b)
        assert n == n0, (what, b, n, n0)
        assert ids.dtype == torch.int32 and torch.equal(ids, ids0), (what, b)
        assert areas.dtype == torch.int64 and tuple(areas.shape) == (n,), (what, b)
        assert torch.equal(areas, areas0.to(torch.int64)), (what, b)
        assert np.array_equal(ids.cpu().numpy().reshape(T, ny, nx), exp), (what, b)
    return n0


FUZZ_SHAPES = [(9, 12, 16), (12, 7, 70), (10, 1, 150), (8, 30, 1), (11, 25, 2), (16, 33, 130), (9, 64, 64), (20, 19, 257)]


@pytest.mark.parametrize("seed", range(8))
def test_forced_blocks_equal_the_single_call(hot, seed):
    """8 seeds x (3 densities x 2 x 2 blobby + 2 noise) = 112 fields, each with blocks of 1, 2, 3, 7, T - 1 and T steps."""
    rng = np.random.default_rng(7000 + seed)
    shape = FUZZ_SHAPES[seed]
    k = 0
    for dens in (0.03, 0.2, 0.55):
        x = lbo.blobby(rng, shape, dens)
        for wrap in (True, False):
            for connect_t in (True, False):
                _check_all_block_lengths(hot, x, wrap, connect_t, (shape, dens, wrap, connect_t))
                k += 1
    for dens in (0.3, 0.9):  # salt and pepper: many small objects and many distinct pairs per wave on every seam
        x = rng.random(shape) < dens
        _check_all_block_lengths(hot, x, bool(seed & 1), True, (shape, "noise", dens))
        k += 1
    assert k == 14


def test_hand_built_seam_cases(hot):
    cases = lbo.seam_cases()
    assert len(cases) >= 50
    for name, x, wrap, n_exp in cases:
        n = _check_all_block_lengths(hot, x, wrap, True, name)
        if n_exp is not None:
            assert n == n_exp, name


def test_hand_built_seam_cases_on_a_wide_grid(hot):
    """The same contacts where a row spans several waves and workgroups (nx = 300): diagonals through the x seam, two events
    joined only through the neighbouring block, and a field of all ones -- one union address under the heaviest load."""
    T, ny, nx = 9, 5, 300
    for t in range(T - 1):
        for wrap in (True, False):
            x = np.zeros((T, ny, nx), bool)
            x[t, 3, nx - 1] = x[t + 1, 4, 0] = True
            x[t, 1, 0] = x[t + 1, 0, nx - 1] = True
            x[t, 2, 100] = x[t + 1, 3, 101] = True
            n = _check_all_block_lengths(hot, x, wrap, True, ("wide diagonal", t, wrap))
            assert n == (3 if wrap else 5)
    for t in range(1, T - 1):
        x = np.zeros((T, ny, nx), bool)
        x[:t + 1, 2, 10] = x[:t + 1, 2, 250] = True
        x[t + 1, 2, 10:251] = True
        x[0, 4, 3] = x[t, 4, 200] = x[t + 1, 4, 5] = x[T - 1, 0, 0] = True
        assert _check_all_block_lengths(hot, x, False, True, ("wide bar later", t)) == 5
        x = np.zeros((T, ny, nx), bool)
        x[t, 2, 10:251] = True
        x[t + 1:, 2, 10] = x[t + 1:, 2, 250] = True
        x[0, 4, 3] = x[t, 4, 200] = x[t + 1, 4, 5] = x[T - 1, 0, 0] = True
        assert _check_all_block_lengths(hot, x, False, True, ("wide bar earlier", t)) == 5
    for wrap in (True, False):
        assert _check_all_block_lengths(hot, np.ones((T, 40, nx), bool), wrap, True, ("wide ones", wrap)) == 1


def test_a_small_field_takes_one_call_and_none_of_the_new_entry_points(hot, monkeypatch):
    rng = np.random.default_rng(3)
    x = lbo.blobby(rng, (6, 20, 30), 0.2)
    xd = _dev(hot, x)
    calls = []
    real = HotPath.call

    def counting(self, name, *args):
        calls.append(name)
        return real(self, name, *args)

    monkeypatch.setattr(HotPath, "call", counting)
    r = hot.label_objects_3d(xd, 20, 30)
    assert calls == ["marex_label3d_i32"]
    assert r["areas"].dtype == torch.int32 and r["areas"].numel() == x.size and r["ids"].dtype == torch.int32
    calls.clear()
    hot.label_objects_3d(xd, 20, 30, max_block_cells=2 * 600)
    assert calls.count("marex_label3d_i32") == 3 and calls.count(NEW_ENTRIES[0]) == 2
    assert calls.count(NEW_ENTRIES[1]) == 1 and calls.count(NEW_ENTRIES[2]) == 3
    calls.clear()
    hot.label_objects_3d(xd, 20, 30, connect_t=False, max_block_cells=2 * 600)
    assert calls.count(NEW_ENTRIES[0]) == 0 and calls.count(NEW_ENTRIES[1]) == 1


def test_refusals_come_before_any_kernel(hot, monkeypatch):
    xd = torch.zeros((4, 600), dtype=torch.uint8, device=hot.device)
    monkeypatch.setattr(HotPath, "call", lambda *a, **k: (_ for _ in ()).throw(AssertionError("a kernel was reached")))
    with pytest.raises(TrackingError, match="one timestep of 600 cells exceeds the labelling block of 599 cells"):
        hot.label_objects_3d(xd, 20, 30, max_block_cells=599)
    with pytest.raises(TrackingError, match="max_block_cells must be positive"):
        hot.label_objects_3d(xd, 20, 30, max_block_cells=0)


def test_entry_points_check_their_arguments(hot):
    from marex_amd.exceptions import ProcessingError

    ids = torch.zeros((2, 12), dtype=torch.int32, device=hot.device)
    table = torch.arange(5, dtype=torch.int32, device=hot.device)
    a32 = torch.ones(4, dtype=torch.int32, device=hot.device)
    a64 = torch.zeros(4, dtype=torch.int64, device=hot.device)
    n = torch.zeros(1, dtype=torch.int32, device=hot.device)
    bad = [("marex_label_seam_union_i32", (None, ids[1], 3, 4, 1, 0, 2, 2, 2, table, 5)),
           ("marex_label_seam_union_i32", (ids[0], ids[1], 0, 4, 1, 0, 2, 2, 2, table, 5)),
           ("marex_label_seam_union_i32", (ids[0], ids[1], 3, 4, 1, 0, 2, 2, 3, table, 5)),   # 2 + 3 reaches table_len
           ("marex_label_seam_union_i32", (ids[0], ids[1], 3, 4, 1, -1, 2, 2, 2, table, 5)),
           ("marex_label_table_resolve_i32", (table, 0, a32, a64, n)),
           ("marex_label_table_resolve_i32", (table, 4, None, a64, n)),
           ("marex_label_table_resolve_i32", (table, 2**31 - 1, a32, a64, n)),
           ("marex_label_apply_table_i32", (ids, 0, table, 5, 0)),
           ("marex_label_apply_table_i32", (ids, 24, table, 5, 5)),
           ("marex_label_apply_table_i32", (ids, 2**31 - 1, table, 5, 0)),
           ("marex_label_apply_table_i32", (ids, 24, None, 5, 0))]
    for name, args in bad:
        with pytest.raises(ProcessingError, match=name):
            hot.call(name, *args)
    hot.sync()
    assert torch.equal(table.cpu(), torch.arange(5, dtype=torch.int32)) and int(ids.abs().sum().item()) == 0


def test_apply_pass_on_unaligned_slices(hot):
    """The 16-byte body of the apply pass with every head / tail length: slices that start 0..3 elements past a 16-byte
    boundary and hold 1..40 elements; IDs the table does not cover become background."""
    rng = np.random.default_rng(9)
    base = torch.from_numpy(rng.integers(0, 7, 64).astype(np.int32)).to(hot.device)
    table = torch.from_numpy(np.array([0, 11, 12, 13, 14, 15, 16, 17, 18, 19], np.int32)).to(hot.device)
    tab = table.cpu().numpy()
    for start in range(4):
        for n in range(1, 41):
            buf = base.clone()
            hot.call("marex_label_apply_table_i32", buf[start:start + n], n, table, 8, 3)  # entries 8 and 9 are out of reach
            exp = base.cpu().numpy().copy()
            v = exp[start:start + n]
            exp[start:start + n] = np.where((v > 0) & (v + 3 < 8), tab[np.minimum(v + 3, 9)], 0)
            assert np.array_equal(buf.cpu().numpy(), exp), (start, n)


def _run(capsys, *args, **kw):
    ds = marex_amd.tracker(*args, **kw).run()
    return ds, capsys.readouterr().out


def _same_run(a, b):
    (da, oa), (db, ob) = a, b
    va, vb = da["ID_field"].values, db["ID_field"].values
    assert va.dtype == vb.dtype == np.int32 and np.array_equal(va, vb)
    assert da.attrs == db.attrs and list(da.attrs) == list(db.attrs)
    assert oa == ob and "Total Events Tracked" in oa


@pytest.mark.parametrize("params", [REFERENCE_ROWS[0][0], REFERENCE_ROWS[3][0], REFERENCE_ROWS[4][0]])
def test_tracker_with_forced_blocks_on_the_reference_fixture(hot, capsys, monkeypatch, params):
    R, Tf, q, poles = params
    ev, mask, lat, lon, tm = load_fixture(poles)
    da = DataArray(ev, dims=("time", "lat", "lon"), coords={"time": tm, "lat": lat, "lon": lon}, attrs={"source": "fixture"})
    mk = DataArray(mask, dims=("lat", "lon"))
    kw = dict(R_fill=R, T_fill=Tf, area_filter_quartile=q, allow_merging=False, quiet=True)
    base = _run(capsys, da, mk, **kw)
    for k in (1, 3, 7, ev.shape[0] - 1, ev.shape[0]):
        _same_run(_run(capsys, da, mk, label_block_steps=k, **kw), base)
    monkeypatch.setattr(trk_mod, "PINNED_ID_FIELD_BYTES", 0)  # the ID field through the pinned staging buffers
    _same_run(_run(capsys, da, mk, label_block_steps=2, **kw), base)
    _same_run(_run(capsys, da, mk, **kw), base)


def _synthetic_coords(T, ny, nx):
    return {"time": np.arange(T), "lat": np.linspace(-70, 70, ny), "lon": np.linspace(0, 360, nx, endpoint=False)}


def _synthetic():
    rng = np.random.default_rng(77)
    T, ny, nx = 14, 48, 96
    ev = lbo.blobby(rng, (T, ny, nx), 0.15)
    mask = np.ones((ny, nx), bool)
    mask[:3] = False
    mask[20:24, 30:40] = False
    da = DataArray(ev, dims=("time", "lat", "lon"), coords=_synthetic_coords(T, ny, nx))
    return ev, mask, da, DataArray(mask, dims=("lat", "lon"))


@pytest.mark.parametrize("regional", [False, True])
def test_tracker_with_forced_blocks_on_a_synthetic_field(hot, capsys, regional):
    ev, mask, da, mk = _synthetic()
    kw = dict(R_fill=2, T_fill=2, area_filter_quartile=0.4, allow_merging=False, regional_mode=regional)
    base = _run(capsys, da, mk, **kw)
    assert base[0].attrs["N_events_final"] > 3
    for k in (1, 2, 5, 13, 14, 100):
        _same_run(_run(capsys, da, mk, label_block_steps=k, **kw), base)


@pytest.mark.parametrize("time_connectivity", [True, False])
def test_identify_objects_with_forced_blocks(hot, time_connectivity):
    ev, mask, da, mk = _synthetic()
    x = ev & mask
    xa = DataArray(x, dims=("time", "lat", "lon"), coords=_synthetic_coords(*x.shape))
    exp, n_exp = lbo.label_whole(x, True, time_connectivity)
    ids0, none, n0 = marex_amd.tracker(da, mk, R_fill=2, allow_merging=False).identify_objects(xa, time_connectivity)
    assert none is None and n0 == n_exp and np.array_equal(ids0.values, exp)
    for k in (1, 3, 13):
        ids, _, n = marex_amd.tracker(da, mk, R_fill=2, allow_merging=False, label_block_steps=k).identify_objects(
            xa, time_connectivity)
        assert n == n0 and ids.values.dtype == np.int32 and np.array_equal(ids.values, ids0.values)


def test_not_enough_device_memory_is_a_tracking_error_with_both_numbers(hot, monkeypatch):
    ev, mask, da, mk = _synthetic()
    monkeypatch.setattr(torch.cuda, "mem_get_info", lambda *a, **k: (1000, 2000))
    monkeypatch.setattr(torch.cuda, "memory_reserved", lambda *a, **k: 0)
    monkeypatch.setattr(torch.cuda, "memory_allocated", lambda *a, **k: 0)
    t = marex_amd.tracker(da, mk, R_fill=2, allow_merging=False)
    need = sum(trk_mod.tracking_memory_need(14, 48, 96, 2, 2).values())
    with pytest.raises(TrackingError, match=rf"tracker.run: needs {need / 1e9:.3f} GB of device memory, 0.000 GB are free"):
        t.run()
    with pytest.raises(TrackingError, match="identify_objects: needs"):
        t.identify_objects(da, True)


def test_a_field_of_2_31_cells_is_labelled_in_two_blocks(hot):
    """2 072 steps of 720 x 1440 = 2 148 249 600 cells >= 2^31, on device tensors only: a 7-step pattern F (slice 0 empty,
    slices 1-6 blobs connected through time) repeated 296 times.  The default plan is 2 071 + 1 steps, so the one seam lies
    between pattern steps 5 and 6 of the last repetition and the result is right only if it is stitched.  One call cannot
    take this field: without the blocked path ``marex_label3d_i32`` refuses it."""
    from marex_amd.engine import plan_time_blocks

    ny, nx, reps = 720, 1440, 296
    C = ny * nx
    T = 7 * reps
    assert T * C >= 2**31 and plan_time_blocks(T, C) == [(0, T - 1), (T - 1, T)]
    rng = np.random.default_rng(2072)
    F = np.zeros((7, ny, nx), bool)
    F[1:] = lbo.blobby(rng, (6, ny // 4, nx // 4), 0.05).repeat(4, axis=1).repeat(4, axis=2)
    assert F[5].any() and F[6].any() and (F[5] & F[6]).any()  # events do cross the seam
    Fd = _dev(hot, F)
    Fi, NF, Fa = _label(hot, Fd, ny, nx, True, True)
    exp, n_exp = lbo.label_whole(F, True, True)
    assert NF == n_exp and NF > 10 and np.array_equal(Fi.cpu().numpy().reshape(7, ny, nx), exp)
    crossing = np.intersect1d(exp[5][exp[5] > 0], exp[6][exp[6] > 0]).size
    assert crossing > 0
    Fi = Fi.clone()
    Fa = Fa.to(torch.int64).clone()
    big = Fd.repeat(reps, 1)
    assert tuple(big.shape) == (T, C)
    r = hot.label_objects_3d(big, ny, nx)
    hot.sync()
    n = int(r["n"].item())
    print(f"\n2^31 field: {T} x {ny} x {nx}, N_F = {NF}, {crossing} events of F cross the seam, n = {n} (expected {reps * NF})")
    assert n == reps * NF
    ids = r["ids"]
    assert ids.dtype == torch.int32 and tuple(ids.shape) == (T, C)
    zero = torch.zeros((), dtype=torch.int32, device=hot.device)
    for k in range(reps):  # one repetition at a time
        want = torch.where(Fi > 0, Fi + k * NF, zero)
        assert torch.equal(ids[7 * k:7 * k + 7], want), f"repetition {k}"
    assert r["areas"].dtype == torch.int64 and torch.equal(r["areas"], Fa.repeat(reps))
