"""GPU parity: the fused rename-and-accumulate pass of the grid tracker's cluster renaming (``marex_event_rename_i32``
through ``HotPath.event_rename``) against the path it replaces -- ``relabel`` on a copy, then the dense
``event_moments`` -- gathered at the compact slots, bit for bit; the span guard; the argument checks."""
import numpy as np
import pytest
import torch

from marex_amd.exceptions import ProcessingError

pytestmark = pytest.mark.gpu

N_EV = 6
#: IDs 0..40 -> events: event 1 split over four IDs, IDs mapped to 0, event 5 without an ID, the table shorter than the largest ID
LUT = np.zeros(33, np.int32)
LUT[[1, 2, 9, 17]], LUT[[3, 4]], LUT[[5, 30, 31, 32]], LUT[[6, 8, 10, 12, 14]], LUT[[20, 21]] = 1, 2, 3, 4, 6

#: (6, 5, 67): 335 cells, no multiple of 64, nx < 200 (both edge flags on the same cells); (6, 3, 231): odd nx for the
#: 2 * x > nx rule, distinct flag bands
SHAPES = [(6, 5, 67), (6, 3, 231)]


def _dev(hot, a):
    return torch.from_numpy(np.array(a, order="C")).to(hot.device)  # np.array copies: the input stays as it is


def _field(T, ny, nx):
    rng = np.random.default_rng(1000 * ny + nx)
    C = ny * nx
    ids = rng.integers(0, 41, (T, C)).astype(np.int32)
    runs = np.repeat(rng.integers(0, 41, (T, (C + 149) // 150)).astype(np.int32), 150, axis=1)[:, :C]
    ids = np.where(rng.random((T, C)) < 0.6, runs, ids)  # runs of 150 cells: across 64-cell pieces and row ends
    ids[rng.random((T, C)) < 0.05] = -3
    ids[:, 40:300] = np.where(ids[:, 40:300] == 3, 4, ids[:, 40:300])
    ids[0, 40:300] = 3                                    # event 2: one run over five pieces and several rows at t = 0 ...
    ids[2][np.isin(ids[2], (3, 4))] = 0                   # ... absent at t = 2, inside its span ...
    ids[5, 7] = 4                                         # ... and back at t = 5
    x = np.arange(C) % nx                                 # event 6 (IDs 20, 21) keeps to one flag band at t = 3, 4, 5
    for t, keep in ((3, x < 100), (4, x >= nx - 100), (5, (x >= 100) & (x < nx - 100))):
        ids[t][np.isin(ids[t], (20, 21)) & ~keep] = 0
    ids[1, :11] = [9, 3, 5, 6, 20, 40, 7, -3, 2, 4, 21]   # every event with an ID, an ID past the table, one mapped to 0
    return ids


def _weights(ny, nx):
    """Multiples of 2^-8 below 2^10: every float64 sum of w, w y, w x over a slice is exact, whatever the order."""
    rng = np.random.default_rng(nx)
    return (rng.integers(1, 2**18, ny * nx) / 256.0).astype(np.float32)


def _spans(ids, lut, n_ev):
    T = ids.shape[0]
    ev = np.where((ids > 0) & (ids < lut.size), lut[np.clip(ids, 0, lut.size - 1)], 0)
    tmin, tmax = np.full(n_ev + 1, 2**31 - 1, np.int64), np.full(n_ev + 1, -1, np.int64)
    for e in range(1, n_ev + 1):
        ts = np.nonzero((ev == e).any(axis=1))[0]
        if ts.size:
            tmin[e], tmax[e] = ts[0], ts[-1]
    assert T > 0
    return ev.astype(np.int32), tmin, tmax


def _expected(hot, ids, ny, nx, lut, n_ev, w):
    """The existing path on a copy: relabel, then the dense event moments with the original IDs next to the renamed ones."""
    ev = _dev(hot, ids)
    ev[ev < 0] = 0        # relabel leaves what has no entry; the rename pass maps it to background
    ev[ev >= lut.size] = 0
    hot.relabel(ev, lut)
    r = hot.event_moments(ev, _dev(hot, ids), ny, nx, n_ev, w)
    return ev.cpu().numpy(), r


def _gather(dense, off, tmin, n_ev):
    """Dense [T, n_ev, ...] values at the compact slots."""
    rows = [dense[tmin[e] + k, e - 1] for e in range(1, n_ev + 1) for k in range(int(off[e + 1] - off[e]))]
    return np.stack(rows) if rows else dense[:0, 0]


@pytest.mark.parametrize("weighted", [False, True], ids=["cells", "weights"])
@pytest.mark.parametrize("shape", SHAPES, ids=["5x67", "3x231"])
def test_rename_pass_equals_relabel_and_dense_moments(hot, shape, weighted):
    T, ny, nx = shape
    ids = _field(T, ny, nx)
    ev_np, tmin, tmax = _spans(ids, LUT, N_EV)
    assert ids.max() >= LUT.size and (ids < 0).any() and tmax[5] < 0 and (tmax[[1, 2, 3, 4, 6]] >= 0).all()
    assert tmin[2] == 0 and tmax[2] == 5 and not (ev_np[2] == 2).any()           # event 2 is absent inside its span
    assert len(np.unique(ids[ev_np == 1])) > 1                                   # event 1 comes from several IDs
    w = _dev(hot, _weights(ny, nx)) if weighted else None
    want_ids, want = _expected(hot, ids, ny, nx, LUT, N_EV, w)
    assert np.array_equal(want_ids, ev_np)
    outs = []
    for _ in range(2):  # a second call on the same input: the same bytes
        d = _dev(hot, ids)
        r = hot.event_rename(d, ny, nx, LUT, tmin, tmax, w)
        off = r["off"]
        assert off.dtype == np.int64 and off.tolist() == np.concatenate([[0], np.cumsum(np.maximum(tmax - tmin + 1, 0) * (tmax >= 0))]).tolist()
        assert np.array_equal(d.cpu().numpy(), want_ids)
        assert r["mom"].dtype == np.int64 and r["mom"].shape == (off[-1], 5)
        assert np.array_equal(r["mom"], _gather(want["mom"], off, tmin, N_EV))
        assert r["gid"].dtype == np.int32 and np.array_equal(r["gid"], _gather(want["gid"], off, tmin, N_EV))
        s2 = int(off[2]) + 2  # event 2's slot at t = 2 stays zero
        assert (r["mom"][s2] == 0).all() and r["gid"][s2] == 0
        if weighted:
            assert r["wmom"].dtype == np.float64 and np.array_equal(r["wmom"], _gather(want["wmom"], off, tmin, N_EV))
            assert (r["wmom"][s2] == 0).all() and (r["wmom"][:, 0] > 0).sum() == (r["gid"] > 0).sum()
        else:
            assert "wmom" not in r
        outs.append(tuple(r[k].tobytes() for k in sorted(r)) + (d.cpu().numpy().tobytes(),))
    assert outs[0] == outs[1]
    # what is not in the compact slots is zero in the dense tables: nothing was lost
    assert r["mom"][:, 0].sum() == want["mom"][..., 0].sum() == (ev_np > 0).sum()
    # the flags: both bands on the same cells when nx < 200, distinct bands otherwise
    fl = r["mom"][:, 4]
    assert set(np.unique(fl[r["gid"] > 0]).tolist()) <= ({3} if nx < 200 else {0, 1, 2, 3})
    if nx >= 200:  # event 6 alone in the left band, in the right band and between them
        assert [int(fl[off[6] + t - tmin[6]]) for t in (3, 4, 5)] == [1, 2, 0] and (r["gid"][off[6] + 3 - tmin[6]:][:3] > 0).all()


def test_one_event_and_a_table_of_one_entry(hot):
    T, ny, nx = SHAPES[0]
    ids = _field(T, ny, nx)
    one = (LUT > 0).astype(np.int32)
    ev_np, tmin, tmax = _spans(ids, one, 1)
    want_ids, want = _expected(hot, ids, ny, nx, one, 1, None)
    d = _dev(hot, ids)
    r = hot.event_rename(d, ny, nx, one, tmin, tmax)
    assert np.array_equal(d.cpu().numpy(), want_ids) and np.array_equal(r["mom"], want["mom"][:, 0])
    assert np.array_equal(r["gid"], want["gid"][:, 0])
    # no event has a step: everything becomes background, no slot
    d = _dev(hot, ids)
    r = hot.event_rename(d, ny, nx, np.zeros(1, np.int32), [0, 0], [-1, -1])
    assert not d.cpu().numpy().any() and r["mom"].shape == (0, 5) and r["gid"].shape == (0,) and r["off"].tolist() == [0, 0, 0]


def test_a_cell_outside_its_events_span_is_counted_not_accumulated(hot):
    """Event 1's span is declared one step short and event 2's slots follow it: a missing guard would add event 1's
    last step to event 2's first slot -- inside the allocation, so nothing can fault."""
    T, ny, nx = SHAPES[0]
    ids = _field(T, ny, nx)
    ev_np, tmin, tmax = _spans(ids, LUT, N_EV)
    assert tmax[1] == T - 1 and tmin[2] == 0
    good = hot.event_rename(_dev(hot, ids), ny, nx, LUT, tmin, tmax)
    short = tmax.copy()
    short[1] -= 1
    d = _dev(hot, ids)
    with pytest.raises(ProcessingError, match=rf"event_rename: {int((ev_np[T - 1] == 1).sum())} cells belong to an event outside"):
        hot.event_rename(d, ny, nx, LUT, tmin, short)
    assert np.array_equal(d.cpu().numpy(), ev_np)  # renamed all the same
    # the same through the library, on buffers of the test's own: event 2's slots hold what they held with the right spans
    length = np.maximum(short - tmin + 1, 0) * (short >= 0)
    off = np.concatenate([[0], np.cumsum(length)]).astype(np.int64)
    n_slots = int(off[-1])
    acc = torch.full((n_slots, 5), -1, dtype=torch.int64, device=hot.device)
    gid = torch.full((n_slots,), -1, dtype=torch.int32, device=hot.device)
    status = torch.full((1,), -1, dtype=torch.int64, device=hot.device)
    d = _dev(hot, ids)
    hot.call("marex_event_rename_i32", d, T, ny, nx, _dev(hot, LUT), LUT.size, N_EV, _dev(hot, tmin.astype(np.int32)),
             _dev(hot, off), n_slots, None, acc, None, gid, status)
    assert int(status.item()) == (ev_np[T - 1] == 1).sum() > 0
    acc, gid = acc.cpu().numpy(), gid.cpu().numpy()
    assert off[2] == good["off"][2] - 1
    assert np.array_equal(acc[off[2]:], good["mom"][good["off"][2]:]) and np.array_equal(gid[off[2]:], good["gid"][good["off"][2]:])
    assert np.array_equal(acc[:off[2]], good["mom"][:off[2]])
    # a span that starts late: the earlier steps are counted
    late = tmin.copy()
    late[1] += 1
    with pytest.raises(ProcessingError, match=rf"event_rename: {int((ev_np[0] == 1).sum())} cells"):
        hot.event_rename(_dev(hot, ids), ny, nx, LUT, late, tmax)


def test_rename_checks_its_arguments_before_the_launch(hot):
    T, ny, nx = SHAPES[0]
    ids = _field(T, ny, nx)
    _, tmin, tmax = _spans(ids, LUT, N_EV)
    d = _dev(hot, ids)
    for bad in (lambda: hot.event_rename(d, ny, nx, LUT, tmin[:-1], tmax[:-1]),             # the table names event 6
                lambda: hot.event_rename(d, ny, nx, LUT.astype(np.int64), tmin, tmax),
                lambda: hot.event_rename(d, ny, nx + 1, LUT, tmin, tmax),
                lambda: hot.event_rename(d.to(torch.int64), ny, nx, LUT, tmin, tmax),
                lambda: hot.event_rename(d, ny, nx, LUT[:0], tmin, tmax),
                lambda: hot.event_rename(d, ny, nx, LUT, tmin, tmax[:-1])):
        with pytest.raises(ProcessingError):
            bad()
    assert np.array_equal(d.cpu().numpy(), ids)  # nothing was written
    lut_d, tm_d = _dev(hot, LUT), _dev(hot, np.zeros(N_EV + 1, np.int32))
    off_d = _dev(hot, np.arange(N_EV + 2, dtype=np.int64))
    acc = torch.zeros((N_EV + 1, 5), dtype=torch.int64, device=hot.device)
    gid = torch.zeros(N_EV + 1, dtype=torch.int32, device=hot.device)
    st = torch.zeros(1, dtype=torch.int64, device=hot.device)
    w = torch.ones(ny * nx, dtype=torch.float32, device=hot.device)
    ok = (d, T, ny, nx, lut_d, LUT.size, N_EV, tm_d, off_d, N_EV + 1, None, acc, None, gid, st)

    def with_(**kw):
        names = ("ids", "T", "ny", "nx", "lut", "lut_len", "n_ev", "ev_tmin", "ev_off", "n_slots", "w", "acc", "wacc", "gid", "status")
        return tuple(kw.get(k, v) for k, v in zip(names, ok))

    cases = [(-4, with_(T=2**31 - 1)), (-4, with_(ny=1, nx=2**31 - 1)), (-4, with_(ny=2**16, nx=2**15)),
             (-1, with_(T=0)), (-1, with_(nx=0)), (-1, with_(n_ev=0)), (-1, with_(lut_len=0)), (-1, with_(n_slots=0)),
             (-1, with_(w=w))]                                                            # weights without their accumulator
    cases += [(-1, with_(**{k: None})) for k in ("ids", "lut", "ev_tmin", "ev_off", "acc", "gid", "status")]
    for code, args in cases:  # refused by the library before any launch
        with pytest.raises(ProcessingError, match=rf"marex_event_rename_i32 failed \(code {code}\)"):
            hot.call("marex_event_rename_i32", *args)
    assert np.array_equal(d.cpu().numpy(), ids) and not acc.any() and not gid.any() and not st.any()
