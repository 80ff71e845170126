"""GPU parity at the launch edges of the gridded fill, the time closing and the mesh sweeps (csrc/marex_morphology.hip):
the cases of tests/track_pre_cases.py -- each named for the edge it reaches, proven there by
tests/test_track_pre_cases_host.py -- against the distance form of the fill, the run-length rule of the closing and the
oracle.  Boolean outputs, compared as the bytes the kernels write (0 / 1, nothing left of the 0xCD the fixture puts into
fresh buffers): bit-exact."""
import functools
import os
import sys

import numpy as np
import pytest
import torch

from oracle import marex_oracle as orc

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import track_pre_cases as tc  # noqa: E402

pytestmark = pytest.mark.gpu

GUARD = 0xA5


def _dev(hot, a):
    return torch.from_numpy(np.ascontiguousarray(a).astype(np.uint8)).to(hot.device)


def _offset_view(hot, t, offset=1):
    """The same bytes as ``t`` in a view ``offset`` bytes into a larger buffer: ``(view, buffer)``; the rest of the buffer
    holds GUARD."""
    n = t.numel()
    buf = torch.full((n + 32,), GUARD, dtype=torch.uint8, device=hot.device)
    v = buf[offset:offset + n].view(t.shape)
    v.copy_(t)
    assert v.is_contiguous() and v.data_ptr() % 8 == (buf.data_ptr() + offset) % 8 and buf.data_ptr() % 16 == 0
    return v, buf


def _guards_intact(buf, offset, n):
    b = buf.cpu().numpy()
    return (b[:offset] == GUARD).all() and (b[offset + n:] == GUARD).all()


def _where(got, exp):
    bad = np.argwhere(got != exp)
    return f"{bad.shape[0]} bytes differ, first at {bad[0].tolist()}: got {got[tuple(bad[0])]}, expected {exp[tuple(bad[0])]}"


# ------------------------------------------------------------------------------------------------------------------------
# fill
# ------------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _fill_expected(name):
    """uint8 ``[T, ny * nx]``.  The distance form (equal to the oracle wherever the oracle is affordable, shown on the
    host); the oracle itself for the long series, where it is the faster of the two."""
    c = tc.fill_case(name)
    x, mask = tc.fill_inputs(name)
    exp = orc.fill_holes(x, mask, c.R, c.regional) if c.kind == "rows" else tc.fill_holes_distance(x, mask, c.R, c.regional)
    exp = exp.reshape(c.T, -1).astype(np.uint8)
    exp.setflags(write=False)
    return exp


def _run_fill(hot, c, x, mask, **kw):
    got = hot.fill_holes(x, mask, c.ny, c.nx, c.R, c.regional, **kw)
    hot.sync()
    return got


@pytest.mark.parametrize("name", [c.name for c in tc.fill_cases()])
def test_fill_case_matches_the_reference(hot, name):
    c = tc.fill_case(name)
    x, mask = tc.fill_inputs(name)
    got = _run_fill(hot, c, _dev(hot, x.reshape(c.T, -1)), _dev(hot, mask.reshape(-1))).cpu().numpy()
    exp = _fill_expected(name)
    assert np.array_equal(got, exp), (name, tc.fill_geometry(c.T, c.ny, c.nx, c.R), _where(got, exp))


def test_fill_refuses_a_radius_of_64_and_launches_nothing(hot):
    c = tc.fill_case("nxp128-R2-periodic")
    x, mask = tc.fill_inputs(c.name)
    out = torch.full((c.T * c.ny * c.nx,), GUARD, dtype=torch.uint8, device=hot.device)
    with pytest.raises(Exception, match=r"R_fill must be in 0\.\.63"):
        hot.fill_holes(_dev(hot, x.reshape(c.T, -1)), _dev(hot, mask.reshape(-1)), c.ny, c.nx, 64, c.regional, wsp={"filled": out})
    hot.sync()
    assert (out.cpu().numpy() == GUARD).all()
    # the same workspace at the limit: written in full
    ok = hot.fill_holes(_dev(hot, x.reshape(c.T, -1)), _dev(hot, mask.reshape(-1)), c.ny, c.nx, 63, c.regional, wsp={"filled": out})
    hot.sync()
    assert ok.data_ptr() == out.data_ptr()
    assert np.array_equal(ok.cpu().numpy(), tc.fill_holes_distance(x, mask, 63, c.regional).reshape(c.T, -1).astype(np.uint8))


OFFSET_SHAPE = (3, 5, 72, 2)  # nx % 8 == 0: the 8-byte path of k_morph_unpack for aligned pointers; nxp = 80, two words


@pytest.mark.parametrize("which", ["mask", "out", "data", "mask+out"])
@pytest.mark.parametrize("regional", [False, True])
def test_fill_through_views_at_a_byte_offset(hot, which, regional):
    """A 2-D mask, an output or a field that is a view one byte into a larger buffer is a valid argument (contiguous, on
    the device): the 8-byte loads and stores of k_morph_unpack are taken only for 8-byte aligned ``mask`` and ``out``,
    the byte path otherwise, with the same bytes and nothing written outside the view."""
    T, ny, nx, R = OFFSET_SHAPE
    rng = np.random.default_rng(72)
    x = rng.random((T, ny, nx)) < 0.4
    mask = rng.random((ny, nx)) < 0.8
    exp = tc.fill_holes_distance(x, mask, R, regional).reshape(T, -1).astype(np.uint8)
    xd, md = _dev(hot, x.reshape(T, -1)), _dev(hot, mask)  # mask stays 2-D
    aligned = hot.fill_holes(xd, md, ny, nx, R, regional)
    hot.sync()
    assert aligned.data_ptr() % 8 == 0 and md.data_ptr() % 8 == 0
    assert np.array_equal(aligned.cpu().numpy(), exp)
    n = T * ny * nx
    wsp, bufs = None, []
    if "mask" in which:
        md, b = _offset_view(hot, md)
        assert md.data_ptr() % 8 == 1 and md.shape == (ny, nx)
        bufs.append((b, ny * nx))
    if "data" in which:
        xd, b = _offset_view(hot, xd)
        bufs.append((b, n))
    if "out" in which:
        ob = torch.full((n + 32,), GUARD, dtype=torch.uint8, device=hot.device)
        wsp = {"filled": ob[1:]}
        bufs.append((ob, n))
    got = hot.fill_holes(xd, md, ny, nx, R, regional, wsp=wsp)
    hot.sync()
    if "out" in which:
        assert got.data_ptr() % 8 == 1 and got.data_ptr() == ob.data_ptr() + 1
    assert np.array_equal(got.cpu().numpy(), exp) and torch.equal(got, aligned)
    for b, m in bufs:
        assert _guards_intact(b, 1, m)


# ------------------------------------------------------------------------------------------------------------------------
# time closing
# ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("T,T_fill", tc.closing_cases())
def test_time_closing_matches_the_run_length_rule(hot, T, T_fill):
    wide = tc.closing_field(T, tc.CLOSING_C_MAX, T_fill)
    exp_wide = tc.time_closing_runs(wide, T_fill).astype(np.uint8)
    for C in tc.CLOSING_C_WIDE + tc.CLOSING_C_SCALAR:
        x = tc.closing_field(T, C, T_fill)
        exp = np.ascontiguousarray(exp_wide[:, :C])
        xd = _dev(hot, x)
        got = hot.time_closing(xd, T_fill)
        hot.sync()
        kernel = tc.closing_geometry(T, C, T_fill, aligned=xd.data_ptr() % 16 == 0 and got.data_ptr() % 16 == 0)[0]
        assert kernel == ("wide" if C % 16 == 0 else "scalar")
        g = got.cpu().numpy()
        assert np.array_equal(g, exp), (T, T_fill, C, kernel, _where(g, exp))
        if C % 16 == 0:  # the same field one byte into a larger buffer, then the output too: the scalar kernel, the same bytes
            xv, xb = _offset_view(hot, xd)
            assert xv.data_ptr() % 16 == 1
            got_v = hot.time_closing(xv, T_fill)
            ob = torch.full((T * C + 32,), GUARD, dtype=torch.uint8, device=hot.device)
            got_o = hot.time_closing(xd, T_fill, wsp={"time_closed": ob[1:]})
            hot.sync()
            assert got_o.data_ptr() == ob.data_ptr() + 1
            assert torch.equal(got_v, got) and torch.equal(got_o, got), (T, T_fill, C)
            assert _guards_intact(xb, 1, T * C) and _guards_intact(ob, 1, T * C)


def test_fill_time_gaps_chain_over_three_time_blocks(hot):
    c = tc.CHAINED
    x, mask = tc.chained_field()
    exp = orc.fill_time_gaps(x, mask, c.R_fill, c.T_fill).reshape(c.T, -1).astype(np.uint8)
    got = hot.fill_time_gaps(_dev(hot, x.reshape(c.T, -1)), _dev(hot, mask.reshape(-1)), c.ny, c.nx, c.R_fill, c.T_fill)
    hot.sync()
    g = got.cpu().numpy()
    assert np.array_equal(g, exp), _where(g, exp)


def test_time_closing_refuses_an_odd_window_and_launches_nothing(hot):
    x = _dev(hot, tc.closing_field(33, 16, 2))
    out = torch.full((33 * 16,), GUARD, dtype=torch.uint8, device=hot.device)
    for bad in (3, -2):
        with pytest.raises(Exception, match="T_fill must be even and >= 0"):
            hot.time_closing(x, bad, wsp={"time_closed": out})
    hot.sync()
    assert (out.cpu().numpy() == GUARD).all()


# ------------------------------------------------------------------------------------------------------------------------
# mesh sweeps
# ------------------------------------------------------------------------------------------------------------------------
def _run_mesh(hot, x, mask, nbr, R, **kw):
    got = hot.fill_holes_mesh(_dev(hot, x), _dev(hot, mask), torch.from_numpy(np.ascontiguousarray(nbr)).to(hot.device), R, **kw)
    hot.sync()
    return got.cpu().numpy()


@pytest.mark.parametrize("R", tc.MESH_R)
def test_mesh_sweeps_match_the_oracle_up_to_the_radius_limit(hot, R):
    x, mask, nbr = tc.mesh_ring()
    exp = orc.fill_holes_mesh(x, mask, nbr, R).astype(np.uint8)
    got = _run_mesh(hot, x, mask, nbr, R)
    assert np.array_equal(got, exp), (R, _where(got, exp))
    # all land: the reference sets land True before its erosions and does not mask again
    land = np.zeros_like(mask)
    got = _run_mesh(hot, x & land[None], land, nbr, R)
    assert np.array_equal(got, orc.fill_holes_mesh(x & land[None], land, nbr, R).astype(np.uint8)), R


@pytest.mark.parametrize("R", [0, 1, 1024])
def test_mesh_of_one_cell(hot, R):
    for nbr in (np.full((3, 1), -1, dtype=np.int32), np.array([[-1], [0], [-1]], dtype=np.int32)):
        for ocean in (True, False):
            x = np.array([[True], [False], [True]])
            mask = np.array([ocean])
            exp = orc.fill_holes_mesh(x, mask, nbr, R).astype(np.uint8)
            assert np.array_equal(_run_mesh(hot, x, mask, nbr, R), exp), (R, nbr.T.tolist(), ocean)


def test_mesh_refuses_a_radius_of_1025_and_launches_nothing(hot):
    x, mask, nbr = tc.mesh_ring()
    out = torch.full((x.size,), GUARD, dtype=torch.uint8, device=hot.device)
    with pytest.raises(Exception, match=r"R_fill must be in 0\.\.1024"):
        _run_mesh(hot, x, mask, nbr, 1025, wsp={"filled_mesh": out})
    hot.sync()
    assert (out.cpu().numpy() == GUARD).all()
