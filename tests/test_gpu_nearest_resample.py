"""Nearest-cell resampling on the device (``marex_nearest_brute_f64``, the voxel search, ``marex_resample_nearest_*``):
every index with ``==`` against the brute-force oracle of tests/nearest_oracle.py from both kernels, on the hand-built
geometries of tests/nearest_cases.py, a random mesh and the reference's mesh fixture; every gathered field byte for byte
against NumPy indexing whatever the windows and the residency, one of them past 2^32 bytes; and the composition with
``event_occurrence`` and ``event_matching``."""
import os
import sys

import numpy as np
import pytest
import torch

import marex_amd
from marex_amd import resample as rs
from marex_amd import zarr_io
from marex_amd.exceptions import DataValidationError
from marex_amd.xr_compat import DataArray

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import nearest_cases as nc  # noqa: E402
import nearest_oracle as no  # noqa: E402

pytestmark = pytest.mark.gpu
CASES = nc.cases()
_oracle = {}


def oracle(name):
    """``(src [3, Ne], ids, dst [3, M], index, q)`` of a case, computed once."""
    if name not in _oracle:
        cs = CASES[name]
        s, d = no.unit_vectors(cs["src_lat"], cs["src_lon"]), no.unit_vectors(cs["dst_lat"], cs["dst_lon"])
        ok = ~np.isnan(s).any(axis=0)
        if "src_mask" in cs:
            ok &= cs["src_mask"]
        ids = np.flatnonzero(ok).astype(np.int32)
        src = np.ascontiguousarray(s[:, ok])
        _oracle[name] = (src, ids, d, *no.brute(src, ids, d))
    return _oracle[name]


def equal(r, index, q, what):
    assert r["index"].dtype == np.int32 and r["q"].dtype == np.float64
    assert np.array_equal(r["index"], index), (what, np.flatnonzero(r["index"] != index)[:5], r["index"][:8], index[:8])
    assert np.array_equal(r["q"], q), what  # +inf where there is none


@pytest.mark.parametrize("name", sorted(CASES))
def test_both_kernels_give_the_oracles_index(hot, name):
    src, ids, dst, index, q = oracle(name)
    equal(hot.nearest_index(src, ids, dst, method="brute"), index, q, "brute")
    for n in nc.voxel_grids(CASES[name], ids.size):
        for max_rings in (None, 1):  # rings until the grid is covered; one ring and the brute kernel for the rest
            r = hot.nearest_index(src, ids, dst, method="voxel", voxels=n, max_rings=max_rings)
            equal(r, index, q, ("voxel", n, max_rings))
            assert r["voxels"] == n and (max_rings == 1 or r["fallback"] == 0)
    # the cell numbers need not ascend: the lowest NUMBER wins a tie, wherever it stands in the table
    if ids.size > 1:
        p = np.random.default_rng(5).permutation(ids.size)
        equal(hot.nearest_index(np.ascontiguousarray(src[:, p]), ids[p], dst, method="brute"), index, q, "brute, permuted")
        equal(hot.nearest_index(np.ascontiguousarray(src[:, p]), ids[p], dst, method="voxel", voxels=2), index, q, "voxel, permuted")


def test_rings_run_until_the_grid_is_exhausted(hot):
    src, ids, dst, index, q = oracle("sparse_in_a_fine_grid")
    assert ids.size == 50
    r = hot.nearest_index(src, ids, dst, method="voxel", voxels=64, max_rings=64)
    equal(r, index, q, "64 rings")
    assert r["fallback"] == 0
    few = hot.nearest_index(src, ids, dst, method="voxel", voxels=64, max_rings=2)
    equal(few, index, q, "2 rings")
    assert 0 < few["fallback"] <= dst.shape[1]


def test_the_fallback_runs_for_a_cell_on_the_far_side(hot):
    src, ids, dst, index, q = oracle("one_cell_on_the_far_side")
    assert ids.tolist() == [30] and index.tolist() == [30, 30, 30]
    r = hot.nearest_index(src, ids, dst, method="voxel", voxels=16, max_rings=1)
    equal(r, index, q, "fallback")
    assert r["fallback"] == 3  # every target was still open after ring 1
    flag = hot.nearest_voxel(hot.voxel_table(src, ids, 16), dst, 1)[2]
    assert flag.cpu().numpy().tolist() == [1, 1, 1]
    assert hot.nearest_index(src, ids, dst, method="voxel", voxels=16, max_rings=16)["fallback"] == 0


def test_the_voxel_table_is_a_permutation_in_voxel_order(hot):
    src, ids, dst, index, q = oracle("sources_1025")
    n = 5
    t = hot.voxel_table(src, ids, n)
    off, srt, sid = t["off"].cpu().numpy(), t["sorted"].cpu().numpy(), t["ids"].cpu().numpy()
    v = np.clip(((src + 1.0) * (0.5 * n)).astype(np.int64), 0, n - 1)
    vox = (v[2] * n + v[1]) * n + v[0]
    assert off[0] == 0 and off[-1] == ids.size and np.array_equal(np.diff(off), np.bincount(vox, minlength=n ** 3))
    assert np.array_equal(np.sort(sid), ids) and np.array_equal(srt, src[:, np.searchsorted(ids, sid)])
    assert np.array_equal(vox[np.searchsorted(ids, sid)], np.repeat(np.arange(n ** 3), np.diff(off)))


def public(cs, **kw):
    return marex_amd.nearest_cell_index(cs["src_lat"], cs["src_lon"], cs["dst_lat"], cs["dst_lon"], src_mask=cs.get("src_mask"), **kw)


@pytest.mark.parametrize("method", ["brute", "voxel"])
def test_masks_and_non_finite_coordinates_through_the_public_path(hot, method):
    for name in ("mask_removes_the_near_cells", "non_finite", "one_cell_on_the_far_side", "date_line", "poles_above_a_ring"):
        cs = CASES[name]
        ds = public(cs, method=method)
        index, dist, _ = no.nearest(cs["src_lat"], cs["src_lon"], cs["dst_lat"], cs["dst_lon"], cs.get("src_mask"))
        assert np.array_equal(ds["index"].values, index) and np.array_equal(ds["distance_km"].values, dist, equal_nan=True), name
        assert ds.attrs["method"] == method
    assert public(CASES["non_finite"], method=method)["index"].values.tolist() == [0, -1, -1, -1]
    assert public(CASES["date_line"], method=method)["index"].values.tolist()[2:] == [1, 2]
    # 0 .. 360 on one side against -180 .. 180 on the other: the same index
    a, b = public(CASES["conventions_0_360_source"], method=method), public(CASES["conventions_0_360_target"], method=method)
    assert np.array_equal(a["index"].values, b["index"].values) and (a["index"].values >= 0).all()


@pytest.mark.parametrize("method", ["brute", "voxel"])
def test_max_distance_just_inside_and_just_outside(hot, method):
    src = ([0.0, 0.0], [0.0, 100.0])
    dst = ([0.0, 0.0, 50.0], [1.0, 2.0, -120.0])
    dist = no.nearest(*src, *dst)[1]
    for km, want in ((dist[0], [0, -1, -1]), (np.nextafter(dist[0], 0), [-1, -1, -1]), (np.nextafter(dist[1], 0), [0, -1, -1]), (dist[1], [0, 0, -1])):
        for voxels in (None, 40, 256):  # a fine grid: the search stops at the limit's chord
            ds = marex_amd.nearest_cell_index(*src, *dst, max_distance_km=km, method=method, voxels=voxels)
            index, d, _ = no.nearest(*src, *dst, max_distance_km=km)
            assert ds["index"].values.tolist() == want == index.tolist(), (km, voxels)
            assert np.array_equal(ds["distance_km"].values, d, equal_nan=True)
    # a limit over a random mesh: the device may give up early, the result is the oracle's
    s, g = nc.sphere_points(3000, 71), nc.grid(45, 90)
    ocean = s[0] < 20.0
    ds = marex_amd.nearest_cell_index(*s, *g, src_mask=ocean, dst_rectilinear=True, max_distance_km=700.0, method=method)
    index, d, _ = no.nearest(*s, *no.expand(*g), src_mask=ocean, max_distance_km=700.0)
    assert np.array_equal(ds["index"].values.reshape(-1), index) and np.array_equal(ds["distance_km"].values.reshape(-1), d, equal_nan=True)
    assert (index < 0).any() and (index >= 0).any()


def test_a_random_mesh_to_a_grid_with_every_method(hot):
    s, g = nc.sphere_points(4200, 81), nc.grid(90, 180, lon0=0.0)
    index, dist, _ = no.nearest(*s, *no.expand(*g))
    auto = "voxel" if 4200 >= rs.AUTO_BRUTE_SOURCES else "brute"  # the rule itself: tests/test_nearest_resample_host.py
    for method, used in (("brute", "brute"), ("voxel", "voxel"), ("auto", auto)):
        ds = marex_amd.nearest_cell_index(*s, *g, dst_rectilinear=True, method=method)
        assert ds["index"].shape == (90, 180) and np.array_equal(ds["index"].values.reshape(-1), index), method
        assert np.array_equal(ds["distance_km"].values.reshape(-1), dist) and ds.attrs["method"] == used
        assert ds.attrs["voxels"] == (rs.default_voxels(4200) if used == "voxel" else 0)
    # the reverse direction, a coarser grid -> the mesh
    g = nc.grid(30, 60)
    ds = marex_amd.nearest_cell_index(*g, *s, src_rectilinear=True, method="voxel")
    assert np.array_equal(ds["index"].values, no.nearest(*no.expand(*g), *s)[0]) and ds.attrs["source_shape"] == (30, 60)


_mesh = {}


def mesh_to_grid():
    """The fixture mesh, the 1-degree grid over its patch and the index between them (through the voxel search)."""
    if not _mesh:
        lat, lon = nc.fixture_mesh()
        gl = np.arange(np.floor(lat.min()), np.ceil(lat.max())) + 0.5
        go = np.arange(np.floor(lon.min()), np.ceil(lon.max())) + 0.5
        ds = marex_amd.nearest_cell_index(lat, lon, DataArray(gl, dims=("lat",)), DataArray(go, dims=("lon",)), dst_rectilinear=True,
                                          method="voxel")
        _mesh.update(lat=lat, lon=lon, gl=gl, go=go, ds=ds, want=no.nearest(lat, lon, *no.expand(gl, go)))
    return _mesh


def test_the_fixture_mesh_to_a_one_degree_grid(hot):
    m = mesh_to_grid()
    index, dist, _ = m["want"]
    assert np.array_equal(m["ds"]["index"].values.reshape(-1), index) and np.array_equal(m["ds"]["distance_km"].values.reshape(-1), dist)
    assert m["ds"].attrs["n_source"] == 405 and m["ds"]["index"].dims == ("lat", "lon")
    b = marex_amd.nearest_cell_index(m["lat"], m["lon"], m["gl"], m["go"], dst_rectilinear=True, method="brute")
    assert np.array_equal(b["index"].values, m["ds"]["index"].values)


# ------------------------------------------------------------------ the gather
def fields(T, C, seed=0):
    g = np.random.default_rng(seed)
    return {"uint8": g.integers(0, 256, (T, C)).astype(np.uint8), "bool": g.random((T, C)) < 0.4,
            "int32": g.integers(-2**31, 2**31 - 1, (T, C)).astype(np.int32), "int64": g.integers(0, 2**31 - 1, (T, C)).astype(np.int64),
            "float32": g.normal(size=(T, C)).astype(np.float32)}


def an_index(C, M, seed):
    index = np.random.default_rng(seed).integers(-1, C, M).astype(np.int32)
    index[:3] = (C - 1, -1, 0)[:M]  # the last source cell, none, the first
    return index


@pytest.mark.parametrize("M", [63, 64, 65, 257])
@pytest.mark.parametrize("name", ["uint8", "bool", "int32", "int64", "float32"])
def test_the_gather_is_numpy_indexing(hot, name, M):
    T, C = 19, 37
    f, index = fields(T, C, M)[name], an_index(C, M, M)
    want_dt = np.int32 if name == "int64" else f.dtype
    fills = {"uint8": (None, 255), "bool": (None, True), "int32": (None, -7), "int64": (None, 12), "float32": (None, -1.5)}[name]
    for fill in fills:
        want = no.gather(f, index, (np.nan if name == "float32" else 0) if fill is None else fill).astype(want_dt)
        for resident in (False, True):
            for B in (None, 1, 2, T):
                x = torch.from_numpy(f).to(hot.device) if resident else f
                out = marex_amd.resample_nearest(x, index, fill=fill, block_steps=B)
                assert type(out.data).__module__.startswith("torch") == resident
                got = out.data.cpu().numpy() if resident else out.values
                assert got.dtype == want_dt and got.shape == (T, M) and got.tobytes() == want.tobytes(), (name, M, fill, resident, B)


def test_gather_edges(hot):
    C = 9
    f = fields(1, C, 3)  # T = 1
    for name in ("uint8", "int32", "float32"):
        index = an_index(C, 65, 1)
        assert np.array_equal(marex_amd.resample_nearest(f[name], index).values, no.gather(f[name], index, np.nan if name == "float32" else 0), equal_nan=True)
        none = marex_amd.resample_nearest(f[name], np.full(130, -1), fill=3).values  # an index of all -1
        assert none.shape == (1, 130) and (none == 3).all()
    # the engine call itself: outputs start as 0xCD bytes, rows a multiple of 4 bytes (four cells per lane) and not
    for M in (64, 68, 66, 1028):
        for dt in (np.uint8, np.int32, np.float32):
            T = 21
            x = np.random.default_rng(M).integers(0, 200, (T, C)).astype(dt)
            index = an_index(C, M, M)
            out = torch.empty((T + 2, M), dtype=getattr(torch, np.dtype(dt).name), device=hot.device)
            out.view(torch.uint8).fill_(0xCD)
            hot.resample_nearest(torch.from_numpy(x).to(hot.device), torch.from_numpy(index).to(hot.device), out[1:T + 1], 5)
            got = out.cpu().numpy()
            assert got[1:T + 1].tobytes() == no.gather(x, index, 5).tobytes(), (M, dt)
            assert (got[[0, T + 1]].view(np.uint8) == 0xCD).all()  # and nothing beyond the window's rows
    with pytest.raises(DataValidationError, match="index values must lie"):
        marex_amd.resample_nearest(f["uint8"], np.array([C]))


def test_an_output_past_32_bits_of_bytes(hot):
    T, C, M = 4100, 1024, 1 << 20
    g = torch.Generator(device="cpu").manual_seed(5)
    field = torch.randint(0, 256, (T, C), dtype=torch.uint8, generator=g).to(hot.device)
    index = torch.randint(-1, C, (M,), dtype=torch.int32, generator=g)
    index[-1] = C - 1
    out = marex_amd.resample_nearest(field, index.numpy(), fill=7).data
    assert out.dtype == torch.uint8 and tuple(out.shape) == (T, M) and out.numel() > 2**32 and out.device == hot.device
    idx = index.to(hot.device).long()
    for a in range(0, T, 512):  # compared on the device in row blocks: nothing of that size crosses to the host
        want = torch.where(idx[None, :] >= 0, field[a:a + 512][:, idx.clamp(min=0)], torch.tensor(7, dtype=torch.uint8, device=hot.device))
        assert torch.equal(out[a:a + 512], want), a
    assert int(out[T - 1, M - 1]) == int(field[T - 1, C - 1])
    # the public path walked that field in windows below 2^31 cells; one engine call over all of it takes the kernel's own
    # row offsets past 2^32 bytes
    whole = torch.empty((T, M), dtype=torch.uint8, device=hot.device)
    whole.fill_(0xCD)
    hot.resample_nearest(field, index.to(hot.device), whole, 7)
    assert T * M > 2**32 and torch.equal(whole, out)


# ------------------------------------------------------------------ composition
def test_resampled_fields_go_into_the_other_statistics(hot):
    m = mesh_to_grid()
    p = os.path.join(nc.FIX, "extremes_unstructured.zarr")
    ev = zarr_io.read_array(os.path.join(p, "extreme_events")).astype(bool)
    T = ev.shape[0]
    index = m["want"][0]
    da = DataArray(ev, dims=("time", "ncells"), coords={"time": ("time", np.arange(T))})
    on_grid = marex_amd.resample_nearest(da, m["ds"])
    want = no.gather(ev, index, False).reshape(T, m["gl"].size, m["go"].size)
    assert on_grid.dims == ("time", "lat", "lon") and on_grid.values.dtype == np.bool_ and np.array_equal(on_grid.values, want)
    occ = marex_amd.event_occurrence(on_grid)
    assert np.array_equal(occ["occurrence"].values, want.sum(axis=0)) and tuple(occ["occurrence"].dims) == ("lat", "lon")
    # an ID field and the same field, both resampled (one resident): every pair lies on the diagonal
    ids = (ev * (1 + (np.arange(405)[None, :] % 7) + 7 * (np.arange(T)[:, None] // 25))).astype(np.int32)
    a = marex_amd.resample_nearest(ids, m["ds"])
    b = marex_amd.resample_nearest(torch.from_numpy(ids).to(hot.device), m["ds"]["index"])
    assert np.array_equal(a.values, b.data.cpu().numpy()) and np.array_equal(a.values.reshape(T, -1), no.gather(ids, index, 0))
    mt = marex_amd.event_matching(a, b)
    assert mt["pair_ID_a"].values.size == np.unique(a.values[a.values > 0]).size > 0
    assert np.array_equal(mt["pair_ID_a"].values, mt["pair_ID_b"].values) and (mt["pair_iou"].values == 1.0).all()
