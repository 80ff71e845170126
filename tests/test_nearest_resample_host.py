"""``marex_amd.nearest_cell_index`` and ``marex_amd.resample_nearest`` without a GPU: the brute-force oracle of
tests/nearest_oracle.py against ``scipy.spatial.cKDTree``, the public path over the NumPy stand-in of
tests/nearest_host_engine.py (validation, rectilinear expansion, masks, ``max_distance_km``, windows, labels, residency),
every refusal, and the engine calls against a recording stub of the library."""
import os
import sys

import numpy as np
import pytest
import torch

import marex_amd
from marex_amd import _stream as ms
from marex_amd import resample as rs
from marex_amd import zarr_io
from marex_amd.engine import HotPath
from marex_amd.exceptions import ConfigurationError, DataValidationError, ProcessingError, TrackingError
from marex_amd.xr_compat import DataArray

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import nearest_cases as nc  # noqa: E402
import nearest_oracle as no  # noqa: E402
from nearest_host_engine import HostEngine  # noqa: E402

#: the bound the project uses for float64 finishes; eight separately rounded float64 operations are far inside it
REL = 1e-12


# ------------------------------------------------------------------ the oracle against cKDTree
def against_tree(src_lat, src_lon, dst_lat, dst_lon):
    """The oracle's ``sqrt(q)`` against the tree's distance, and its index wherever the tree's runner-up is farther than
    the bound; returns the share of targets the second comparison leaves out."""
    from scipy.spatial import cKDTree

    s, d = no.unit_vectors(src_lat, src_lon), no.unit_vectors(dst_lat, dst_lon)
    index, q = no.brute(s, None, d)
    k = min(2, s.shape[1])
    dist, near = cKDTree(s.T).query(d.T, k=k, workers=1)
    dist, near = dist.reshape(d.shape[1], k), near.reshape(d.shape[1], k)
    assert (index >= 0).all()
    assert (np.abs(np.sqrt(q) - dist[:, 0]) <= REL * dist[:, 0]).all()
    clear = np.ones(d.shape[1], bool) if k == 1 else dist[:, 1] > dist[:, 0] * (1.0 + REL)
    assert np.array_equal(index[clear], near[clear, 0])
    return 1.0 - clear.mean()


def test_oracle_against_ckdtree_on_random_geometries():
    for n_src, n_dst, seed in ((1, 50, 1), (2, 50, 2), (700, 3000, 3), (5000, 4000, 4)):
        left_out = against_tree(*nc.sphere_points(n_src, seed), *nc.sphere_points(n_dst, 1000 + seed))
        assert left_out <= 0.01, (n_src, left_out)  # the comparison cannot pass by skipping everything
    # the hand-built geometries without exact ties by construction
    for name, cs in nc.cases().items():
        if cs.get("ties") or "src_mask" in cs or name == "non_finite":
            continue
        assert against_tree(cs["src_lat"], cs["src_lon"], cs["dst_lat"], cs["dst_lon"]) <= 0.01, name


def test_oracle_against_ckdtree_from_the_fixture_mesh_to_a_one_degree_grid():
    lat, lon = nc.fixture_mesh()
    assert lat.shape == (405,)
    # the grid that covers the mesh's patch, cell centres at half degrees
    gl = np.arange(np.floor(lat.min()), np.ceil(lat.max())) + 0.5
    go = np.arange(np.floor(lon.min()), np.ceil(lon.max())) + 0.5
    assert against_tree(lat, lon, *no.expand(gl, go)) <= 0.01


def test_ties_are_ties_and_the_lowest_cell_wins():
    cs = nc.cases()
    for name, want in (("between_two", [0]), ("between_two_swapped", [0]), ("duplicate_sources", [1, 2, 1])):
        c = cs[name]
        s, d = no.unit_vectors(c["src_lat"], c["src_lon"]), no.unit_vectors(c["dst_lat"], c["dst_lon"])
        index, q = no.brute(s, None, d)
        assert index.tolist() == want, name
        # ... although another cell has exactly the same q
        qq = ((s[0][:, None] - d[0][None]) ** 2 + (s[1][:, None] - d[1][None]) ** 2) + (s[2][:, None] - d[2][None]) ** 2
        assert ((qq == q[None]).sum(axis=0) >= 2).all(), name
    # cell numbers that are not ascending: the lowest NUMBER wins, not the first position
    s, d = no.unit_vectors([0.0, 0.0, 5.0], [1.0, -1.0, 0.0]), no.unit_vectors([0.0], [0.0])
    assert no.brute(s, np.array([7, 3, 5]), d)[0].tolist() == [3]


def test_unit_vectors_are_the_oracles_bytes():
    lat, lon = nc.sphere_points(500, 9)
    lat[3], lon[4], lon[5] = np.nan, np.inf, np.nan
    assert rs.unit_vectors(lat, lon).tobytes() == no.unit_vectors(lat, lon).tobytes()
    gl, go = nc.grid(6, 11, lon0=0.0)
    assert rs.unit_vectors(gl[:, None], go[None, :]).reshape(3, -1).tobytes() == no.unit_vectors(*no.expand(gl, go)).tobytes()
    assert rs.default_voxels(1) == 1 and rs.default_voxels(2_100_000) == 296 and rs.default_voxels(10 ** 9) == 1024
    assert rs.search_limit(None, 6371.0) == np.inf and rs.search_limit(6371.0 * np.pi, 6371.0) == np.inf
    # q above the limit always fails the host's distance test, q of the distance itself does not
    for km in (1.0, 55.5, 1000.0, 9000.0, 19000.0):
        lim = rs.search_limit(km, 6371.0)
        assert no.distance_km(np.nextafter(lim, np.inf)) > km and lim > (2 * np.sin(km / (2 * 6371.0))) ** 2


# ------------------------------------------------------------------ the public path over the stand-in
@pytest.fixture
def host_engine(monkeypatch):
    import marex_amd.detect as det

    eng = HostEngine()
    monkeypatch.setattr(det, "get_engine", lambda device=0: eng)
    monkeypatch.setattr(ms, "_free_bytes", lambda e: 1 << 30)
    return eng


def _no_gpu(monkeypatch):
    import marex_amd.detect as det

    def no_gpu(*a, **k):
        raise AssertionError("the validation touched the GPU engine")

    monkeypatch.setattr(det, "get_engine", no_gpu)


def test_every_case_through_the_public_path(host_engine):
    for name, cs in nc.cases().items():
        ds = marex_amd.nearest_cell_index(cs["src_lat"], cs["src_lon"], cs["dst_lat"], cs["dst_lon"], src_mask=cs.get("src_mask"))
        index, dist, _ = no.nearest(cs["src_lat"], cs["src_lon"], cs["dst_lat"], cs["dst_lon"], cs.get("src_mask"))
        assert ds["index"].values.dtype == np.int32 and np.array_equal(ds["index"].values, index), name
        assert ds["distance_km"].values.dtype == np.float64 and np.array_equal(ds["distance_km"].values, dist, equal_nan=True), name
        assert ds.attrs["n_source"] == cs["src_lat"].size and ds.attrs["source_shape"] == (cs["src_lat"].size,)
        assert ds["index"].dims == ("cells",) and np.array_equal(ds["index"].coords["lat"].values, cs["dst_lat"], equal_nan=True)
    ds = marex_amd.nearest_cell_index(**{k: v for k, v in nc.cases()["non_finite"].items()})
    assert ds["index"].values.tolist() == [0, -1, -1, -1] and np.isnan(ds["distance_km"].values[1:]).all()
    # the engine saw the eligible cells only, with their numbers
    assert host_engine.calls[-1][-2:] == (2, 4)


def test_mesh_grid_and_conventions(host_engine):
    lat, lon = nc.fixture_mesh()
    gl, go = nc.grid(18, 36, lon0=0.0)  # 0 .. 360 against the mesh's own convention
    mesh_lat = DataArray(lat, dims=("ncells",), coords={"ncells": ("ncells", np.arange(405))})
    mesh_lon = DataArray(lon, dims=("ncells",))
    # mesh -> rectilinear grid
    ds = marex_amd.nearest_cell_index(mesh_lat, mesh_lon, DataArray(gl, dims=("latitude",)), go, dst_rectilinear=True, method="voxel", voxels=7)
    want, dist, _ = no.nearest(lat, lon, *no.expand(gl, go))
    assert ds["index"].shape == (18, 36) and ds["index"].dims == ("latitude", "lon") and np.array_equal(ds["index"].values.reshape(-1), want)
    assert np.array_equal(ds["index"].coords["latitude"].values, gl) and np.array_equal(ds["index"].coords["lon"].values, go)
    assert ds.attrs["method"] == "voxel" and ds.attrs["voxels"] == 7 and ds.attrs["radius_km"] == 6371.0 and ds.attrs["fallback_targets"] == 0
    assert host_engine.calls[-1][:4] == ("nearest_index", "voxel", 7, 7)
    # the same targets in -180 .. 180: the same index
    ds2 = marex_amd.nearest_cell_index(lat, lon, gl, np.where(go > 180, go - 360, go), dst_rectilinear=True, method="brute")
    assert np.array_equal(ds2["index"].values, ds["index"].values) and ds2.attrs["voxels"] == 0 and ds2.attrs["method"] == "brute"
    # grid -> mesh, with the source's C order; another radius scales the distances
    ds = marex_amd.nearest_cell_index(gl, go, mesh_lat, mesh_lon, src_rectilinear=True, radius_km=1.0)
    want, dist, _ = no.nearest(*no.expand(gl, go), lat, lon, radius_km=1.0)
    assert ds["index"].dims == ("ncells",) and np.array_equal(ds["index"].values, want) and np.array_equal(ds["distance_km"].values, dist)
    assert ds.attrs["n_source"] == 18 * 36 and ds.attrs["source_shape"] == (18, 36) and "ncells" in ds["index"].coords
    assert ds.attrs["method"] == "brute"  # auto: few source cells
    # grid -> grid and a curvilinear source [y, x] with a 2-D mask
    la2, lo2 = (a.reshape(18, 36) for a in no.expand(gl, go))
    ocean = la2 < 30.0
    fl, fo = nc.grid(9, 12)
    ds = marex_amd.nearest_cell_index(la2, lo2, fl, fo, src_mask=ocean, dst_rectilinear=True)
    want, _, _ = no.nearest(la2, lo2, *no.expand(fl, fo), src_mask=ocean)
    assert np.array_equal(ds["index"].values.reshape(-1), want) and ocean.reshape(-1)[want].all() and ds["index"].dims == ("lat", "lon")
    # auto: the brute kernel below AUTO_BRUTE_SOURCES eligible cells, whatever the targets; the voxel search from there on
    n = rs.AUTO_BRUTE_SOURCES
    s_lat, s_lon = nc.sphere_points(n + 1, 11)
    keep = np.ones(n + 1, bool)
    for mask, used in ((None, "voxel"), (np.r_[keep[:-2], False, False], "brute"), (np.r_[keep[:-1], False], "voxel")):
        ds = marex_amd.nearest_cell_index(s_lat, s_lon, np.zeros(3), np.arange(3.0), src_mask=mask)
        ne = n + 1 if mask is None else int(mask.sum())
        assert ds.attrs["method"] == used and host_engine.calls[-1][:4] == (
            "nearest_index", used, rs.default_voxels(ne) if used == "voxel" else 0, rs.default_max_rings(rs.default_voxels(ne)))


def test_max_distance_is_the_hosts_comparison(host_engine):
    # two targets on the equator, 1 and 2 degrees from the only source
    src = ([0.0], [0.0])
    dist = no.nearest(*src, [0.0, 0.0], [1.0, 2.0])[1]
    ds = marex_amd.nearest_cell_index(*src, [0.0, 0.0], [1.0, 2.0], max_distance_km=dist[0])  # exactly at the limit: kept
    assert ds["index"].values.tolist() == [0, -1] and ds["distance_km"].values[0] == dist[0] and np.isnan(ds["distance_km"].values[1])
    ds = marex_amd.nearest_cell_index(*src, [0.0, 0.0], [1.0, 2.0], max_distance_km=np.nextafter(dist[0], 0))  # just outside
    assert ds["index"].values.tolist() == [-1, -1]
    ds = marex_amd.nearest_cell_index(*src, [0.0, 0.0], [1.0, 2.0], max_distance_km=np.nextafter(dist[1], np.inf))
    assert ds["index"].values.tolist() == [0, 0]
    assert host_engine.calls[-1][4] == rs.search_limit(np.nextafter(dist[1], np.inf), 6371.0) < np.inf


def _fields(T, C, seed=0):
    g = np.random.default_rng(seed)
    return {"uint8": g.integers(0, 4, (T, C)).astype(np.uint8), "bool": g.random((T, C)) < 0.4, "int32": g.integers(-5, 2**31 - 1, (T, C)).astype(np.int32),
            "int64": g.integers(0, 2**31 - 1, (T, C)).astype(np.int64), "float32": g.normal(size=(T, C)).astype(np.float32)}


def test_resample_through_the_stand_in(host_engine):
    T, C, M = 7, 11, 13
    index = np.random.default_rng(1).integers(-1, C, M).astype(np.int64)
    index[:3] = (-1, C - 1, 0)
    for name, f in _fields(T, C).items():
        out = marex_amd.resample_nearest(f, index)
        want_dt = np.int32 if name == "int64" else f.dtype
        fill = np.nan if name == "float32" else 0
        assert out.values.dtype == want_dt and out.shape == (T, M) and out.dims == ("time", "cells"), name
        assert np.array_equal(out.values, no.gather(f, index, fill).astype(want_dt), equal_nan=True), name
        # windows of every length, host and resident: the same bytes
        for B in (1, 2, 3, T, None):
            host_engine.calls.clear()
            for resident in (False, True):
                o = marex_amd.resample_nearest(torch.from_numpy(f) if resident else f, index, block_steps=B)
                assert (type(o.data).__module__.startswith("torch")) == resident
                o = o.data.numpy() if resident else o.values
                assert o.dtype == want_dt and o.tobytes() == np.asarray(out.values).tobytes(), (name, B, resident)
            steps = [c[1] for c in host_engine.calls if c[0] == "resample_nearest"]
            assert steps == 2 * [min(B or T, T - a) for a in range(0, T, B or T)]
    # an explicit fill
    assert (marex_amd.resample_nearest(_fields(T, C)["float32"], index, fill=-9.5).values[:, 0] == -9.5).all()
    assert (marex_amd.resample_nearest(_fields(T, C)["int32"], index, fill=-7).values[:, 0] == -7).all()
    assert marex_amd.resample_nearest(_fields(T, C)["bool"], index, fill=True).values[:, 0].all()
    assert (marex_amd.resample_nearest(_fields(T, C)["uint8"], index, fill=255).values[:, 0] == 255).all()


def test_resample_carries_time_and_the_targets_labels(host_engine):
    lat, lon = nc.fixture_mesh()
    gl, go = nc.grid(6, 8)
    ds = marex_amd.nearest_cell_index(lat, lon, DataArray(gl, dims=("lat",)), DataArray(go, dims=("lon",)), dst_rectilinear=True, max_distance_km=4000.0)
    assert (ds["index"].values < 0).any() and (ds["index"].values >= 0).any()
    tv = np.datetime64("2001-01-01") + np.arange(5).astype("timedelta64[D]")
    f = DataArray(_fields(5, 405)["bool"], dims=("time", "ncells"), coords={"time": ("time", tv), "lat": ("ncells", lat)})
    for index in (ds, ds["index"]):
        out = marex_amd.resample_nearest(f, index)
        assert out.dims == ("time", "lat", "lon") and out.shape == (5, 6, 8) and out.values.dtype == np.bool_
        assert np.array_equal(out.coords["time"].values, tv) and np.array_equal(out.coords["lat"].values, gl) and np.array_equal(out.coords["lon"].values, go)
        assert np.array_equal(out.values.reshape(5, -1), no.gather(f.values, ds["index"].values, False))
    # a (time, y, x) source and a plain index array: n_source is taken from the field
    g = _fields(3, 12)["int32"].reshape(3, 3, 4)
    out = marex_amd.resample_nearest(g, np.array([[11, -1], [0, 5]]), fill=-1)
    assert out.dims == ("time", "y", "x") and out.values.tolist() == [[[r[2, 3], -1], [r[0, 0], r[1, 1]]] for r in g]
    # empty sides need no device
    assert marex_amd.resample_nearest(np.zeros((0, 4), np.float32), np.array([1, 2])).shape == (0, 2)
    assert marex_amd.resample_nearest(np.zeros((3, 4), np.uint8), np.zeros(0, np.int32)).shape == (3, 0)
    for f, index, shape in ((torch.zeros((0, 4)), np.array([1, 2]), (0, 2)), (torch.zeros((3, 4), dtype=torch.bool), np.zeros(0, np.int32), (3, 0)),
                            (torch.zeros((3, 0), dtype=torch.int32), np.array([-1, -1]), (3, 2))):  # resident in, resident out
        o = marex_amd.resample_nearest(f, index, fill=None if f.dtype != torch.int32 else 4)
        assert isinstance(o.data, torch.Tensor) and o.data.dtype == f.dtype and tuple(o.shape) == shape and (o.data == 4).all()


def test_refusals_come_before_the_device(monkeypatch):
    _no_gpu(monkeypatch)
    V, Cf = DataValidationError, ConfigurationError
    ok = dict(src_lat=[0.0, 1.0], src_lon=[0.0, 1.0], dst_lat=[0.5], dst_lon=[0.5])
    for kw, err, msg in [(dict(src_lat=[0.0, 90.5]), V, "src_lat must lie in -90 .. 90"), (dict(dst_lat=[-91.0]), V, "dst_lat must lie in"),
                         (dict(src_mask=[False, False]), V, "no eligible source cell"), (dict(src_lat=[np.nan, 0.0], src_mask=[True, False]), V, "no eligible"),
                         (dict(src_lat=[np.nan, np.nan]), V, "no eligible source cell"), (dict(src_mask=[True]), V, "src_mask must be a bool array"),
                         (dict(src_mask=[1, 0]), V, "src_mask must be a bool array"), (dict(src_lon=[0.0]), V, "one common shape"),
                         (dict(src_rectilinear=True, src_lat=np.zeros((2, 2))), V, "needs a 1-D"), (dict(dst_lat=["a"]), V, "must be numbers"),
                         (dict(voxels=0), Cf, "voxels must be a positive integer"), (dict(voxels=2.0), Cf, "voxels must be"),
                         (dict(voxels=True), Cf, "voxels must be"), (dict(voxels=1025), Cf, "voxels must be"), (dict(voxels=-3), Cf, "voxels must be"),
                         (dict(method="kdtree"), Cf, "method must be 'auto', 'voxel' or 'brute'"), (dict(method=None), Cf, "method must be"),
                         (dict(max_distance_km=0), Cf, "max_distance_km must be a finite number above 0"),
                         (dict(max_distance_km=np.nan), Cf, "max_distance_km must be"), (dict(radius_km=-1.0), Cf, "radius_km must be")]:
        with pytest.raises(err, match=msg):
            marex_amd.nearest_cell_index(**{**ok, **kw})
    f = np.zeros((3, 5), np.uint8)
    for field, index, kw, err, msg in [
            (f, np.array([0.0, 1.0]), {}, V, "index must be an integer array"), (f, np.array([True, False]), {}, V, "index must be an integer"),
            (f, np.array([0, 5]), {}, V, "index values must lie in -1 .. n_source - 1"), (f, np.array([-2, 0]), {}, V, "index values must lie"),
            (f, np.array(3), {}, V, "at least one dimension"), (np.zeros((3, 5)), np.array([0]), {}, V, "a float field must be float32"),
            (np.zeros((3, 5), np.complex64), np.array([0]), {}, V, "field must be a mask"), (np.zeros(5, np.uint8), np.array([0]), {}, V, "field must be"),
            (np.full((2, 2), -1, np.int64), np.array([0]), {}, V, "non-negative"), (np.full((2, 2), 2**31, np.int64), np.array([0]), {}, V, "fit int32"),
            (f, np.array([0]), dict(fill=256), Cf, "fill of this field must be an integer in 0 .. 255"), (f, np.array([0]), dict(fill=0.5), Cf, "fill of this"),
            (f > 0, np.array([0]), dict(fill=2), Cf, "integer in 0 .. 1"), (f.astype(np.int32), np.array([0]), dict(fill=2**31), Cf, "fill of this"),
            (f.astype(np.float32), np.array([0]), dict(fill="x"), Cf, "fill of a float field"), (f, np.array([0]), dict(block_steps=0), Cf, "block_steps")]:
        with pytest.raises(err, match=msg):
            if "non-negative" in msg or "fit int32" in msg:  # the range check of the ID windows sits behind the engine
                import marex_amd.detect as det

                monkeypatch.setattr(det, "get_engine", lambda device=0: HostEngine())
                monkeypatch.setattr(ms, "_free_bytes", lambda e: 1 << 30)
            marex_amd.resample_nearest(field, index, **kw)
    _no_gpu(monkeypatch)
    # an index made for another source
    eng = HostEngine()
    import marex_amd.detect as det

    monkeypatch.setattr(det, "get_engine", lambda device=0: eng)
    ds = marex_amd.nearest_cell_index([0.0, 1.0, 2.0], [0.0, 1.0, 2.0], [0.5], [0.5])
    _no_gpu(monkeypatch)
    with pytest.raises(V, match="the index was made for another source geometry"):
        marex_amd.resample_nearest(np.zeros((2, 4), np.uint8), ds)


def test_the_output_must_fit(monkeypatch):
    import marex_amd.detect as det

    eng = HostEngine()
    monkeypatch.setattr(det, "get_engine", lambda device=0: eng)
    T, C, M = 6, 10, 40
    f, index = np.zeros((T, C), np.float32), np.zeros(M, np.int32)
    monkeypatch.setattr(ms, "_free_bytes", lambda e: 4 * T * M + 4 * M + 4 * C * T - 1)
    with pytest.raises(TrackingError, match="resample_nearest: needs"):
        marex_amd.resample_nearest(f, index)
    assert marex_amd.resample_nearest(f, index, block_steps="auto").shape == (T, M)


# ------------------------------------------------------------------ the engine calls against a recording stub
class _Ctx:
    handle = object()

    def __init__(self, log):
        self.log = log

    def check(self, rc, what):
        self.log.append(("check", rc, what))


class _Lib:
    def __init__(self, log):
        self.log = log

    def __getattr__(self, name):
        if not name.startswith("marex_"):
            raise AttributeError(name)

        def fn(*args):
            self.log.append((name, args))
            return 0

        return fn


def _engine():
    log = []
    hot = HotPath.__new__(HotPath)
    hot.device = torch.device("cpu")
    hot.ctx, hot.lib = _Ctx(log), _Lib(log)
    hot._bind_stream = lambda: None
    hot._check_fits = lambda nbytes, what, details: log.append(("fits", nbytes))
    hot._dev = lambda a, dtype=None: torch.from_numpy(np.ascontiguousarray(a if dtype is None else a.astype(dtype)))
    return hot, log


def test_engine_calls_hand_the_library_what_the_header_declares():
    hot, log = _engine()
    N, M = 5, 9
    src, dst, ids = torch.zeros((3, N), dtype=torch.float64), torch.zeros((3, M), dtype=torch.float64), torch.arange(N, dtype=torch.int32)
    index, q = hot.nearest_brute(src, ids, dst)
    assert log[0] == ("marex_nearest_brute_f64", (hot.ctx.handle, src.data_ptr(), ids.data_ptr(), N, dst.data_ptr(), M, None, M, index.data_ptr(), q.data_ptr()))
    assert index.dtype == torch.int32 and q.dtype == torch.float64 and tuple(index.shape) == tuple(q.shape) == (M,)
    sel = torch.tensor([2, 4], dtype=torch.int32)
    hot.nearest_brute(src, None, dst, sel=sel, index=index, q=q)
    assert log[-2][1] == (hot.ctx.handle, src.data_ptr(), None, N, dst.data_ptr(), M, sel.data_ptr(), 2, index.data_ptr(), q.data_ptr())
    log.clear()
    tab = hot.voxel_table(src, ids, 3)
    count = [e for e in log if e[0] == "marex_voxel_count_f64"][0][1]
    scat = [e for e in log if e[0] == "marex_voxel_scatter_f64"][0][1]
    assert count[:4] == (hot.ctx.handle, src.data_ptr(), N, 3) and ("fits", 16 * 27 + 28 * N) in log
    assert scat == (hot.ctx.handle, src.data_ptr(), ids.data_ptr(), N, 3, tab["off"].data_ptr(), count[4], tab["sorted"].data_ptr(), tab["ids"].data_ptr())
    assert tuple(tab["off"].shape) == (28,) and tab["off"].dtype == torch.int32 and tuple(tab["sorted"].shape) == (3, N) and tab["n"] == 3
    index, q, flag = hot.nearest_voxel(tab, dst, 2, 0.25)
    assert log[-2][1] == (hot.ctx.handle, tab["sorted"].data_ptr(), tab["ids"].data_ptr(), N, tab["off"].data_ptr(), 3, dst.data_ptr(), M, 2, 0.25,
                          index.data_ptr(), q.data_ptr(), flag.data_ptr()) and flag.dtype == torch.uint8
    # the stub leaves the flags as they are: mark two targets, and the brute kernel runs over exactly those
    log.clear()
    hot._buf = lambda wsp, name, shape, dtype, device: (torch.tensor([0, 1, 0, 0, 1, 0, 0, 0, 0], dtype=dtype) if name == "nn_flag"
                                                      else torch.zeros(shape, dtype=dtype))
    r = hot.nearest_index(src.numpy(), ids.numpy(), dst.numpy(), method="voxel", voxels=2, max_rings=1)
    last = [e for e in log if e[0] == "marex_nearest_brute_f64"][0][1]
    assert r["fallback"] == 2 and r["voxels"] == 2 and last[7] == 2 and last[6] is not None and r["index"].dtype == np.int32 and r["q"].shape == (M,)
    assert [e for e in log if e[0] == "marex_nearest_voxel_f64"][0][1][8] == 1
    assert hot.nearest_index(src, None, dst)["voxels"] == 0
    log.clear()
    for dt, name, fill in ((torch.uint8, "marex_resample_nearest_u8", 7), (torch.int32, "marex_resample_nearest_i32", -3), (torch.float32, "marex_resample_nearest_f32", 1.5)):
        x, out, ix = torch.zeros((4, N), dtype=dt), torch.zeros((6, M), dtype=dt), torch.zeros(M, dtype=torch.int32)
        hot.resample_nearest(x[1:3], ix, out[2:4], fill)
        assert log[-2] == (name, (hot.ctx.handle, x[1:3].data_ptr(), 2, N, ix.data_ptr(), M, fill, out[2:4].data_ptr()))


def test_engine_refusals():
    hot, log = _engine()
    P = ProcessingError
    src, dst = torch.zeros((3, 5), dtype=torch.float64), torch.zeros((3, 9), dtype=torch.float64)
    for f, msg in [(lambda: hot.nearest_brute(src.float(), None, dst), "the sources must be a contiguous, non-empty float64"),
                   (lambda: hot.nearest_brute(src, None, dst.T), "the targets must be"), (lambda: hot.nearest_brute(np.zeros((2, 5)), None, dst), "float64 \\[3, N\\] unit vectors"),
                   (lambda: hot.nearest_brute(src[:, :0], None, dst), "non-empty"), (lambda: hot.nearest_brute(src, torch.zeros(4, dtype=torch.int32), dst), "the cell numbers must be"),
                   (lambda: hot.nearest_brute(src, None, dst, sel=torch.zeros(2, dtype=torch.int32)), "a target list needs"),
                   (lambda: hot.nearest_brute(src, None, dst, sel=torch.zeros(0, dtype=torch.int32), index=torch.zeros(9, dtype=torch.int32), q=torch.zeros(9, dtype=torch.float64)), "a target list needs"),
                   (lambda: hot.voxel_table(src, None, 0), "1 .. 1024 voxels per axis"), (lambda: hot.voxel_table(src, None, 1025), "voxels per axis"),
                   (lambda: hot.voxel_table(src, None, 2.0), "voxels per axis"), (lambda: hot.nearest_voxel(hot.voxel_table(src, None, 2), dst, -1), "must not be negative"),
                   (lambda: hot.nearest_voxel(hot.voxel_table(src, None, 2), dst, 1, float("nan")), "must not be negative"),
                   (lambda: hot.nearest_index(src, None, dst, method="auto"), "the method is 'brute' or 'voxel'"),
                   (lambda: hot.resample_nearest(torch.zeros((2, 5), dtype=torch.float64), torch.zeros(3, dtype=torch.int32), torch.zeros((2, 3), dtype=torch.float64), 0), "the field must be"),
                   (lambda: hot.resample_nearest(torch.zeros((2, 5)), torch.zeros(3, dtype=torch.int64), torch.zeros((2, 3)), 0), "the index must be an int32"),
                   (lambda: hot.resample_nearest(torch.zeros((2, 5)), torch.zeros(3, dtype=torch.int32), torch.zeros((2, 4)), 0), "the output must be"),
                   (lambda: hot.resample_nearest(torch.zeros((2, 5)), torch.zeros(3, dtype=torch.int32), torch.zeros((3, 2)).T, 0), "the output must be"),
                   (lambda: hot.resample_nearest(torch.zeros((2, 5), dtype=torch.uint8), torch.zeros(3, dtype=torch.int32), torch.zeros((2, 3), dtype=torch.uint8), 256), "the fill of a")]:
        with pytest.raises(P, match=msg):
            f()
    assert not [e for e in log if e[0].startswith("marex_nearest") or e[0].startswith("marex_resample")]
