"""The hand-built geometries shared by tests/test_nearest_resample_host.py and tests/test_gpu_nearest_resample.py.  A case
is a dict: ``src_lat``, ``src_lon``, ``dst_lat``, ``dst_lon`` (flat, degrees) and optionally ``src_mask``, ``voxels`` (the
voxel grids the device test runs it with beside the default) and ``ties`` (the geometry has exact ties by construction: it
is kept out of the cKDTree comparison, which cannot know the tie rule).  Not collected by pytest."""
import os

import numpy as np

FIX = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "ref_fixtures")
BRUTE_TILE = 1024  # NB_TILE of marex_nearest.hip


def sphere_points(n, seed):
    """``n`` points uniform on the sphere: ``(lat, lon)`` in degrees, lon in -180 .. 180."""
    g = np.random.default_rng(seed)
    return np.degrees(np.arcsin(g.uniform(-1.0, 1.0, n))), g.uniform(-180.0, 180.0, n)


def grid(ny, nx, lon0=-180.0):
    """Cell centres of a regular ``ny x nx`` grid as 1-D ``(lat, lon)``; ``lon0`` is its western edge."""
    return -90.0 + (np.arange(ny) + 0.5) * (180.0 / ny), lon0 + (np.arange(nx) + 0.5) * (360.0 / nx)


def fixture_mesh():
    """``(lat, lon)`` of the 405 cells of the reference's unstructured fixture."""
    from marex_amd import zarr_io

    p = os.path.join(FIX, "extremes_unstructured.zarr")
    return zarr_io.read_array(os.path.join(p, "lat")).astype(np.float64), zarr_io.read_array(os.path.join(p, "lon")).astype(np.float64)


def case(src, dst, **kw):
    return dict(src_lat=np.asarray(src[0], np.float64), src_lon=np.asarray(src[1], np.float64), dst_lat=np.asarray(dst[0], np.float64),
                dst_lon=np.asarray(dst[1], np.float64), **kw)


def cases():
    """name -> case."""
    c = {}
    c["one_source_one_target"] = case(([10.0], [20.0]), ([-30.0], [-100.0]))
    for M in (63, 64, 65, 257):  # a wave, a wave and a lane, more than one block
        c[f"targets_{M}"] = case(sphere_points(40, 1), sphere_points(M, 100 + M))
    for N in (BRUTE_TILE - 1, BRUTE_TILE, BRUTE_TILE + 1):  # one below, at and one above the brute kernel's LDS tile
        c[f"sources_{N}"] = case(sphere_points(N, N), sphere_points(130, 7))
    # duplicates: cells 3 and 1 are the same point, so are 4 and 2; the lowest cell number wins
    c["duplicate_sources"] = case(([50.0, 10.0, -20.0, 10.0, -20.0], [0.0, 30.0, 60.0, 30.0, 60.0]),
                                  ([10.5, -20.5, 10.0], [30.5, 59.0, 30.0]), ties=True)
    # a target exactly between two sources: x and z of both are equal, y differs in sign only
    c["between_two"] = case(([0.0, 0.0], [1.0, -1.0]), ([0.0], [0.0]), ties=True)
    c["between_two_swapped"] = case(([0.0, 0.0], [-1.0, 1.0]), ([0.0], [0.0]), ties=True)
    ring = np.arange(0.0, 360.0, 30.0)
    c["poles_above_a_ring"] = case((np.full(ring.size, 60.0), ring), ([90.0, -90.0], [0.0, 123.0]), ties=True)
    c["poles_above_a_southern_ring"] = case((np.full(ring.size, -45.0), ring), ([90.0, -90.0], [77.0, 0.0]), ties=True)
    c["date_line"] = case(([0.0, 0.0, 0.0], [0.0, 179.9, -179.9]), ([0.0, 0.0, 0.05, -0.05], [180.0, -180.0, 179.95, -179.95]), ties=True)
    s = sphere_points(300, 21)
    d = sphere_points(200, 22)
    c["conventions_0_360_source"] = case((s[0], np.mod(s[1], 360.0)), d)
    c["conventions_0_360_target"] = case(s, (d[0], np.mod(d[1], 360.0)))
    c["one_voxel"] = case(sphere_points(90, 31), sphere_points(70, 32), voxels=(1,))
    # voxels=2: the faces are the coordinate planes; sources with z = 0 exactly (the equator), x = 0 and y = 0
    c["on_the_voxel_face"] = case(([0.0, 0.0, 0.0, 0.0, 45.0, -45.0, 30.0], [0.0, 90.0, 180.0, -90.0, 90.0, 0.0, 45.0]),
                                  ([0.1, -0.1, 0.0, 44.0, -1.0, 1.0, 89.0], [1.0, 1.0, 91.0, 89.0, 179.0, -91.0, 10.0]), voxels=(2,))
    c["sparse_in_a_fine_grid"] = case(sphere_points(50, 41), sphere_points(150, 42), voxels=(64,))
    # the mask removes every cell of the targets' hemisphere
    s = sphere_points(400, 51)
    d = sphere_points(100, 52)
    d = (np.abs(d[0]), d[1])
    c["mask_removes_the_near_cells"] = case(s, d, src_mask=s[0] < -10.0)
    c["one_cell_on_the_far_side"] = case((np.r_[sphere_points(30, 61)[0], -80.0], np.r_[sphere_points(30, 61)[1], 10.0]),
                                         ([80.0, 75.0, 60.0], [-170.0, 170.0, 180.0]), src_mask=np.r_[np.zeros(30, bool), True])
    c["non_finite"] = case(([10.0, np.nan, 20.0, 30.0, 40.0], [0.0, 5.0, np.inf, 10.0, np.nan]),
                           ([20.0, np.nan, 30.0, 10.0], [1.0, 0.0, -np.inf, np.nan]))
    return c


def voxel_grids(cs, n_eligible):
    """The voxel grids a case is searched with: its own and the default of its size."""
    from marex_amd.resample import default_voxels

    return tuple(sorted(set(cs.get("voxels", ())) | {default_voxels(n_eligible), 3}))
