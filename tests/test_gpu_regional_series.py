"""The regional series on the device: ``marex_regional_series_u8`` / ``marex_regional_series_i32`` through
``HotPath.regional_series`` against the NumPy oracle at the edges of the kernel's layout -- integers equal, float64 sums
byte for byte on dyadic inputs and within the derived bound on normal ones -- the cross-checks against the statistics that
exist already, and the public path on a grid and a mesh."""
import os
import sys

import numpy as np
import pytest

import marex_amd
from marex_amd.exceptions import DataValidationError, ProcessingError
from marex_amd.xr_compat import DataArray

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import regional_series_cases as rc  # noqa: E402
import regional_series_oracle as ro  # noqa: E402

pytestmark = pytest.mark.gpu
F = np.float32


def _days(n, start="2003-12-20"):
    return (np.datetime64(start) + np.arange(n)).astype("datetime64[ns]")


# 1, around a piece of one cell per lane, around a piece of four, and -- from the layout the library reports -- one below, at
# and above a wave pass and a workgroup of both layouts, and one vector of four cells below and above those of the
# four-cells-per-lane layout (1023 and 1025 fall to one cell per lane); C % 4 != 0 among them
SHAPES = sorted({1, 63, 64, 65, 255, 257, *rc.layout_edges()})


@pytest.mark.parametrize("C", SHAPES)
def test_every_level_at_the_layout_edges(hot, C):
    rng = np.random.default_rng(C)
    T = 2
    reg, R = rc.region_map("edges" if C > 64 else "mod3", C)
    q = rng.integers(0, 2**40, C).astype(np.int64)
    wf = rc.dyadic_weights(rng, C)
    x = rc.mask_field(rng, T, C)
    anom = rc.spoil(rng, rc.dyadic_anomalies(rng, (T, C)), x)
    thr = rc.thresholds(rng, 3, C)
    doy = np.array([2, 0], np.int32)
    ids = rc.id_field(rng, T, C)
    # the mask alone (four cells per lane where C % 4 == 0), with anomalies, with thresholds (one cell per lane)
    rc.assert_same(rc.run_engine(hot, x, reg, R, q=q), rc.oracle(x, reg, R, q=q))
    rc.assert_same(rc.run_engine(hot, x, reg, R), rc.oracle(x, reg, R))
    rc.assert_same(rc.run_engine(hot, x, reg, R, q=q, wf=wf, anom=anom), rc.oracle(x, reg, R, q=q, wf=wf, anom=anom))
    rc.assert_same(rc.run_engine(hot, x, reg, R, q=q, wf=wf, anom=anom, thr=thr, doy=doy),
                   rc.oracle(x, reg, R, q=q, wf=wf, anom=anom, thr=thr, doy=doy))
    rc.assert_same(rc.run_engine(hot, x.astype(bool), reg, R, anom=anom, thr=thr, doy=doy),
                   rc.oracle(x, reg, R, anom=anom, thr=thr, doy=doy))
    # the ID field
    rc.assert_same(rc.run_engine(hot, ids, reg, R, q=q, wf=wf, anom=anom, thr=thr, doy=doy),
                   rc.oracle(ids, reg, R, q=q, wf=wf, anom=anom, thr=thr, doy=doy))
    rc.assert_same(rc.run_engine(hot, ids, reg, R, q=q, anom=anom, match=3), rc.oracle(ids, reg, R, q=q, anom=anom, match=3))


@pytest.mark.parametrize("T", [1, 2, rc.ROW_STRIDE - 1, rc.ROW_STRIDE, rc.ROW_STRIDE + 1])
def test_rows_around_the_row_stride(hot, T):
    rng = np.random.default_rng(100 + T)
    doy = rng.integers(0, 4, T).astype(np.int32)
    for C, name in ((4100, "one"), (515, "edges")):  # four cells per lane, workgroups of one region; one cell per lane, mixed
        reg, R = rc.region_map(name, C)
        x = rc.mask_field(rng, T, C)
        anom = rc.spoil(rng, rc.dyadic_anomalies(rng, (T, C)), x)
        wf = rc.dyadic_weights(rng, C)
        thr = rc.thresholds(rng, 4, C)
        rc.assert_same(rc.run_engine(hot, x, reg, R, wf=wf, anom=anom), rc.oracle(x, reg, R, wf=wf, anom=anom))
        rc.assert_same(rc.run_engine(hot, x, reg, R, wf=wf, anom=anom, thr=thr, doy=doy),
                       rc.oracle(x, reg, R, wf=wf, anom=anom, thr=thr, doy=doy))


@pytest.mark.parametrize("C", [1024, 1022, 4099])
def test_uint8_field_one_byte_past_an_aligned_address(hot, C):
    rng = np.random.default_rng(C)
    T = 3
    reg, R = rc.region_map("edges", C)
    x = rc.mask_field(rng, T, C)
    anom = rc.dyadic_anomalies(rng, (T, C))
    q = rng.integers(0, 2**30, C).astype(np.int64)
    exp = rc.oracle(x, reg, R, q=q, anom=anom)
    rc.assert_same(rc.run_engine(hot, x, reg, R, q=q, anom=anom, offset=1), exp)
    rc.assert_same(rc.run_engine(hot, x, reg, R, q=q, anom=anom), exp)


@pytest.mark.parametrize("name,C", [("one", 4100), ("one", 12289), ("holes", 4100), ("own", 130), ("mod3", 4100), ("edges", 8200)])
def test_region_maps(hot, name, C):
    rng = np.random.default_rng(len(name) + C)
    T = 3
    reg, R = rc.region_map(name, C)
    if name == "own":
        assert R == 130  # 64 distinct regions in every full wave
    x = rc.mask_field(rng, T, C, 0.6)
    ids = rc.id_field(rng, T, C)
    anom = rc.spoil(rng, rc.dyadic_anomalies(rng, (T, C)), x)
    wf, q = rc.dyadic_weights(rng, C), rng.integers(0, 2**45, C).astype(np.int64)
    thr = rc.thresholds(rng, 2, C)
    doy = np.array([1, 0, 1], np.int32)
    for f in (x, ids):
        rc.assert_same(rc.run_engine(hot, f, reg, R, q=q), rc.oracle(f, reg, R, q=q))
        rc.assert_same(rc.run_engine(hot, f, reg, R, q=q, wf=wf, anom=anom), rc.oracle(f, reg, R, q=q, wf=wf, anom=anom))
        rc.assert_same(rc.run_engine(hot, f, reg, R, q=q, wf=wf, anom=anom, thr=thr, doy=doy),
                       rc.oracle(f, reg, R, q=q, wf=wf, anom=anom, thr=thr, doy=doy))
    if name == "edges":
        exp = rc.oracle(x, reg, R, q=q)
        assert exp["cnt"][:, 3].sum() == 0 and exp["cnt"].sum() > 0  # the region without cells
        assert exp["cnt"][..., 0].sum() == int((x > 0)[:, (reg >= 0) & (reg < R)].sum())  # indices outside 0 .. R - 1 add nothing


@pytest.mark.parametrize("name", ["one", "mod3", "edges"])
def test_areas_unit_zero_and_just_under_2_61(hot, name):
    rng = np.random.default_rng(7)
    T, C = 2, 8200
    reg, R = rc.region_map(name, C)
    x = np.ones((T, C), np.uint8)  # every cell present: the slot of R = 1 holds the whole table
    x[1] = rc.mask_field(rng, 1, C, 0.7)[0]
    e, q, wf = rc.near_2_61(rng, C)
    q0 = q.copy()
    q0[::3] = 0
    anom = rc.dyadic_anomalies(rng, (T, C))
    thr = rc.thresholds(rng, 1, C)
    doy = np.zeros(T, np.int32)
    for qq in (None, q0, q):
        exp = rc.oracle(x, reg, R, q=qq)
        rc.assert_same(rc.run_engine(hot, x, reg, R, q=qq), exp)
        rc.assert_same(rc.run_engine(hot, x, reg, R, q=qq, anom=anom, thr=thr, doy=doy),
                       rc.oracle(x, reg, R, q=qq, anom=anom, thr=thr, doy=doy))
        rc.assert_same(rc.run_engine(hot, x.astype(np.int32) * 4, reg, R, q=qq, match=4), exp)
    if name == "one":
        assert int(exp["area"][0, 0]) == sum(int(v) for v in q) > 2**61 - 2**40  # the carries between the 32-bit halves
        assert np.array_equal(rc.oracle(x, reg, R)["area"], rc.oracle(x, reg, R)["cnt"][..., 0])


def test_nan_infinities_negative_slots_and_slots_without_a_finite_cell(hot):
    rng = np.random.default_rng(3)
    T, C = 4, 2052
    reg, R = rc.region_map("mod3", C)
    x = rc.mask_field(rng, T, C, 0.5)
    anom = rc.spoil(rng, rc.dyadic_anomalies(rng, (T, C)), x)
    anom[1] = -np.abs(rc.dyadic_anomalies(rng, C)) - F(0.5)  # every slot of step 1 is negative: the key of the maximum
    anom[2, reg == 1] = np.where(rng.random(int((reg == 1).sum())) < 0.5, rc.NAN, rc.INF)  # slot (2, 1): no finite cell
    anom[3, reg == 2] = F(-0.0)
    exp = rc.oracle(x, reg, R, anom=anom)
    assert (exp["vmax"][1] < 0).all() and np.isnan(exp["vmax"][2, 1]) and exp["cnt"][2, 1].tolist()[0] == 0 < exp["cnt"][2, 1, 1]
    assert exp["area"][2, 1] == 0 and exp["sums"][2, 1].tolist() == [0.0, 0.0] and np.signbit(exp["vmax"][3, 2])
    for kw in (dict(), dict(wf=rc.dyadic_weights(rng, C), q=rng.integers(0, 99, C).astype(np.int64))):
        rc.assert_same(rc.run_engine(hot, x, reg, R, anom=anom, **kw), rc.oracle(x, reg, R, anom=anom, **kw))
        one = np.zeros(C, np.int32)
        rc.assert_same(rc.run_engine(hot, x, one, 1, anom=anom, **kw), rc.oracle(x, one, 1, anom=anom, **kw))


def test_dayofyear_rows_to_the_366th_and_undefined_thresholds(hot):
    rng = np.random.default_rng(4)
    T, C = 6, 1030
    reg, R = rc.region_map("edges", C)
    x = rc.mask_field(rng, T, C, 0.6)
    anom = rc.spoil(rng, rc.dyadic_anomalies(rng, (T, C)) / F(16), x)
    thr = rc.thresholds(rng, 366, C)
    thr[365, ::5] = rc.NAN
    doy = np.array([364, 365, 0, 58, 59, 365], np.int32)
    q = rng.integers(0, 2**35, C).astype(np.int64)
    exp = rc.oracle(x, reg, R, q=q, anom=anom, thr=thr, doy=doy)
    assert (exp["cat_cnt"].sum(axis=(0, 1)) > 0).all()  # every class, the undefined one included
    rc.assert_same(rc.run_engine(hot, x, reg, R, q=q, anom=anom, thr=thr, doy=doy), exp)
    assert np.array_equal(exp["cat_cnt"].sum(axis=2), exp["cnt"][..., 0]) and np.array_equal(exp["cat_area"].sum(axis=2), exp["area"])
    bad = doy.copy()
    bad[2] = 366
    with pytest.raises(ProcessingError, match="present cells lie under a step label outside its range"):
        rc.run_engine(hot, x, reg, R, q=q, anom=anom, thr=thr, doy=bad)


def test_windows_give_the_bytes_of_one_call(hot):
    rng = np.random.default_rng(5)
    T, C = 37, 4100
    for name in ("one", "edges"):
        reg, R = rc.region_map(name, C)
        x = rc.mask_field(rng, T, C)
        ids = rc.id_field(rng, T, C)
        anom = rc.spoil(rng, rc.dyadic_anomalies(rng, (T, C)), x)
        wf, q = rc.dyadic_weights(rng, C), rng.integers(0, 2**40, C).astype(np.int64)
        thr = rc.thresholds(rng, 5, C)
        doy = rng.integers(0, 5, T).astype(np.int32)
        for f, kw in ((x, dict(q=q, wf=wf, anom=anom)), (ids, dict(q=q, wf=wf, anom=anom, thr=thr, doy=doy)), (x, dict())):
            whole = rc.run_engine(hot, f, reg, R, **kw)
            rc.assert_same(whole, rc.oracle(f, reg, R, **kw))
            for cuts in ((0, 1, T - 1, T), (0, 19, T)):
                part = rc.run_engine(hot, f, reg, R, cuts=cuts, **kw)
                for k in ("area", "cnt", "sums", "vmax", "cat_cnt", "cat_area"):
                    assert (whole[k] is None) == (part[k] is None)
                    assert whole[k] is None or whole[k].tobytes() == part[k].tobytes(), (k, cuts)


def test_int32_match_and_negative_ids(hot):
    rng = np.random.default_rng(6)
    T, C = 3, 2100
    reg, R = rc.region_map("edges", C)
    ids = rc.id_field(rng, T, C)
    anom = rc.dyadic_anomalies(rng, (T, C))
    for m in (0, 2, 5, 9):
        rc.assert_same(rc.run_engine(hot, ids, reg, R, anom=anom, match=m), rc.oracle(ids, reg, R, anom=anom, match=m))
    ids[1, 77] = -3
    with pytest.raises(DataValidationError, match="Object IDs must be non-negative"):
        rc.run_engine(hot, ids, reg, R, anom=anom)
    with pytest.raises(DataValidationError, match="Object IDs must be non-negative"):
        marex_amd.regional_series(ids, regions=np.maximum(reg, -1))


def test_normal_anomalies_stay_within_the_derived_bound(hot):
    rng = np.random.default_rng(8)
    T, C = 3, 12300
    x = rc.mask_field(rng, T, C, 0.5)
    anom = rc.spoil(rng, rng.standard_normal((T, C)).astype(F), x)
    wf = rng.uniform(0.1, 3.0, C).astype(F)
    for name in ("one", "mod3", "edges"):
        reg, R = rc.region_map(name, C)
        r = rc.run_engine(hot, x, reg, R, wf=wf, anom=anom)
        rc.assert_same(r, rc.oracle(x, reg, R, wf=wf, anom=anom), float_bytes=False)
        rc.assert_within_bound(r, x, reg, R, wf, anom)


# ---------------------------------------------------------------- against the statistics that exist already
def test_rows_as_regions_equal_the_zonal_sections(hot):
    rng = np.random.default_rng(9)
    T, ny, nx = 5, 7, 36
    x = rc.mask_field(rng, T, ny * nx).reshape(T, ny, nx)
    anom = rc.spoil(rng, rc.dyadic_anomalies(rng, (T, ny * nx)), x.reshape(T, -1)).reshape(T, ny, nx)
    thr = rc.thresholds(rng, 1, ny * nx).reshape(ny, nx)
    rows = np.repeat(np.arange(ny)[:, None], nx, axis=1)
    ds = marex_amd.regional_series(x, regions=rows, dat_anomaly=anom, thresholds=thr)
    occ = marex_amd.event_occurrence(x, zonal=True, zonal_by="step")
    li = marex_amd.local_intensity(x, anom, thresholds=thr, zonal=True, zonal_by="step")
    # event_occurrence counts every present cell, the series without anomalies too
    assert np.array_equal(np.asarray(marex_amd.regional_series(x, regions=rows)["cells"].values),
                          np.asarray(occ["presence_cells"].values).astype(np.int64))
    assert np.array_equal(np.asarray(ds["category_cells"].values), np.asarray(li["category_cells"].values).astype(np.int64))
    assert np.asarray(ds["category_cells"].values).sum() > 0


def test_equals_event_intensity_on_the_materialised_id_field(hot):
    rng = np.random.default_rng(10)
    T, C = 6, 1500
    x = rc.mask_field(rng, T, C)
    anom = rc.spoil(rng, rc.dyadic_anomalies(rng, (T, C)), x)
    regions = (np.arange(C) // 400).astype(np.int32)  # basins 0 .. 3
    w = rc.dyadic_weights(rng, C) + F(1)
    ds = marex_amd.regional_series(x, regions=regions, cell_areas=w, dat_anomaly=anom)
    ev = marex_amd.event_intensity(((regions + 1)[None, :] * x).astype(np.int32), anom, cell_areas=w)
    cells, integral, vmax = (np.asarray(ds[k].values) for k in ("cells", "intensity_integral", "intensity_max"))
    assert np.array_equal(cells, np.asarray(ev["intensity_cells"].values))
    assert np.array_equal(integral, np.asarray(ev["intensity_integral"].values), equal_nan=True)
    assert np.array_equal(vmax, np.asarray(ev["intensity_max"].values), equal_nan=True) and cells.sum() > 0


# ---------------------------------------------------------------- the public path
def _assert_dataset(ds, exp, lead):
    assert sorted(ds.data_vars) == sorted(exp)
    for k, want in exp.items():
        got = np.asarray(ds[k].values)
        assert got.shape == want.shape and got.dtype == want.dtype, (k, got.shape, want.shape, got.dtype, want.dtype)
        assert np.array_equal(got, want, equal_nan=got.dtype.kind == "f"), k
    assert tuple(ds["cells"].dims) == (lead, "region") and tuple(ds["region_area"].dims) == ("region",)


def test_public_path_on_a_grid(hot):
    import torch

    rng = np.random.default_rng(11)
    T, ny, nx = 40, 9, 44
    C = ny * nx
    tv = _days(T)
    x = rc.mask_field(rng, T, C)
    anom = rc.spoil(rng, rc.dyadic_anomalies(rng, (T, C)), x)
    thr = rc.thresholds(rng, 366, C)
    regions = (np.add.outer(np.arange(ny) // 3, 10 * (np.arange(nx) // 15))).reshape(-1) * 7 - 7  # -7 is no region
    valid = rng.random(C) < 0.9
    area_y = np.cos(np.radians(np.linspace(-60, 60, ny))) * 100
    doy = marex_amd.calendar._to_year_doy(tv)[1].astype(np.int32) - 1
    year = np.asarray(tv.astype("datetime64[Y]").astype(np.int64))
    exp = ro.regional_series(x, regions, np.repeat(area_y, nx), anom, thr, doy, valid, year - year.min(), 2)
    dims = ("time", "lat", "lon")
    coords = {"time": ("time", tv)}
    f = DataArray(x.reshape(T, ny, nx), dims=dims, coords=coords)
    a = DataArray(anom.reshape(T, ny, nx), dims=dims, coords=coords)
    h = DataArray(np.ascontiguousarray(np.moveaxis(thr.reshape(366, ny, nx), 0, -1)), dims=("lat", "lon", "dayofyear"))
    kw = dict(regions=regions.reshape(ny, nx), cell_areas=area_y, mask=valid.reshape(ny, nx), by="year")
    ds = marex_amd.regional_series(f, dat_anomaly=a, thresholds=h, **kw)
    _assert_dataset(ds, exp, "time")
    assert np.asarray(ds["cells"].coords["region"].values).tolist() == sorted(set(regions[regions >= 0].tolist()))
    assert np.asarray(ds["category_cells"].coords["category"].values).tolist() == list(marex_amd.regional.CATEGORIES)
    assert np.asarray(ds["steps_by"].coords["year"].values).tolist() == [2003, 2004] and np.array_equal(ds["cells"].coords["time"].values, tv)
    # the three threshold layouts, host and resident inputs, bool and uint8, windows: the same bytes
    others = [
        marex_amd.regional_series(f, dat_anomaly=a, thresholds=thr.reshape(366, ny, nx), **kw),
        marex_amd.regional_series(DataArray(torch.from_numpy(x.reshape(T, ny, nx).astype(bool)).to(hot.device), dims=dims, coords=coords),
                                  dat_anomaly=torch.from_numpy(anom.reshape(T, ny, nx)).to(hot.device),
                                  thresholds=torch.from_numpy(thr.reshape(366, ny, nx)).to(hot.device),
                                  **{**kw, "by": (year - year.min()).astype(np.int32)}),
        marex_amd.regional_series(DataArray(x.reshape(T, ny, nx).astype(bool), dims=dims, coords=coords), dat_anomaly=a, thresholds=h,
                                  block_steps=7, **kw),
    ]
    for o in others:
        for k in ds.data_vars:
            assert np.asarray(o[k].values).tobytes() == np.asarray(ds[k].values).tobytes(), k
    # (*space) alone, by labels, no areas
    g = np.linspace(0.2, 1.2, C).astype(F)
    lab = (np.arange(T) % 3).astype(np.int32)
    exp = ro.regional_series(x, regions, None, anom, g[None], np.zeros(T, np.int32), None, lab, 3)
    ds = marex_amd.regional_series(x.reshape(T, ny, nx), regions=regions.reshape(ny, nx), dat_anomaly=anom.reshape(T, ny, nx),
                                   thresholds=g.reshape(ny, nx), by=lab)
    _assert_dataset(ds, exp, "time")
    assert np.array_equal(np.asarray(ds["category_area"].values), np.asarray(ds["category_cells"].values).astype(np.float64))


def test_public_path_on_a_mesh_and_the_tracker_method(hot):
    from marex_amd.track_mesh import mesh_weight_tables

    rng = np.random.default_rng(12)
    T, C = 9, 3001
    ids = rc.id_field(rng, T, C)
    anom = rc.spoil(rng, rc.dyadic_anomalies(rng, (T, C)), ids)
    # orders of magnitude apart, as on a mesh, and whole numbers below 2^22: the sums of area x anomaly stay exact
    areas = rng.integers(1, 2**10, C) * 2.0 ** rng.integers(0, 12, C)
    regions = rng.integers(-1, 12, C) * 3
    exp = ro.regional_series(ids, regions, areas, anom)
    ds = marex_amd.regional_series(DataArray(ids, dims=("time", "ncells")), regions=regions, cell_areas=areas,
                                   dat_anomaly=DataArray(anom, dims=("time", "ncells")))
    _assert_dataset(ds, exp, "time")
    e, q = marex_amd.regional.area_weight_table(areas)
    e4, q4 = mesh_weight_tables(areas, np.zeros(C), np.zeros(C))
    assert e == e4 and q.tobytes() == q4[0].tobytes()
    S = np.zeros((T, 12), object)
    ok = (ids > 0) & np.isfinite(anom) & (regions >= 0)[None]
    for t in range(T):
        np.add.at(S[t], (regions // 3)[ok[t]], q.astype(object)[ok[t]])
    assert np.array_equal(np.asarray(ds["area"].values), np.ldexp(S.astype(np.float64), -e))
    exp5 = ro.regional_series(ids, regions, areas, None, match=5)
    _assert_dataset(marex_amd.regional_series(ids, regions=regions, cell_areas=areas, event_id=5), exp5, "time")



# ---------------------------------------------------------------- the tracker's method on tracked fields
def _same_bytes(a, b):
    assert list(a.data_vars) == list(b.data_vars)
    for k in a.data_vars:
        assert np.asarray(a[k].values).tobytes() == np.asarray(b[k].values).tobytes(), k


@pytest.mark.parametrize("merging", [True, False], ids=["merge", "basic"])
def test_grid_tracker_method_on_its_own_tracked_field(hot, merging):
    from intensity_cases import blob_anomalies, blobs

    ev = blobs()
    T, ny, nx = ev.shape
    tv = np.arange(T).astype("datetime64[D]").astype("datetime64[ns]")
    lat, lon = np.linspace(-57.5, 57.5, ny).astype(F), np.linspace(3.75, 356.25, nx).astype(F)
    valid = np.ones((ny, nx), bool)
    valid[5:9, 6:12] = False  # land under the first disc's path
    valid[:, 40] = False
    ev = ev & valid[None]
    dims = ("time", "lat", "lon")
    coords = {"time": ("time", tv), "lat": ("lat", lat), "lon": ("lon", lon)}
    trk = marex_amd.tracker(DataArray(ev, dims=dims, coords=coords, name="extreme_events"), DataArray(valid, dims=("lat", "lon")),
                            R_fill=1, T_fill=2, area_filter_quartile=0.2, timechunks=4, coordinate_units="degrees",
                            allow_merging=merging, grid_resolution=7.5)
    events = trk.run()
    ids = np.asarray(events["ID_field"].values)
    assert ids.shape == ev.shape and ids.max() >= 2 and not ids[:, ~valid].any()
    anom = blob_anomalies(ev.shape)
    thr = rc.thresholds(np.random.default_rng(13), 1, ny * nx).reshape(ny, nx)
    ex = marex_amd.Dataset({"dat_anomaly": DataArray(anom, dims=dims, coords=coords), "thresholds": DataArray(thr, dims=("lat", "lon"))})
    regions = np.add.outer(np.arange(ny) // 8, 3 * (np.arange(nx) // 16))  # 3 x 3 blocks, some with land
    # what the tracker holds: the [ny, nx] mask, and float32 areas of the area pass with merging only
    assert np.array_equal(trk._mask_host, valid)
    areas = trk._cell_weights if merging else None
    assert (areas is not None and areas.shape == (ny, nx) and areas.dtype == F and np.ptp(areas) > 0) if merging else \
        getattr(trk, "_cell_weights", None) is None
    ds = trk.regional_series(events, ex, regions=regions, by="year")
    free = marex_amd.regional_series(events["ID_field"], regions=regions, mask=valid, cell_areas=areas, dat_anomaly=ex["dat_anomaly"],
                                     thresholds=ex["thresholds"], by="year")
    _same_bytes(ds, free)
    a1 = None if areas is None else areas.reshape(-1)
    exp = ro.regional_series(ids.reshape(T, -1), regions.reshape(-1), a1, anom.reshape(T, -1), thr.reshape(1, -1), np.zeros(T, np.int32),
                             valid.reshape(-1), np.zeros(T, np.int32), 1)
    _assert_dataset(ds, exp, "time")
    assert np.array_equal(ds["cells"].coords["time"].values, tv) and np.asarray(ds["cells"].values).sum() > 0
    # masked and weighted: not the series of an unmasked map or of unit areas
    assert np.asarray(ds["region_cells"].values).sum() == int(valid.sum()) < ny * nx
    if merging:
        assert not np.array_equal(np.asarray(ds["area"].values), np.asarray(ds["cells"].values).astype(np.float64))
    else:  # the basic tracker keeps no areas: cells, unless they are passed
        assert np.array_equal(np.asarray(ds["area"].values), np.asarray(ds["cells"].values).astype(np.float64))
        w = np.cos(np.radians(lat)).astype(np.float64)
        _same_bytes(trk.regional_series(events, ex, regions=regions, cell_areas=w, block_steps=5),
                    marex_amd.regional_series(events["ID_field"], regions=regions, mask=valid, cell_areas=w,
                                              dat_anomaly=ex["dat_anomaly"], thresholds=ex["thresholds"]))
    # a presence field instead of the events, no extremes Dataset
    _same_bytes(trk.regional_series(DataArray(ev, dims=dims, coords=coords), regions=regions),
                marex_amd.regional_series(ev, regions=regions, mask=valid, cell_areas=areas))
    with pytest.raises(TypeError, match="unexpected keyword argument 'zonal'"):
        trk.regional_series(events, regions=regions, zonal=True)


def test_mesh_tracker_method_on_its_own_tracked_field(hot):
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
    ids = np.asarray(events["ID_field"].values)
    T, C = ids.shape
    assert ids.max() >= 2
    valid, areas = np.asarray(f["mask"]).astype(bool), np.asarray(f["areas"])
    rng = np.random.default_rng(9)
    anom = (rng.integers(1, 2**13, ids.shape) / 1024.0).astype(F)
    anom[rng.random(ids.shape) < 0.02] = np.nan
    regions = (np.asarray(f["lat"]) > np.median(f["lat"])).astype(np.int64) * 5 + 2  # two regions, 2 and 7
    ex = marex_amd.Dataset({"dat_anomaly": DataArray(anom, dims=("time", "ncells"))})
    ds = trk.regional_series(events, ex, regions=regions)
    _same_bytes(ds, marex_amd.regional_series(events["ID_field"], regions=regions, mask=valid, cell_areas=areas, dat_anomaly=anom))
    exp = ro.regional_series(ids, regions, areas, anom, mask=valid)
    # Mesh areas are any float32, so the partial sums need not be representable: every integer and the maximum equal the
    # oracle, the two sums lie within their bound of math.fsum.  All terms are positive here (anomalies > 0), so S and W
    # carry a relative error of at most 2 n u each, and their quotient, one more division, of at most (4 n + 1) u.
    W, S, A, n = ro.exact_sums(ids, np.where(valid, (regions - 2) // 5, -1), 2, areas.astype(F), anom)
    for k, want in exp.items():
        got = np.asarray(ds[k].values)
        assert got.shape == want.shape and got.dtype == want.dtype, k
        if k == "intensity_integral":
            assert np.array_equal(np.isnan(got), n == 0) and (np.abs(got - S)[n > 0] <= (2 * n * ro.U * A)[n > 0]).all()
        elif k == "intensity_mean":
            live = n > 0
            assert np.array_equal(np.isnan(got), ~live) and (W[live] > 0).all()
            ref = S / np.where(live, W, 1)  # three more roundings: the two fsum results and this division
            assert (np.abs(got - ref)[live] <= ((4 * n + 4) * ro.U * ref)[live]).all()
        else:
            assert np.array_equal(got, want, equal_nan=got.dtype.kind == "f"), k
    assert np.asarray(ds["cells"].coords["region"].values).tolist() == [2, 7] and np.asarray(ds["cells"].values).sum() > 0
    e, q = marex_amd.regional.area_weight_table(areas)
    S = np.zeros((T, 2), object)
    ok = (ids > 0) & np.isfinite(anom) & valid[None]
    for t in range(T):
        np.add.at(S[t], ((regions - 2) // 5)[ok[t]], q.astype(object)[ok[t]])
    assert np.array_equal(np.asarray(ds["area"].values), np.ldexp(S.astype(np.float64), -e))
