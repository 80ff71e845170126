"""The tracker's object stages (compute_area, calculate_centroid, calculate_object_properties, check_overlap_slice,
find_overlapping_objects, enforce_overlap_threshold; marEx/track.py:1499-1518, 2050-2552) on the host: hand-computed
centroids, the oracle of tests/objects_oracle.py against brute force, the reference's enforce_overlap_threshold cases
and the checks that run before any GPU call -- no GPU needed."""
import logging
import os
import sys

import numpy as np
import pytest

import marex_amd
from marex_amd.exceptions import ConfigurationError, DataValidationError
from marex_amd.xr_compat import DataArray, Dataset

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import objects_oracle as oo  # noqa: E402

NX_LIST = [1, 50, 100, 150, 199, 200, 201, 360]


def _tracker(regional_mode=False, **kw):
    ev = np.zeros((2, 3, 4), dtype=bool)
    ev[0, 1, 1] = True
    da = DataArray(ev, dims=("time", "lat", "lon"), coords={"time": np.arange(2), "lat": np.arange(3.0), "lon": np.arange(4.0)})
    mask = DataArray(np.ones((3, 4), dtype=bool), dims=("lat", "lon"))
    return marex_amd.tracker(da, mask, R_fill=0, area_filter_quartile=0.5, allow_merging=False, regional_mode=regional_mode, **kw)


@pytest.fixture
def no_gpu(monkeypatch):
    import marex_amd.detect as det

    def refuse(*a, **k):
        raise AssertionError("the GPU engine was touched")

    monkeypatch.setattr(det, "get_engine", refuse)


def _mask(nx, cols, ny=3, rows=(1,)):
    m = np.zeros((ny, nx), dtype=bool)
    for r in rows:
        m[r, list(cols)] = True
    return m


# (nx, columns of the object in one row, expected column centroid), computed by hand from the seam rule:
# near left = a column < 100, near right = a column >= nx - 100; then columns > nx // 2 count as column - nx
HAND_CENTROIDS = [
    (360, (0, 1, 2, 359), 0.5),           # straddles the seam, positive mean: (0 + 1 + 2 - 1) / 4
    (360, (0, 1, 358, 359), 359.5),       # negative mean -0.5, + nx
    (360, (100, 200), 150.0),             # in neither band
    (1, (0,), 0.0),                       # both bands are the whole row; 0 > 0 // 2 is false
    (50, (0, 49), 49.5),                  # (0 - 1) / 2 + 50
    (50, (10, 20), 15.0),                 # both bands, nothing right of 25
    (50, (20, 30), 0.0),                  # both columns in both bands; 30 > 25 -> -20; mean 0.0, not negative
    (100, (0, 99), 99.5),
    (150, (10, 140), 0.0),                # 10 < 100 and 140 >= 50; 140 > 75 -> -10; mean 0.0, not negative
    (150, (76,), 76.0),                   # one column in both bands: 76 - 150 = -74 < 0 -> 76
    (199, (0, 198), 198.5),
    (199, (98, 100), 198.5),              # 100 >= 99 is in the right band; 100 > 99 -> -99; mean -0.5 -> 198.5
    (200, (10, 150), 180.0),              # 150 > 100 -> -50; mean -20 -> 180
    (200, (99, 100), 99.5),               # 100 >= 100 but 100 > 100 is false: plain mean
    (201, (99, 101), 200.5),              # 101 >= 101; 101 > 100 -> -100; mean -0.5 -> 200.5
    (201, (99, 100), 99.5),               # 100 < 101: not near the right edge
]


@pytest.mark.parametrize("nx,cols,expected", HAND_CENTROIDS)
def test_hand_computed_centroids(nx, cols, expected):
    m = _mask(nx, cols)
    y, x = _tracker().calculate_centroid(m)
    assert (y, x) == (1.0, expected)
    assert oo.centroid(m) == (1.0, expected)
    ids = m.astype(np.int32) * 7
    got_id, got_area, got_c = oo.object_properties(ids)
    assert got_id.tolist() == [7] and got_area.tolist() == [float(len(cols))]
    assert got_c[:, 0].tolist() == [1.0, expected]


@pytest.mark.parametrize("nx,cols,expected", HAND_CENTROIDS)
def test_regional_mode_takes_the_plain_mean(nx, cols, expected):
    m = _mask(nx, cols)
    plain = float(np.mean(cols))
    assert _tracker(regional_mode=True).calculate_centroid(m) == (1.0, plain)
    assert _tracker(regional_mode=True).calculate_centroid(m, (0.25, 0.75)) == (0.25, 0.75)
    assert oo.centroid(m, regional_mode=True) == (1.0, plain)


def test_original_centroid_is_kept_off_the_seam():
    m = _mask(360, (100, 101))
    assert _tracker().calculate_centroid(m, (5.0, 6.0)) == (5.0, 6.0)
    m = _mask(360, (0, 359))
    assert _tracker().calculate_centroid(m, (5.0, 6.0)) == (5.0, 359.5)


@pytest.mark.parametrize("regional_mode", [False, True])
def test_fast_oracle_equals_object_by_object_oracle(regional_mode):
    rng = np.random.default_rng(11)
    for nx in NX_LIST:
        for dens in (0.05, 0.3, 0.9):
            ids = np.where(rng.random((3, 5, nx)) < dens, rng.integers(1, 9, (3, 5, nx)), 0).astype(np.int32)
            ids[1] = 0  # an empty slice
            a = oo.object_properties_slow(ids, regional_mode)
            b = oo.object_properties(ids, regional_mode)
            for u, v in zip(a, b):
                assert u.dtype == v.dtype and np.array_equal(u, v), (nx, dens)


def test_overlap_oracle_against_brute_force():
    rng = np.random.default_rng(3)
    for shape in ((1, 4, 5), (2, 3, 3), (5, 6, 7), (4, 1, 30), (6, 9, 1)):
        for dens in (0.0, 0.2, 0.7, 1.0):
            ids = np.where(rng.random(shape) < dens, rng.integers(1, 6, shape), 0).astype(np.int32)
            exp = oo.overlaps_brute_force(ids)
            got = oo.find_overlapping_objects(ids)
            assert got.dtype == np.int32 and got.shape[1] == 3 and np.array_equal(got, exp), (shape, dens)
            if shape[0] >= 2:
                assert np.array_equal(oo.check_overlap_slice(ids[0], ids[1]), oo.overlaps_brute_force(ids[:2]))
    assert oo.check_overlap_slice(np.zeros((2, 2), np.int32), np.ones((2, 2), np.int32)).shape == (0, 3)


def _props(ids, areas):
    coord = {"ID": ("ID", np.asarray(ids))}
    return Dataset({"area": DataArray(np.asarray(areas, dtype=np.float64), dims=("ID",), coords=coord)}, coords=coord)


def test_enforce_overlap_threshold_empty_valid_overlaps():
    """Reference tests/test_track_edge_cases.py::TestEnforceOverlapThreshold, the empty case, with allow_merging=False."""
    trk = _tracker(regional_mode=True)
    overlap_list = np.array([[999, 1000, 50.0], [1001, 1002, 60.0]], dtype=np.float32)
    result = trk.enforce_overlap_threshold(overlap_list, _props([1, 2], [100.0, 200.0]))
    assert result.shape == (0, 3) and result.dtype == np.int32
    assert trk.enforce_overlap_threshold(np.zeros((0, 3), np.int32), _props([1], [1.0])).shape == (0, 3)


def test_enforce_overlap_fraction_greater_than_one(caplog):
    """The reference's > 1.0 case with allow_merging=False: the warning goes to the marex_amd logger."""
    trk = _tracker(regional_mode=True, overlap_threshold=0.1)
    overlap_list = np.array([[1, 2, 150], [3, 4, 80]], dtype=np.int32)
    props = _props([1, 2, 3, 4], [100.0, 120.0, 200.0, 300.0])
    with caplog.at_level(logging.WARNING, logger="marex_amd"):
        result = trk.enforce_overlap_threshold(overlap_list, props)
    assert result is not None and len(result) > 0
    assert result.dtype == np.int32 and result.tolist() == [[1, 2, 150], [3, 4, 80]]
    assert any("overlap fractions > 1.0" in r.getMessage() for r in caplog.records)
    exp = oo.enforce_overlap_threshold(overlap_list, [1, 2, 3, 4], [100.0, 120.0, 200.0, 300.0], 0.1)
    assert np.array_equal(result, exp)


def test_enforce_overlap_threshold_matches_the_oracle():
    rng = np.random.default_rng(8)
    ids = np.arange(1, 40)
    areas = rng.integers(1, 50, ids.size).astype(np.float64)
    ov = np.stack([rng.integers(1, 45, 200), rng.integers(1, 45, 200), rng.integers(1, 60, 200)], axis=1).astype(np.int32)
    for thr in (0.0, 0.25, 0.5, 1.0, 2.0):
        got = _tracker(overlap_threshold=thr).enforce_overlap_threshold(ov, _props(ids[::-1], areas[::-1]))
        exp = oo.enforce_overlap_threshold(ov, ids, areas, thr)
        assert got.dtype == ov.dtype and np.array_equal(got, exp), thr


def test_enforce_overlap_threshold_refuses_repeated_ids():
    with pytest.raises(DataValidationError, match="repeated IDs"):
        _tracker().enforce_overlap_threshold(np.array([[1, 2, 3]], np.int32), _props([1, 2, 1], [4.0, 5.0, 6.0]))


def test_the_methods_exist():
    for name in ("compute_area", "calculate_centroid", "calculate_object_properties", "check_overlap_slice",
                 "find_overlapping_objects", "enforce_overlap_threshold"):
        assert callable(getattr(marex_amd.tracker, name, None)), name


def test_overlap_threshold_is_stored():
    assert _tracker().overlap_threshold == 0.5
    assert _tracker(overlap_threshold=0.3).overlap_threshold == 0.3


@pytest.mark.parametrize("props", [["label", "area", "eccentricity"], ["bbox"], ["centroid", "perimeter"]])
def test_unsupported_property_raises_before_any_engine_call(no_gpu, props):
    ids = np.zeros((2, 3, 4), np.int32)
    with pytest.raises(ConfigurationError) as ei:
        _tracker().calculate_object_properties(ids, props)
    assert "label" in ei.value.details and "centroid" in ei.value.details and "area" in ei.value.details


def test_bad_id_fields_raise_before_any_engine_call(monkeypatch):
    """Host-side validation of the ID field happens before the first kernel; the engine is created but never called."""
    import marex_amd.detect as det

    class NoKernels:
        device = "cpu"

        def __getattr__(self, name):
            raise AssertionError(f"engine.{name} was called")

    monkeypatch.setattr(det, "get_engine", lambda *a, **k: NoKernels())
    trk = _tracker()
    with pytest.raises(DataValidationError, match="non-negative"):
        trk.calculate_object_properties(np.full((2, 3, 4), -1, np.int64))
    with pytest.raises(DataValidationError, match="fit int32"):
        trk.find_overlapping_objects(np.full((2, 3, 4), 2**31, np.int64))
    with pytest.raises(DataValidationError, match="integers"):
        trk.find_overlapping_objects(np.zeros((2, 3, 4), np.float32))
    with pytest.raises(DataValidationError, match="Invalid dimensions"):
        trk.find_overlapping_objects(DataArray(np.zeros((2, 3, 4), np.int32), dims=("time", "y", "lon")))


def test_compute_area_counts_cells_per_timestep():
    rng = np.random.default_rng(2)
    ev = rng.random((5, 4, 6)) < 0.4
    tm = np.arange(5) * 10
    da = DataArray(ev, dims=("time", "lat", "lon"), coords={"time": tm})
    a = _tracker().compute_area(da)
    assert tuple(a.dims) == ("time",) and a.values.dtype == np.int64
    assert np.array_equal(a.values, oo.compute_area(ev))
    assert np.array_equal(np.asarray(a.coords["time"].values), tm)
    t = DataArray(np.ascontiguousarray(ev.transpose(2, 0, 1)), dims=("lon", "time", "lat"))
    assert np.array_equal(_tracker().compute_area(t).values, oo.compute_area(ev))
