"""Basic tracker (marEx.tracker(..., allow_merging=False), track.py:1162-1497) on the host: the oracle chain against the
numbers the reference's tests pin, the oracle's numbering, and the constructor's validation -- no GPU needed."""
import os
import sys

import numpy as np
import pytest

import marex_amd
from marex_amd import zarr_io
from marex_amd.exceptions import ConfigurationError, DataValidationError, TrackingError
from marex_amd.xr_compat import DataArray

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import track_oracle as tor  # noqa: E402

FIX = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "ref_fixtures", "extremes_gridded.zarr")

# tests/test_gridded_tracking.py of the reference: (R_fill, T_fill, quartile, exclude poles) -> N_objects_prefiltered,
# N_objects_filtered, N_events_final, preprocessed_area_fraction (test_basic_tracking 23-77,
# test_different_filtering_parameters 205-260, test_temporal_gap_filling 262-320)
REFERENCE_ROWS = [
    ((4, 0, 0.5, True), (549, 274, 24, 0.9724)),
    ((2, 0, 0.0, False), (1046, 1045, 152, 1.0622)),
    ((2, 0, 0.8, False), (1046, 209, 21, 1.5423)),
    ((2, 0, 0.5, False), (1046, 522, 54, 1.1650)),
    ((2, 4, 0.5, False), (1041, 522, 38, 1.0080)),
]


def load_fixture(exclude_poles: bool):
    ev = zarr_io.read_array(os.path.join(FIX, "extreme_events")).astype(bool)
    mask = zarr_io.read_array(os.path.join(FIX, "mask")).astype(bool)
    lat = zarr_io.read_array(os.path.join(FIX, "lat"))
    lon = zarr_io.read_array(os.path.join(FIX, "lon"))
    tm = zarr_io.read_array(os.path.join(FIX, "time"))
    if exclude_poles:  # mask.where((lat < 85) & (lat > -90), other=False)
        mask = mask & ((lat < 85) & (lat > -90))[:, None]
    return ev, mask, lat, lon, tm


@pytest.mark.parametrize("params,expected", REFERENCE_ROWS)
def test_oracle_reproduces_the_reference_tracking_numbers(params, expected):
    R, Tf, q, poles = params
    ev, mask, *_ = load_fixture(poles)
    ids, attrs = tor.run(ev, mask, R, Tf, q)
    n0, n1, nev, frac = expected
    assert (attrs["N_objects_prefiltered"], attrs["N_objects_filtered"], attrs["N_events_final"]) == (n0, n1, nev)
    assert round(attrs["preprocessed_area_fraction"], 4) == frac
    assert int(ids.max()) == nev and int(ids.min()) == 0
    assert np.array_equal(np.unique(ids), np.arange(nev + 1))


def test_oracle_numbering_is_scipy_scan_order_without_the_seam():
    from scipy import ndimage as ndi

    rng = np.random.default_rng(5)
    for shape, dens in (((6, 17, 23), 0.3), ((1, 9, 40), 0.5), ((12, 1, 30), 0.4), ((5, 8, 1), 0.6)):
        x = rng.random(shape) < dens
        exp, n = ndi.label(x, structure=np.ones((3, 3, 3), dtype=bool))
        got, m = tor.label_3d(x, wrap_x=False)
        assert m == n and np.array_equal(got, exp)
        # columns 0 and nx - 1 never touch: the seam changes nothing either
        if shape[2] > 2:
            x[:, :, -1] = False
            exp, n = ndi.label(x, structure=np.ones((3, 3, 3), dtype=bool))
            got, m = tor.label_3d(x, wrap_x=True)
            assert m == n and np.array_equal(got, exp)


def test_oracle_joins_across_the_seam_diagonally_in_time():
    x = np.zeros((2, 3, 8), dtype=bool)
    x[0, 0, 7] = True   # (t-1, y-1, x = nx-1)
    x[1, 1, 0] = True   # (t, y, x = 0)
    ids, n = tor.label_3d(x, wrap_x=True)
    assert n == 1 and ids[0, 0, 7] == ids[1, 1, 0] == 1
    ids, n = tor.label_3d(x, wrap_x=False)
    assert n == 2 and ids[0, 0, 7] == 1 and ids[1, 1, 0] == 2


def _da(ev=None, dims=("time", "lat", "lon"), coords=None):
    if ev is None:
        ev = np.zeros((4, 6, 8), dtype=bool)
        ev[1, 2, 3] = True
    T, ny, nx = ev.shape
    c = {"time": np.arange(T), "lat": np.linspace(-80, 80, ny), "lon": np.linspace(0, 360, nx, endpoint=False)}
    return DataArray(ev, dims=dims, coords=c if coords is None else coords)


def _mask(ny=6, nx=8, dtype=bool, value=True):
    return DataArray(np.full((ny, nx), value, dtype=dtype), dims=("lat", "lon"))


@pytest.mark.parametrize("kwargs,exc,prefix", [
    (dict(), ConfigurationError, "allow_merging=True is not supported"),
    (dict(allow_merging=False, unstructured_grid=True), ConfigurationError, "unstructured_grid=True is not supported"),
    (dict(allow_merging=False, checkpoint="save"), ConfigurationError, "checkpoint='save' is not supported"),
    (dict(allow_merging=False, checkpoint="load"), ConfigurationError, "checkpoint='load' is not supported"),
    (dict(allow_merging=False, data_bin=_da(np.zeros((4, 6, 8), bool), dims=("time", "y", "lon"))), DataValidationError,
     "Invalid dimensions for gridded data"),
    (dict(allow_merging=False, data_bin=_da(coords={"time": np.arange(4), "lat": np.arange(6)})), DataValidationError,
     "Missing required coordinates"),
    (dict(allow_merging=False, data_bin=_da(np.zeros((4, 6, 8), np.int8))), DataValidationError,
     "Input DataArray must be binary"),
    (dict(allow_merging=False, mask=_mask(dtype=np.int8, value=1)), DataValidationError, "Mask must be binary"),
    (dict(allow_merging=False, mask=_mask(value=False)), DataValidationError, "Mask contains only False values"),
    (dict(allow_merging=False, area_filter_quartile=1.5), ConfigurationError, "Invalid area_filter_quartile value"),
    (dict(allow_merging=False, area_filter_quartile=-0.1), ConfigurationError, "Invalid area_filter_quartile value"),
    (dict(allow_merging=False, area_filter_absolute=0), ConfigurationError, "Invalid area_filter_absolute value"),
    (dict(allow_merging=False, area_filter_quartile=0.5, area_filter_absolute=10), ConfigurationError,
     "Cannot specify both area filtering parameters"),
    (dict(allow_merging=False, T_fill=3), ConfigurationError, "T_fill must be even for temporal symmetry"),
    (dict(allow_merging=False, grid_resolution=0.0), DataValidationError, "grid_resolution must be a positive number"),
    (dict(allow_merging=False, grid_resolution=-1), DataValidationError, "grid_resolution must be a positive number"),
    (dict(allow_merging=False, cell_areas=DataArray(np.ones((6, 8)), dims=("y", "x"))), DataValidationError,
     "Invalid cell_areas dimensions for structured grid"),
])
def test_constructor_errors_before_any_gpu_call(kwargs, exc, prefix, monkeypatch):
    import marex_amd.detect as det

    def no_gpu(*a, **k):
        raise AssertionError("the constructor touched the GPU engine")

    monkeypatch.setattr(det, "get_engine", no_gpu)
    kw = dict(data_bin=_da(), mask=_mask(), R_fill=2)
    kw.update(kwargs)
    with pytest.raises(exc) as ei:
        marex_amd.tracker(**kw)
    assert str(ei.value).startswith(prefix), str(ei.value)


def test_valid_configuration_constructs_without_a_gpu(monkeypatch):
    import marex_amd.detect as det

    monkeypatch.setattr(det, "get_engine", lambda *a, **k: (_ for _ in ()).throw(AssertionError("GPU touched")))
    t = marex_amd.tracker(_da(), _mask(), R_fill=2, area_filter_absolute=5, T_fill=2, allow_merging=False, grid_resolution=1.0,
                          cell_areas=DataArray(np.ones((6, 8)), dims=("lat", "lon")), temp_dir="/nonexistent", quiet=True)
    assert t.area_filter_quartile == 0.0 and t.area_filter_absolute == 5   # _resolve_area_filtering_parameters
    t = marex_amd.tracker(_da(), _mask(), R_fill=2, allow_merging=False)
    assert t.area_filter_quartile == 0.5 and t.T_fill == 2


def test_fields_of_2_31_cells_are_refused_before_labelling():
    with pytest.raises(TrackingError, match="more than 2"):
        marex_amd.tracker._check_size((1826, 1440, 1440))
    marex_amd.tracker._check_size((1826, 720, 1440))  # cfg2 after trimming fits


def test_track_module_imports_without_gpu():
    import marex_amd.track as trk

    assert trk.tracker is marex_amd.tracker and "tracker" in marex_amd.__all__ and "TrackingError" in marex_amd.__all__
