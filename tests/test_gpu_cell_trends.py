"""GPU parity: per-cell trends (``marex_trend_stats_f64`` and ``marex_trend_select_f64`` through ``HotPath.call``, the
engine wrappers and ``marex_amd.cell_trends``) against the NumPy oracle of tests/trends_oracle.py.  The integers, the
selected slopes, the medians and the five sums are all bit-equal to the oracle (``assert_array_equal``, NaNs in the same
places): wave and workgroup tails, every step count at which the kernels change their path (LDS tile up to 64 steps for
the selection and up to 128 for the statistics, re-read above), an unaligned ``y``, every count of valid samples, ties,
slopes of both signs over sixty orders of magnitude, ranks at and past the ends, the status word, and the public path on
host and resident maps."""
import os
import sys

import numpy as np
import pytest
import torch

import marex_amd
from marex_amd.exceptions import ProcessingError
from marex_amd.xr_compat import DataArray

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import trends_cases as tc  # noqa: E402
import trends_oracle as to  # noqa: E402

pytestmark = pytest.mark.gpu
CASES = {name: (y, x) for name, y, x in tc.all_cases()}
_WANT = {}


def want_of(name):
    """The oracle's answer to a case, computed once: the statistics, a rank table and the slopes at its ranks."""
    if name not in _WANT:
        y, x = CASES[name]
        st = to.stats(y, x)
        ranks = tc.rank_table(st["n"], np.random.default_rng(len(name)))
        _WANT[name] = (st, ranks, to.select(y, x, ranks))
    return _WANT[name]


def to_dev(hot, a, misaligned=False):
    """A float64 copy of ``a`` on the device; ``misaligned``: a contiguous view that starts one element (8 bytes) past
    the start of an allocation, so it is not 16-byte aligned."""
    a = np.ascontiguousarray(a, dtype=np.float64)
    if not misaligned:
        return torch.from_numpy(a).to(hot.device)
    buf = torch.zeros(a.size + 4, dtype=torch.float64, device=hot.device)
    v = buf[1:1 + a.size].view(a.shape)
    v.copy_(torch.from_numpy(a))
    assert v.data_ptr() % 16 == 8 and v.is_contiguous()
    return v


def raw(hot, y, x, ranks, misaligned=False):
    """Both entry points on the test's own buffers: one spare canary row behind every output, the select output poisoned."""
    G, C = y.shape
    K = ranks.shape[0]
    yd, xd = to_dev(hot, y, misaligned), to_dev(hot, x)
    i32 = lambda: torch.full((2, C), -77, dtype=torch.int32, device=hot.device)  # noqa: E731
    n, s, ties = i32(), i32(), i32()
    med = torch.full((3, C), -77.0, dtype=torch.float64, device=hot.device)
    sums = torch.full((6, C), -77.0, dtype=torch.float64, device=hot.device)
    out = torch.full((K + 1, C), -77.0, dtype=torch.float64, device=hot.device)
    status = torch.zeros(2, dtype=torch.int64, device=hot.device)
    rd = torch.from_numpy(np.ascontiguousarray(ranks, dtype=np.int32)).to(hot.device)
    hot.call("marex_trend_stats_f64", yd, xd, G, C, n, s, ties, med, sums, status)
    hot.call("marex_trend_select_f64", yd, xd, G, C, rd, K, out, status)
    got = {k: v.cpu().numpy() for k, v in dict(n=n, s=s, ties=ties, med=med, sums=sums, out=out, status=status).items()}
    for k in ("n", "s", "ties", "med", "sums", "out"):
        assert (got[k][-1] == -77).all(), f"{k}: the row behind the output was written"
        got[k] = got[k][:-1]
    for k in ("n", "s", "ties"):
        got[k] = got[k][0]
    assert got["status"].tolist() == [0, 0]
    return got


def check(hot, name, misaligned=False):
    y, x = CASES[name]
    st, ranks, sel = want_of(name)
    got = raw(hot, y, x, ranks, misaligned)
    for k in ("n", "s", "ties", "med", "sums"):
        assert got[k].dtype == st[k].dtype, (name, k)
        np.testing.assert_array_equal(got[k], st[k], err_msg=f"{name} {k}")
    np.testing.assert_array_equal(got["out"], sel, err_msg=f"{name} select")


@pytest.mark.parametrize("name", [c[0] for c in tc.shape_cases()])
def test_cells_and_steps_equal_the_oracle(hot, name):
    """C in 1, 63, 64, 65, 257, 4001 at 40 steps; G in 2, 3, 40, 64, 65, 128, 129, 256 at 130 cells: missing samples, ties,
    regular and irregular x, seven ranks per cell (two groups of pivots) among them -1, P, 0, P - 1 and a repeated one."""
    check(hot, name)


@pytest.mark.parametrize("name", [c[0] for c in tc.edge_cases()])
def test_sample_counts_ties_and_slope_ranges_equal_the_oracle(hot, name):
    """A cell each without a sample, with one, with two, with the first and last only, constant, two-valued, of small
    counts, of +-0.0, of magnitudes 1e-30 .. 1e30 in both signs, of +-Inf as missing; a different pattern of missing
    steps in every lane."""
    check(hot, name)
    y, x = CASES[name]
    st, ranks, sel = want_of(name)
    P = st["n"].astype(np.int64) * (st["n"] - 1) // 2
    assert np.isnan(sel[0]).all() and np.isnan(sel[1]).all()  # the ranks -1 and P
    assert (np.isnan(sel[2]) == (P == 0)).all() and (np.isnan(sel[3]) == (P == 0)).all()  # 0 and P - 1
    np.testing.assert_array_equal(sel[4], sel[5])


@pytest.mark.parametrize("name", ["cells65", "steps129", "special5_irr"])
def test_a_y_that_is_only_8_byte_aligned(hot, name):
    check(hot, name, misaligned=True)


def test_engine_wrappers_and_their_checks(hot):
    y, x = CASES["cells257"]
    st, ranks, sel = want_of("cells257")
    yd, xd = to_dev(hot, y), to_dev(hot, x)
    got = hot.trend_stats(yd, xd)
    for k in ("n", "s", "ties", "med", "sums"):
        np.testing.assert_array_equal(got[k].cpu().numpy(), st[k], err_msg=k)
    np.testing.assert_array_equal(hot.trend_select(yd, xd, ranks).cpu().numpy(), sel)
    np.testing.assert_array_equal(hot.trend_select(yd, xd, torch.from_numpy(ranks[:1].copy()).to(hot.device)).cpu().numpy(), sel[:1])
    bad = [(yd.float(), xd, "y must be a contiguous float64"), (yd.t(), xd, "y must be a contiguous float64"),
           (yd.cpu(), xd, "y must be a contiguous float64"), (yd, xd[:-1].contiguous(), "y must be .G, C. and x .G."),
           (yd[:1], xd[:1], "2 <= G <= 256"), (yd, xd.float(), "x must be a contiguous float64")]
    for a, b, msg in bad:
        with pytest.raises(ProcessingError, match=msg):
            hot.trend_stats(a, b)
        with pytest.raises(ProcessingError, match=msg):
            hot.trend_select(a, b, ranks)
    for r in (ranks.astype(np.int64), ranks[:, :-1], ranks[0], ranks[:0]):
        with pytest.raises(ProcessingError, match="ranks must be int32"):
            hot.trend_select(yd, xd, r)
    for args in ((yd, xd, 1, 257), (yd, xd, 257, 257), (yd, xd, 40, 0), (None, xd, 40, 257)):  # the library's own guards
        with pytest.raises(ProcessingError, match="marex_trend_stats_f64"):
            hot.call("marex_trend_stats_f64", *args, got["n"], got["s"], got["ties"], got["med"], got["sums"],
                     torch.zeros(2, dtype=torch.int64, device=hot.device))


def assert_public(ds, y, x, space, alpha=0.05):
    exp = to.cell_trends(np.asarray(y, np.float64).reshape(y.shape[0], -1), x, alpha)
    assert sorted(ds.data_vars) == sorted(exp)
    for k, want in exp.items():
        got = np.asarray(ds[k].values)
        assert got.shape == tuple(space) and got.dtype == want.dtype, (k, got.shape, got.dtype)
        np.testing.assert_array_equal(got.reshape(-1), want, err_msg=k)


def test_public_grid_with_land_and_mesh(hot):
    G, ny, nx = 40, 20, 40
    y = tc.mixed(G, ny * nx, 77)
    y[:, np.random.default_rng(1).random(ny * nx) < 0.3] = np.nan  # land
    yrs = np.arange(1982, 1982 + G)
    da = DataArray(y.reshape(G, ny, nx), dims=("year", "lat", "lon"),
                   coords={"year": ("year", yrs), "lat": ("lat", np.linspace(-40, 40, ny)), "lon": ("lon", np.arange(nx) * 2.0)})
    ds = marex_amd.cell_trends(da)
    assert_public(ds, y, yrs.astype(np.float64), (ny, nx))
    assert tuple(ds["sen_slope"].dims) == ("lat", "lon") and (ds["n"].values == 0).sum() > 100
    resident = DataArray(torch.from_numpy(y.reshape(G, ny, nx)).to(hot.device), dims=("year", "lat", "lon"), coords={"year": ("year", yrs)})
    again = marex_amd.cell_trends(resident, alpha=0.01)
    assert_public(again, y, yrs.astype(np.float64), (ny, nx), 0.01)
    mesh = tc.mixed(30, 405, 78)
    xm = tc.irregular_x(30)
    assert_public(marex_amd.cell_trends(mesh, x=xm), mesh, xm, (405,))


@pytest.mark.parametrize("dtype", [np.float32, np.uint32, np.float64])
def test_public_dtypes_host_and_resident(hot, dtype):
    G, C = 25, 300
    rng = np.random.default_rng(9)
    y = rng.poisson(3.0, (G, C)).astype(dtype)
    if np.dtype(dtype).kind == "f":
        y = (y + rng.integers(0, 4, (G, C)) * 0.25).astype(dtype)
        y[rng.random((G, C)) < 0.2] = np.nan
    x = np.arange(G, dtype=np.float64)
    assert_public(marex_amd.cell_trends(y), y, x, (C,))
    t = torch.from_numpy(y.astype(np.int32) if dtype is np.uint32 else y).to(hot.device)
    assert_public(marex_amd.cell_trends(t), y, x, (C,))


def test_chained_from_local_intensity_by_year(hot):
    """The annual maps of ``local_intensity`` fed straight in: ``days`` (uint32 counts) and ``intensity_mean`` (NaN in a
    year without an extreme day), the years taken from the coordinate."""
    ny, nx, n_years = 6, 11, 7
    tv = np.arange("2001-01-01", f"{2001 + n_years}-01-01", dtype="datetime64[D]")
    T = tv.size
    rng = np.random.default_rng(4)
    anom = rng.normal(0, 1, (T, ny, nx)).astype(np.float32)
    ramp = (np.arange(T) / T)[:, None, None] * rng.uniform(-1, 1, (1, ny, nx))
    mask = (anom + ramp) > 1.6
    mask[:, 0, :3] = False  # cells that never see an extreme: intensity_mean is NaN in every year
    coords = {"time": ("time", tv), "lat": ("lat", np.arange(ny) * 1.0), "lon": ("lon", np.arange(nx) * 1.0)}
    li = marex_amd.local_intensity(DataArray(mask, dims=("time", "lat", "lon"), coords=coords),
                                   DataArray(anom, dims=("time", "lat", "lon"), coords=coords), by="year")
    years = np.asarray(li["days"].coords["year"].values)
    assert years.tolist() == list(range(2001, 2001 + n_years))
    for var in ("days", "intensity_mean"):
        v = np.asarray(li[var].values)
        assert v.shape == (n_years, ny, nx)
        ds = marex_amd.cell_trends(li, var=var)
        assert_public(ds, v, years.astype(np.float64), (ny, nx))
        assert tuple(ds["mk_p"].dims) == ("lat", "lon")
    assert np.isnan(np.asarray(li["intensity_mean"].values)).any()
