"""Heat stress on the device (``marex_group_mean_f32``, ``marex_heat_stress_f32``): every output byte for byte against the
row-loop oracle of tests/heat_stress_oracle.py, and the integers and ``dhw`` with ``==`` against the direct definition --
hand-built columns, launch edges, windows, status and refusals, the climatology kernel, the reference's SST fixture, the
composition with the other statistics, and one field whose ``dhw`` output passes 2^32 bytes."""
import os
import sys

import numpy as np
import pytest
import torch

import marex_amd
from marex_amd import zarr_io
from marex_amd.exceptions import ProcessingError
from marex_amd.xr_compat import DataArray

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import heat_stress_cases as hc  # noqa: E402
import heat_stress_oracle as ho  # noqa: E402

pytestmark = pytest.mark.gpu
F = np.float32
FIX = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "ref_fixtures")


def dev(hot, a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(hot.device)


def same_bytes(a, b, what=""):
    a, b = np.asarray(a), np.asarray(b)
    assert a.dtype == b.dtype and a.shape == b.shape, (what, a.dtype, b.dtype, a.shape, b.shape)
    if a.dtype.kind == "f":  # every NaN as one
        a, b = np.where(np.isnan(a), np.nan, a).astype(a.dtype), np.where(np.isnan(b), np.nan, b).astype(b.dtype)
    if a.tobytes() != b.tobytes():
        bad = np.argwhere(~((a == b) | ((a != a) & (b != b))))
        raise AssertionError((what, len(bad), bad[:5].tolist(), a[tuple(bad[0])], b[tuple(bad[0])]))


def engine_kw(kw):
    return dict(window=kw.get("window", 84), hotspot_min=kw.get("hmin", 1.0), steps_per_week=kw.get("spw", 7.0),
                levels=kw.get("lev", (4.0, 8.0)), grp=kw.get("grp"), G=kw.get("G", 1))


def run_dev(hot, x, m, kw, B=None, summary=True, xd=None):
    """``HotPath.heat_stress`` over the field in windows of ``B`` steps: ``(result, dhw, alert)`` on the host.  The outputs
    start as 0xCD bytes, so an element the kernel forgets shows."""
    T, C = x.shape
    ek = engine_kw(kw)
    xd = dev(hot, x) if xd is None else xd
    dd = torch.empty((T, C), dtype=torch.float32, device=hot.device)
    ad = torch.empty((T, C), dtype=torch.uint8, device=hot.device)
    dd.view(torch.uint8).fill_(0xCD), ad.fill_(0xCD)
    acc = r = None
    for a in range(0, T, B or T):
        b, lead = min(T, a + (B or T)), min(ek["window"], a)
        r = hot.heat_stress(xd[a - lead:b], m, t0=a, lead=lead, dhw=dd, alert=ad, summary=summary, acc=acc, finish=b >= T, **ek)
        acc = r["acc"]
    return r, dd.cpu().numpy(), ad.cpu().numpy()


def run_walk(x, m, kw):
    T, C = x.shape
    dhw, alert = np.zeros((T, C), F), np.zeros((T, C), np.uint8)
    return ho.walk(x, m, dhw=dhw, alert=alert, **kw), dhw, alert


def against_both(hot, x, m, kw, B=None, integers=False):
    """The device against the row loop (bytes) and the direct definition (``==``); returns the row loop's results."""
    r, dd, ad = run_dev(hot, x, m, kw, B)
    st, dhw, alert = run_walk(x, m, kw)
    same_bytes(dd, dhw, "dhw"), same_bytes(ad, alert, "alert")
    for k in ho.SUMMARY:
        same_bytes(r[k], st[k], k)
    d = ho.direct(x, m, integers=integers, **kw)
    assert np.array_equal(dd, d["dhw"], equal_nan=True) and np.array_equal(ad, d["alert"])
    for k in ho.SUMMARY:
        assert np.array_equal(r[k], d[k], equal_nan=True), k
    return st, dhw, alert


@pytest.mark.parametrize("case", hc.columns(), ids=lambda c: c["name"])
def test_hand_built_columns_alone_and_inside_a_row(hot, case):
    for x, m, at in ((case["x"][:, None], np.array([case["m"]], F), 0), (*hc.in_a_row(case), 37)):
        st, dhw, alert = against_both(hot, x, m, case["kw"])
        e = case["expect"]  # the oracle meets them in tests/test_heat_stress_host.py; here the device does, through it
        if "alert" in e:
            assert alert[:, at].tolist() == e["alert"]
        for t, v in e.get("dhw", {}).items():
            assert dhw[t, at] == F(v)


def test_a_hot_step_leaves_without_a_residue(hot):
    """One hot step beside neighbours of 1023.99 and 2^-10 in the same window of 366: after exactly ``window`` steps each is
    gone and ``dhw`` is 0.0 again, not a residue."""
    W, T = 366, 2 * 366 + 3
    d = np.zeros((T, 3), F)
    d[5, :] = [F(1.7), F(1023.99), hc.TINY]
    d[9, :] = [F(1023.99), hc.TINY, F(3.3)]
    d[200, :] = [hc.TINY, F(7.123456), F(1023.99)]
    m = np.array([0.0, 16.0, 0.0], F)
    kw = dict(window=W, hmin=hc.TINY, spw=7.0)
    st, dhw, alert = against_both(hot, (d + m).astype(F), m, kw, integers=True)
    assert (dhw[200 + W:] == 0.0).all() and (dhw[5:200 + W] > 0).all() and dhw[9 + W - 1, 0] > dhw[9 + W, 0] > 0


@pytest.mark.parametrize("window", hc.WINDOWS)
def test_launch_edges_of_time_and_window(hot, window):
    rng = np.random.default_rng(window)
    for i, T in enumerate(hc.t_edges(window)):
        C = hc.C_EDGES[(i + window) % len(hc.C_EDGES)] if window < 84 else (1, 3, 65)[i % 3]
        x, m = hc.field(T, C, rng)
        grp = rng.integers(0, 3, T).astype(np.int32)
        against_both(hot, x, m, dict(window=window, hmin=0.5, spw=7.0, lev=(0.25, 1.0, 4.0), grp=grp, G=3), integers=window >= 84)


@pytest.mark.parametrize("C", hc.C_EDGES)
def test_launch_edges_of_the_row(hot, C):
    rng = np.random.default_rng(C)
    x, m = hc.field(2 * 7 + 3, C, rng)
    against_both(hot, x, m, dict(window=7, hmin=1.0, spw=7.0, lev=(0.5, 1.0)), integers=True)
    r, dd, ad = run_dev(hot, x, m, dict(window=7, lev=(0.5, 1.0)), summary=False)  # the build without accumulators: the same fields
    st, dhw, alert = run_walk(x, m, dict(window=7, lev=(0.5, 1.0)))
    same_bytes(dd, dhw), same_bytes(ad, alert)
    assert set(r) == {"acc"}


@pytest.mark.parametrize("window", [1, 7, 84])
def test_windows_against_the_whole_field(hot, window):
    rng = np.random.default_rng(100 + window)
    T, C = 2 * window + 3, 257
    x, m = hc.field(T, C, rng)
    grp = (np.arange(T) // max(window, 2)).astype(np.int32) % 3  # changes on the boundaries of B = window and inside the others
    kw = dict(window=window, hmin=0.75, spw=3.5, lev=(1.0, 2.0), grp=grp, G=3)
    whole, dd, ad = run_dev(hot, x, m, kw)
    xd = dev(hot, x)
    for B in sorted({1, 2, max(window - 1, 1), window, window + 1, T}):
        r, d2, a2 = run_dev(hot, x, m, kw, B, xd=xd)
        same_bytes(d2, dd, ("dhw", B)), same_bytes(a2, ad, ("alert", B))
        same_bytes(r["acc"]["state"].cpu().numpy(), whole["acc"]["state"].cpu().numpy(), ("state", B))
        for k in ho.SUMMARY:
            same_bytes(r[k], whole[k], (k, B))


def _dated(x, start, shape=None):
    T = x.shape[0]
    tv = np.datetime64(start) + np.arange(T).astype("timedelta64[D]")
    if shape:
        return DataArray(x.reshape((T,) + shape), dims=("time", "lat", "lon"), coords={"time": ("time", tv)}), tv
    return DataArray(x, dims=("time", "cells"), coords={"time": ("time", tv)}), tv


def test_the_public_call_by_year_across_a_year_end_in_both_layouts(hot):
    """A grid and a mesh, host and resident input, whole and in windows: ``by="year"`` over 2001-11-20 .. 2002-02-07 with the
    climatology of its own first 60 days; every variable equals the oracle, and resident input gives resident fields."""
    rng = np.random.default_rng(12)
    T, ny, nx = 80, 5, 13
    x, _ = hc.field(T, ny * nx, rng)
    grid, tv = _dated(x, "2001-11-20", (ny, nx))
    mesh, _ = _dated(x, "2001-11-20")
    year = tv.astype("datetime64[Y]").astype(int) + 1970
    base = np.arange(T) < 60
    lab = np.where(base, tv.astype("datetime64[M]").astype(int) % 12, -1).astype(np.int32)
    cst = ho.group_walk(x, 0, lab, 12)
    mean, m, month = ho.climatology(cst["sum"], cst["cnt"])
    kw = dict(window=10, hmin=0.5, spw=7.0, lev=(0.5, 1.0, 2.0), grp=year - 2001, G=2)
    st, dhw, alert = run_walk(x, m, kw)
    names = (("dhw_max", "dhw_max"), ("time_of_dhw_max", "tmax"), ("hotspot_max", "hotspot_max"), ("alert_steps", "alert_steps"),
             ("invalid_steps", "invalid"), ("level_onset", "onset"))
    for field, B in ((grid, None), (mesh, 7), (mesh, "auto")):
        ds = marex_amd.heat_stress(field, baseline=base, by="year", window=10, hotspot_min=0.5, levels=(0.5, 1.0, 2.0), return_dhw=True,
                                   return_alert=True, block_steps=B)
        assert ds["dhw_max"].dims == ("year",) + field.dims[1:] and ds["dhw_max"].coords["year"].values.tolist() == [2001, 2002]
        same_bytes(ds["mmm"].values.reshape(-1), m, "mmm")
        for name, k in names:
            same_bytes(ds[name].values.reshape(st[k].shape), st[k], name)
        same_bytes(ds["dhw"].values.reshape(T, -1), dhw), same_bytes(ds["alert_level"].values.reshape(T, -1), alert)
    res = marex_amd.heat_stress(dev(hot, x).view(T, ny, nx), m.reshape(ny, nx), by=year - 2001, window=10, hotspot_min=0.5,
                                levels=(0.5, 1.0, 2.0), return_dhw=True, return_alert=True, block_steps=9)
    assert res["dhw"].data.device == hot.device and res["dhw"].data.dtype == torch.float32 and res["alert_level"].data.dtype == torch.uint8
    assert tuple(res["dhw"].data.shape) == (T, ny, nx) and res["dhw_max"].dims == ("group", "y", "x")
    same_bytes(res["dhw"].data.cpu().numpy().reshape(T, -1), dhw), same_bytes(res["alert_level"].data.cpu().numpy().reshape(T, -1), alert)
    for name, k in names:
        same_bytes(res[name].values.reshape(st[k].shape), st[k], name)
    cl = marex_amd.monthly_maximum_climatology(grid, baseline=base, block_steps=11)
    same_bytes(cl["monthly_mean"].values.reshape(12, -1), mean), same_bytes(cl["mmm_month"].values.reshape(-1), month)
    same_bytes(cl["monthly_count"].values.reshape(12, -1), cst["cnt"]), same_bytes(cl["mmm"].values.reshape(-1), m)


def test_a_label_out_of_range_counts_in_status_and_raises(hot):
    rng = np.random.default_rng(3)
    x, m = hc.field(6, 65, rng)
    grp = np.array([0, 1, 5, 1, -1, 0], np.int32)
    with pytest.raises(ProcessingError, match="heat_stress: 130 cells lie under a step label outside its range"):
        run_dev(hot, x, m, dict(window=2, grp=grp, G=2))
    xd = dev(hot, x)
    acc = hot.heat_stress(xd, m, window=2, grp=grp, G=2, finish=False)["acc"]  # what it did write: the other steps, as the oracle
    st = ho.walk(x, m, window=2, grp=grp, G=2)
    assert st["status"] == 130 and int(acc["status"].cpu()[0]) == 130
    same_bytes(acc["alert_steps"].cpu().numpy().view(np.uint32), st["alert_steps"])
    lab = np.array([0, -1, 12, 3, -2, 3], np.int32)
    with pytest.raises(ProcessingError, match="group_mean: 130 cells lie under a step label outside its range"):
        hot.group_mean(xd, lab, 12)
    acc = hot.group_mean(xd, lab, 12, finish=False)["acc"]
    gst = ho.group_walk(x, 0, lab, 12)
    same_bytes(acc["sum"].cpu().numpy(), gst["sum"]), same_bytes(acc["cnt"].cpu().numpy().view(np.uint32), gst["cnt"])


def test_the_library_refuses_its_argument_classes(hot):
    C, T = 8, 4
    x, m = torch.zeros((T, C), device=hot.device), torch.zeros(C, device=hot.device)
    f64, i32, u64 = torch.zeros((2, C), dtype=torch.float64, device=hot.device), torch.zeros((2, 3, C), dtype=torch.int32, device=hot.device), \
        torch.zeros(1, dtype=torch.int64, device=hot.device)
    lab, lev = torch.zeros(T, dtype=torch.int32, device=hot.device), torch.ones(2, device=hot.device)
    big = 2**31 - 1

    def gm(**kw):
        a = dict(x=x, t0=0, Tb=T, C=C, lab=lab, G=2, sum=f64, cnt=i32, status=u64)
        a.update(kw)
        hot.call("marex_group_mean_f32", *a.values())

    def hs(**kw):
        a = dict(x=x, mmm=m, t0=0, lead=0, Tb=T, C=C, window=2, hmin=1.0, spw=7.0, levels=lev, L=2, grp=lab, G=1, state=f64, dhw_max=i32,
                 tmax=i32, hotspot_max=i32, alert_steps=i32, invalid=i32, onset=i32, dhw=None, alert=None, status=u64)
        a.update(kw)
        hot.call("marex_heat_stress_f32", *a.values())

    gm(), hs(), hs(grp=None), hs(L=0, levels=None)  # the valid calls pass
    hs(**{k: None for k in ("dhw_max", "tmax", "hotspot_max", "alert_steps", "invalid", "onset")})
    for kw in (dict(x=None), dict(lab=None), dict(sum=None), dict(cnt=None), dict(status=None), dict(Tb=0), dict(C=0), dict(t0=-1), dict(G=0)):
        with pytest.raises(ProcessingError, match=r"marex_group_mean_f32 failed \(code -1\)"):
            gm(**kw)
    for kw in (dict(C=big), dict(t0=big - T), dict(t0=big)):
        with pytest.raises(ProcessingError, match=r"marex_group_mean_f32 failed \(code -4\)"):
            gm(**kw)
    for kw in (dict(x=None), dict(mmm=None), dict(state=None), dict(status=None), dict(Tb=0), dict(C=0), dict(t0=-1, lead=-1), dict(window=0),
               dict(window=367), dict(lead=1), dict(t0=5, lead=5), dict(hmin=2.0 ** -11), dict(hmin=1024.0), dict(hmin=float("nan")), dict(spw=0.0),
               dict(spw=float("inf")), dict(L=7), dict(L=-1), dict(levels=None), dict(G=0), dict(grp=None, G=2), dict(tmax=None),
               dict(onset=None), dict(dhw_max=None, tmax=None)):
        with pytest.raises(ProcessingError, match=r"marex_heat_stress_f32 failed \(code -1\)"):
            hs(**kw)
    for kw in (dict(C=big), dict(t0=big - T, lead=2), dict(t0=big, lead=2)):
        with pytest.raises(ProcessingError, match=r"marex_heat_stress_f32 failed \(code -4\)"):
            hs(**kw)
    torch.cuda.synchronize()


@pytest.mark.parametrize("magnitudes", ["kelvin", "celsius", "wide"])
def test_the_climatology_kernel_sums_in_ascending_step(hot, magnitudes):
    """Magnitudes near 300 (Kelvin), near 0 (degrees Celsius around the freezing point, both signs) and -- "wide" -- spread
    over fourteen decades.  Float64 sums of a few dozen float32 values of one magnitude are exact, whatever the order: the
    significands span fewer than 53 bits.  Only the wide case has sums that are not order-free, so there equal bytes mean the
    order of the row loop, and the test checks that another order gives other bits.  Labels -1 are skipped, month 5 has no
    sample, cells 0 and 1 get equal means in two months, NaN and Inf samples are not counted; windows of every length."""
    rng = np.random.default_rng(7 + len(magnitudes))
    T, C = 75, 257
    x = ({"kelvin": 300.0, "celsius": 0.0, "wide": 0.0}[magnitudes] + rng.normal(0, 3, (T, C))).astype(F)
    if magnitudes == "wide":
        x = (x * 10.0 ** rng.uniform(-12, 2, (T, C))).astype(F)
    x[rng.random((T, C)) < 0.08] = np.nan
    x[3, 5], x[4, 5] = np.inf, -np.inf
    lab = rng.integers(-1, 12, T).astype(np.int32)
    lab[lab == 4] = -1
    x[:, 0] = np.where(np.isin(lab, (2, 7)), F(301.5), F(290.25))  # months 3 and 8 tie above all the others
    x[:, 1] = F(1.5)                                               # every month ties: the first that has a sample
    xd = dev(hot, x)
    st = ho.group_walk(x, 0, lab, 12)
    assert not st["cnt"][4].any() and np.array_equal(st["cnt"], ho.group_direct_counts(x, lab, 12))
    whole = hot.group_mean(xd, lab, 12)
    same_bytes(whole["sum"], st["sum"], "sum"), same_bytes(whole["cnt"], st["cnt"], "cnt")
    shuffled = np.stack([np.sum(x[lab == g][::-1].astype(np.float64), axis=0, where=np.isfinite(x[lab == g][::-1])) for g in range(12)])
    assert (shuffled != st["sum"]).any() == (magnitudes == "wide")  # only there another order has other bits
    for B in (1, 2, 7, 8, 9, 74):
        acc = r = None
        for a in range(0, T, B):
            r = hot.group_mean(xd[a:a + B], lab, 12, t0=a, acc=acc, finish=a + B >= T)
            acc = r["acc"]
        same_bytes(r["sum"], st["sum"], ("sum", B)), same_bytes(r["cnt"], st["cnt"], ("cnt", B))
    ds = marex_amd.monthly_maximum_climatology(xd, months=np.where(lab >= 0, lab, 0) + 1, baseline=lab >= 0, block_steps=10)
    mean, m, month = ho.climatology(st["sum"], st["cnt"])
    same_bytes(ds["monthly_mean"].values, mean), same_bytes(ds["mmm"].values, m), same_bytes(ds["mmm_month"].values, month)
    first = int(np.flatnonzero(st["cnt"][:, 1])[0]) + 1
    assert month[0] == 3 and m[0] == F(301.5) and month[1] == first and np.isnan(mean[4]).all() and (month != 5).all()


_sst = {}


def gridded_sst():
    if not _sst:
        p = os.path.join(FIX, "sst_gridded.zarr")
        x = zarr_io.read_array(os.path.join(p, "to")).copy()
        tm = zarr_io.decode_cf_time(zarr_io.read_array(os.path.join(p, "time")), zarr_io.array_attrs(os.path.join(p, "time")))
        x[:, 1, 1] = np.nan
        lat, lon = zarr_io.read_array(os.path.join(p, "lat")), zarr_io.read_array(os.path.join(p, "lon"))
        _sst["da"] = DataArray(x, dims=("time", "lat", "lon"), coords={"time": tm, "lat": lat, "lon": lon}, name="to")
        _sst["ds"] = marex_amd.heat_stress(_sst["da"], baseline=(1982, 2001), by="year", return_dhw=True, return_alert=True)
    return _sst["da"], _sst["ds"]


def test_the_reference_sst_fixture_equals_the_oracle(hot):
    """The reference's gridded SST (14 611 days of 20 x 40 cells, Kelvin; one cell set to NaN): ``mmm`` from its first 20
    years, then the annual maps, ``dhw`` and ``alert_level``.  Bytes against the row loop, ``==`` against the definition."""
    da, ds = gridded_sst()
    x = np.asarray(da.values).reshape(da.shape[0], -1)
    tv = np.asarray(da.coords["time"].values)
    year = tv.astype("datetime64[Y]").astype(int) + 1970
    lab = np.where(year <= 2001, tv.astype("datetime64[M]").astype(int) % 12, -1).astype(np.int32)
    cst = ho.group_walk(x, 0, lab, 12)
    m = ho.climatology(cst["sum"], cst["cnt"])[1]
    same_bytes(ds["mmm"].values.reshape(-1), m, "mmm")
    G = int(year.max() - 1982 + 1)
    kw = dict(grp=(year - 1982).astype(np.int32), G=G)
    st, dhw, alert = run_walk(x, m, kw)
    d = ho.direct(x, m, integers=True, **kw)
    assert ds["dhw_max"].shape == (G, 20, 40) and ds["dhw_max"].coords["year"].values.tolist() == list(range(1982, 1982 + G))
    for name, k in (("dhw_max", "dhw_max"), ("time_of_dhw_max", "tmax"), ("hotspot_max", "hotspot_max"), ("alert_steps", "alert_steps"),
                    ("invalid_steps", "invalid"), ("level_onset", "onset"), ("dhw", "dhw"), ("alert_level", "alert")):
        got = ds[name].values.reshape((st[k] if k in st else d[k]).shape)
        same_bytes(got, {"dhw": dhw, "alert": alert}.get(k, st.get(k)), name)
        assert np.array_equal(got, d[k], equal_nan=True), name
    assert np.nanmax(ds["dhw_max"].values) > 0 and (ds["invalid_steps"].values.sum(axis=0).reshape(-1) > 0).sum() == 1
    print("fixture: largest dhw", float(np.nanmax(ds["dhw_max"].values)), "steps per alert class", ds["alert_steps"].values.sum(axis=(0, 2, 3)).tolist())


def test_the_outputs_compose_with_the_other_statistics(hot):
    da, ds = gridded_sst()
    alert = ds["alert_level"].values
    hot_mask = DataArray((alert >= 3) & (alert != 255), dims=da.dims, coords=da.coords)
    occ = marex_amd.event_occurrence(hot_mask, by="year")
    assert occ["occurrence"].shape == (20, 40) and occ["occurrence_by"].shape[1:] == (20, 40)
    assert int(occ["occurrence"].values.sum()) == int(ds["alert_steps"].values[:, 3:].sum())
    reg = marex_amd.regional_series(hot_mask)
    assert reg["cells"].shape == (da.shape[0], 1) and int(reg["cells"].values.sum()) == int(occ["occurrence"].values.sum())
    tr = marex_amd.cell_trends(ds["dhw_max"])  # the abscissae are the years; the cell without mmm is land
    assert tr["sen_slope"].shape == (20, 40) and tr["n"].values[1, 1] == 0 and (np.delete(tr["n"].values.reshape(-1), 41) == 41).all()


def test_a_field_whose_dhw_output_passes_4_gib(hot):
    """66 steps of 2^24 + 64 cells: the ``dhw`` output is 4.43 GB, so a 32-bit offset would wrap within it.  The field is built
    on the device from a short pattern; a few hundred sampled cells, the last one included, against the oracle."""
    T, C, W = 66, 2**24 + 64, 7
    assert T * C * 4 > 2**32
    rng = np.random.default_rng(64)
    col = rng.normal(0.5, 1.5, (T, 1)).astype(F)
    col[rng.integers(0, T, 3)] = np.nan
    off = rng.uniform(-1.0, 1.0, 4099).astype(F)  # a prime: the pattern does not align with the waves
    cells = torch.arange(C, device=hot.device) % 4099
    xd = dev(hot, col) + dev(hot, off)[cells][None, :]  # float32 [T, C], one rounding per element
    md = (dev(hot, rng.uniform(27.0, 29.0, 257).astype(F))[torch.arange(C, device=hot.device) % 257]).contiguous()
    xd += md[None, :]
    assert xd.dtype == torch.float32 and xd.is_contiguous() and tuple(xd.shape) == (T, C)
    dd = torch.empty((T, C), dtype=torch.float32, device=hot.device)
    ad = torch.empty((T, C), dtype=torch.uint8, device=hot.device)
    acc = None
    for a, b in ((0, 40), (40, T)):
        lead = min(W, a)
        r = hot.heat_stress(xd[a - lead:b], md, t0=a, lead=lead, window=W, hotspot_min=0.5, levels=(0.5, 1.0), dhw=dd, alert=ad, acc=acc,
                            finish=b >= T)
        acc = r["acc"]
    idx = np.unique(np.concatenate([rng.integers(0, C, 300), [0, 63, 64, 2**24 - 1, 2**24, C - 65, C - 64, C - 2, C - 1]]))
    it = torch.from_numpy(idx).to(hot.device)
    x, m = xd[:, it].cpu().numpy(), md[it].cpu().numpy()
    st, dhw, alert = run_walk(x, m, dict(window=W, hmin=0.5, lev=(0.5, 1.0)))
    same_bytes(dd[:, it].cpu().numpy(), dhw, "dhw"), same_bytes(ad[:, it].cpu().numpy(), alert, "alert")
    for k in ho.SUMMARY:
        same_bytes(r[k][..., idx], st[k], k)
    assert (dhw > 0).any() and (alert >= 3).any()
