"""GPU parity: occurrence statistics (``marex_occurrence_u8`` / ``marex_occurrence_i32`` through ``HotPath.call``,
``HotPath.occurrence`` and ``marex_amd.event_occurrence``) against the NumPy oracle of tests/occurrence_oracle.py.  Every
output is an integer count or one float64 division of two of them, so everything compares with ``array_equal``: shapes and
types, grid and mesh classes, step labels, the state carried across time windows, selected IDs, the guards, 64-bit row
offsets, and the public API on the reference's fixture stores."""
import os
import sys

import numpy as np
import pytest
import torch

import marex_amd
from marex_amd import zarr_io
from marex_amd.exceptions import DataValidationError, ProcessingError
from marex_amd.xr_compat import DataArray

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import occurrence_oracle as oo  # noqa: E402

pytestmark = pytest.mark.gpu
FIX = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "ref_fixtures")


def field(T, C, dtype, seed=0, negatives=True):
    """IDs 0..6 with about 40 % of the cells present and, for int32, a few negative cells; column 0 is present throughout."""
    rng = np.random.default_rng(seed + 1000 * T + C)
    x = np.where(rng.random((T, C)) < 0.4, rng.integers(1, 7, (T, C)), 0).astype(np.int32)
    if dtype == np.int32 and negatives:
        x[rng.random((T, C)) < 0.02] = -3
    x[:, 0] = 1
    return x.astype(dtype)


def to_dev(hot, a, misaligned=False):
    """A copy of ``a`` on the device; ``misaligned``: a contiguous view that starts one byte past an aligned address."""
    a = np.array(a, order="C")
    if not misaligned:
        return torch.from_numpy(a).to(hot.device)
    assert a.dtype == np.uint8
    buf = torch.zeros(a.size + 16, dtype=torch.uint8, device=hot.device)
    v = buf[1:1 + a.size].view(a.shape)
    v.copy_(torch.from_numpy(a))
    assert v.data_ptr() % 4 == 1 and v.is_contiguous()
    return v


def tab(hot, v):
    return None if v is None else torch.from_numpy(np.asarray(v, np.int32)).to(hot.device)


def kernel(hot, x, t0=0, match=0, grp=None, G=1, sgrp=None, G2=0, cls=None, R=0, runs=True, bufs=None):
    """One library call on buffers of the test's own (zeroed once, one spare group behind cell_cnt and sec_cnt as a canary)."""
    Tb, C = x.shape
    if bufs is None:
        bufs = {"cell_cnt": torch.zeros((G + 1, C), dtype=torch.int32, device=hot.device),
                "runs": torch.zeros((3, C), dtype=torch.int32, device=hot.device) if runs else None,
                "sec_cnt": torch.zeros((G2 + 1, R), dtype=torch.int64, device=hot.device) if sgrp is not None else None,
                "status": torch.zeros(2, dtype=torch.int64, device=hot.device),
                "grp": tab(hot, grp), "sgrp": tab(hot, sgrp), "cls": tab(hot, cls)}
    fn = "marex_occurrence_i32" if x.dtype == torch.int32 else "marex_occurrence_u8"
    hot.call(fn, x, t0, Tb, C, match, bufs["grp"], G, bufs["sgrp"], G2, bufs["cls"], R, bufs["runs"], bufs["cell_cnt"],
             bufs["sec_cnt"], bufs["status"])
    return bufs


def read(bufs):
    out = {k: (None if bufs[k] is None else bufs[k].cpu().numpy()) for k in ("cell_cnt", "runs", "sec_cnt", "status")}
    assert not out["cell_cnt"][-1].any() and (out["sec_cnt"] is None or not out["sec_cnt"][-1].any())  # the canaries
    out["cell_cnt"] = out["cell_cnt"][:-1].view(np.uint32)
    out["runs"] = None if out["runs"] is None else out["runs"].view(np.uint32)
    out["sec_cnt"] = None if out["sec_cnt"] is None else out["sec_cnt"][:-1].view(np.uint64)
    return out


def check(hot, x_h, misaligned=False, match=0, grp=None, G=1, sgrp=None, G2=0, cls=None, R=0):
    """The kernel on ``x_h`` against the oracle, twice: equal bytes, inputs unmodified."""
    outs = []
    for _ in range(2):
        x = to_dev(hot, x_h, misaligned)
        r = read(kernel(hot, x, 0, match, grp, G, sgrp, G2, cls, R))
        assert np.array_equal(x.cpu().numpy(), x_h)
        outs.append(b"".join(v.tobytes() for v in r.values() if v is not None))
    assert outs[0] == outs[1]
    what = (x_h.shape, x_h.dtype, misaligned, match)
    assert np.array_equal(r["cell_cnt"], oo.cell_counts(x_h, grp, G, match)), what
    assert np.array_equal(r["runs"], oo.run_stats(x_h, match)), what
    if sgrp is not None:
        assert np.array_equal(r["sec_cnt"], oo.section_counts(x_h, sgrp, G2, cls, R, match)), what
    st = oo.status(x_h, grp, G, sgrp, G2, cls, R, match)
    assert r["status"].tolist() == st, what
    return r


def mesh_classes(C, R, seed=3):
    """A shuffled class table: some cells at -1, one at R (both counted nowhere), class 1 with a single cell, class 2 empty."""
    rng = np.random.default_rng(seed)
    cls = rng.integers(3, R, C).astype(np.int32)
    cls[rng.random(C) < 0.1] = -1
    cls[0], cls[C // 2], cls[C - 1] = 0, 1, R
    assert (cls == 1).sum() == 1 and not (cls == 2).any() and (cls == -1).any()
    return cls


SHAPES = [(7, 5), (9, 333), (6, 693), (5, 4200)]
KINDS = [(np.uint8, False), (np.uint8, True), (np.int32, False)]
KIND_IDS = ["u8", "u8-misaligned", "i32"]


@pytest.mark.parametrize("dtype,misaligned", KINDS, ids=KIND_IDS)
@pytest.mark.parametrize("shape", SHAPES + [(6, 700)], ids=lambda s: f"{s[0]}x{s[1]}")
def test_shapes_and_types_equal_the_oracle(hot, shape, dtype, misaligned):
    """Fewer cells than a wave, a ragged last wave, a ragged last workgroup, several workgroups; uint8 at C = 693 (one cell
    per lane) and at C = 700 and 4200 (four cells per lane; the misaligned view falls back to one), int32 at the same."""
    T, C = shape
    x = field(T, C, dtype)
    grp = np.arange(T, dtype=np.int32) % 4        # cyclic, G = 5: group 4 has no step
    cls = mesh_classes(C, 9) if C >= 64 else (np.arange(C, dtype=np.int32) - 1)
    R = 9 if C >= 64 else C - 2
    r = check(hot, x, misaligned, 0, grp, 5, np.arange(T, dtype=np.int32), T, cls, R)
    assert not r["cell_cnt"][4].any() and r["cell_cnt"][0][0] == len(range(0, T, 4)) and r["runs"][2][0] == T
    if dtype == np.int32:
        assert r["status"][0] == (x < 0).sum() > 0


@pytest.mark.parametrize("dtype,misaligned", KINDS, ids=KIND_IDS)
@pytest.mark.parametrize("nx", [24, 100, 128])
def test_grid_classes(hot, nx, dtype, misaligned):
    """The classes are the grid rows: a wave spans three rows (nx = 24), the boundaries fall inside waves at varying lanes
    (100), the classes of a wave are uniform (128)."""
    T, ny = 6, 11
    x = field(T, ny * nx, dtype)
    cls = np.repeat(np.arange(ny, dtype=np.int32), nx)
    months = np.array([0, 0, 1, 1, 1, 3], np.int32)
    r = check(hot, x, misaligned, 0, None, 1, months, 4, cls, ny)
    assert np.array_equal(r["sec_cnt"][0], (x[:2].reshape(2, ny, nx) > 0).sum(axis=(0, 2))) and not r["sec_cnt"][2].any()


@pytest.mark.parametrize("dtype,misaligned", KINDS, ids=KIND_IDS)
@pytest.mark.parametrize("C", [693, 700])
def test_mesh_classes(hot, C, dtype, misaligned):
    T, R = 6, 70  # more distinct classes in a wave than a grid ever has
    x = field(T, C, dtype)
    x[:, C // 2] = 1       # the single cell of class 1 is present throughout
    cls = mesh_classes(C, R)
    r = check(hot, x, misaligned, 0, None, 1, np.zeros(T, np.int32), 1, cls, R)
    assert r["sec_cnt"][0][1] == T and r["sec_cnt"][0][2] == 0
    assert r["sec_cnt"].sum() == (x[:, (cls >= 0) & (cls < R)] > 0).sum()


LABELS = {"year": [0, 0, 0, 1, 1, 1, 2, 2, 2], "season": [0, 1, 2, 3, 0, 1, 2, 3, 0], "every row": [0, 1, 0, 1, 0, 1, 0, 1, 0],
          "unused group": [0, 0, 3, 3, 3, 0, 0, 3, 3], "none": None}


@pytest.mark.parametrize("dtype", [np.uint8, np.int32], ids=["u8", "i32"])
@pytest.mark.parametrize("name", list(LABELS))
def test_step_labels(hot, name, dtype):
    """Contiguous, cyclic and alternating labels, G = 1 with a null table, a group no step uses (it stays 0), and one
    section group per step (G2 = T)."""
    T, C = 9, 700
    x = field(T, C, dtype)
    grp = LABELS[name]
    G = 1 if grp is None else 4
    cls = np.repeat(np.arange(7, dtype=np.int32), 100)
    sgrp = np.arange(T, dtype=np.int32) if name != "season" else np.asarray(LABELS["season"], np.int32)
    r = check(hot, x, False, 0, grp, G, sgrp, T if name != "season" else 4, cls, 7)
    if name == "unused group":
        assert not r["cell_cnt"][1].any() and not r["cell_cnt"][2].any() and r["cell_cnt"][3].any()
    # the same through the engine: fresh buffers are poisoned there, so the zeroing shows
    from marex_amd.engine import HotPath

    assert HotPath.POISON
    clean = np.where(x.astype(np.int64) < 0, 0, x).astype(dtype)
    e = hot.occurrence(to_dev(hot, clean), grp=grp, G=G, sgrp=sgrp, G2=int(sgrp.max()) + 1, cls=cls, R=7)
    assert np.array_equal(e["cell_cnt"], oo.cell_counts(clean, grp, G)) and e["cell_cnt"].dtype == np.uint32
    assert np.array_equal(e["runs"], oo.run_stats(clean)) and e["runs"].dtype == np.uint32
    assert np.array_equal(e["sec_cnt"], oo.section_counts(clean, sgrp, int(sgrp.max()) + 1, cls, 7)) and e["sec_cnt"].dtype == np.uint64


def carry_field(T, C, dtype):
    """For every boundary s = 1 .. T - 1: column 2 s - 1 holds a run ending exactly at s - 1, column 2 s one starting
    exactly at s; column 0 is one run crossing every boundary; the rest is random."""
    x = field(T, C, dtype, seed=7)
    for s in range(1, T):
        x[:, 2 * s - 1] = (np.arange(T) < s) * 2
        x[:, 2 * s] = (np.arange(T) >= s) * 3
    return x


@pytest.mark.parametrize("dtype,misaligned", KINDS, ids=KIND_IDS)
def test_windows_carry_the_state(hot, dtype, misaligned):
    """T = 9: every split into two windows, and the split into nine, gives the bytes of the single call -- run_state,
    cell_cnt and sec_cnt; the labels change exactly at the boundary of the split."""
    T, C = 9, 700
    x_h = carry_field(T, C, dtype)
    cls = np.repeat(np.arange(7, dtype=np.int32), 100)
    for s in range(1, T):
        lab = (np.arange(T) >= s).astype(np.int32)
        args = (0, lab, 2, lab, 2, cls, 7)
        whole = read(kernel(hot, to_dev(hot, x_h, misaligned), 0, *args))
        assert np.array_equal(whole["runs"], oo.run_stats(x_h)) and np.array_equal(whole["cell_cnt"], oo.cell_counts(x_h, lab, 2))
        assert whole["runs"][:, 2 * s - 1].tolist() == [0, 1, s] and whole["runs"][:, 2 * s].tolist() == [T - s, 1, T - s]
        assert whole["runs"][:, 0].tolist() == [T, 1, T]
        for cuts in ([0, s, T], list(range(T + 1))):
            if s > 1 and len(cuts) > 3:
                continue  # the split into nine once
            bufs = None
            for a, b in zip(cuts[:-1], cuts[1:]):
                bufs = kernel(hot, to_dev(hot, x_h[a:b], misaligned), a, *args, bufs=bufs)
            got = read(bufs)
            for k in ("cell_cnt", "runs", "sec_cnt", "status"):
                assert got[k].tobytes() == whole[k].tobytes(), (s, cuts, k)


@pytest.mark.parametrize("dtype,misaligned", KINDS, ids=KIND_IDS)
def test_selected_ids(hot, dtype, misaligned):
    T, C = 9, 700
    x = field(T, C, dtype)
    cls = np.repeat(np.arange(7, dtype=np.int32), 100)
    for match in (4, 9, 1):  # a selected ID, one absent from the field, ID 1
        r = check(hot, x, misaligned, match, None, 1, np.zeros(T, np.int32), 1, cls, 7)
        assert np.array_equal(r["cell_cnt"][0], (x == match).sum(0))
    ids = [4, 9, 1]
    clean = np.where(x.astype(np.int64) < 0, 0, x).astype(dtype)
    e = hot.occurrence(to_dev(hot, clean, misaligned), event_ids=ids)
    assert np.array_equal(e["dur"], np.stack([(clean == k).sum(0) for k in ids])) and e["dur"].dtype == np.uint32
    assert np.array_equal(e["cell_cnt"][0], (clean > 0).sum(0))


def test_guards(hot):
    T, C = 6, 693
    x = field(T, C, np.int32)
    neg = int((x < 0).sum())
    assert neg > 0
    with pytest.raises(DataValidationError, match="Object IDs must be non-negative"):
        marex_amd.event_occurrence(x)
    with pytest.raises(DataValidationError, match="Object IDs must be non-negative"):
        marex_amd.event_occurrence(to_dev(hot, x), event_ids=[2], block_steps=4)
    with pytest.raises(DataValidationError, match=f"{neg} negative cells"):
        hot.occurrence(to_dev(hot, x), event_ids=[2, 3])
    # a label >= G handed straight to the engine: counted, nothing corrupted (read() checks the spare group behind the outputs)
    clean = np.maximum(x, 0)
    grp = np.array([0, 1, 2, 7, -1, 1], np.int32)
    sgrp = np.array([0, 5, 0, 0, -4, 0], np.int32)
    cls = np.repeat(np.arange(7, dtype=np.int32), 99)
    r = check(hot, clean, False, 0, grp, 3, sgrp, 1, cls, 7)
    lost = int((clean[3] > 0).sum() + (clean[4] > 0).sum() + (clean[1] > 0).sum() + (clean[4] > 0).sum())
    assert r["status"].tolist() == [0, lost]
    with pytest.raises(ProcessingError, match=f"occurrence: {int((clean[3] > 0).sum() + (clean[4] > 0).sum())} present cells lie under"):
        hot.occurrence(to_dev(hot, clean), grp=grp, G=3)
    for bad in (lambda: hot.occurrence(to_dev(hot, clean).to(torch.int64)), lambda: hot.occurrence(to_dev(hot, clean).t()),
                lambda: hot.occurrence(to_dev(hot, clean), t0=-1), lambda: hot.occurrence(to_dev(hot, clean), G=2),
                lambda: hot.occurrence(to_dev(hot, clean), grp=grp[:3], G=8), lambda: hot.occurrence(to_dev(hot, clean), sgrp=sgrp, G2=6),
                lambda: hot.occurrence(to_dev(hot, clean), cls=cls[:-1], sgrp=sgrp, G2=6, R=7),
                lambda: hot.occurrence(to_dev(hot, clean), event_ids=[0]),
                lambda: hot.occurrence(to_dev(hot, clean), G=1, acc=hot.occurrence(to_dev(hot, clean), grp=grp, G=8, finish=False)["acc"])):
        with pytest.raises(ProcessingError):
            bad()


@pytest.mark.parametrize("fn,dtype", [("marex_occurrence_u8", np.uint8), ("marex_occurrence_i32", np.int32)])
def test_return_codes(hot, fn, dtype):
    T, C = 6, 700
    x = to_dev(hot, field(T, C, dtype, negatives=False))
    lab, cls = tab(hot, np.zeros(T, np.int32)), tab(hot, np.zeros(C, np.int32))
    cnt = torch.zeros((1, C), dtype=torch.int32, device=hot.device)
    runs = torch.zeros((3, C), dtype=torch.int32, device=hot.device)
    sec = torch.zeros((1, 1), dtype=torch.int64, device=hot.device)
    st = torch.zeros(2, dtype=torch.int64, device=hot.device)
    ok = (x, 0, T, C, 0, lab, 1, lab, 1, cls, 1, runs, cnt, sec, st)
    names = ("x", "t0", "Tb", "C", "match", "grp", "G", "sgrp", "G2", "cls", "R", "run_state", "cell_cnt", "sec_cnt", "status")

    def with_(**kw):
        return tuple(kw.get(k, v) for k, v in zip(names, ok))

    cases = [(-4, with_(C=2**31 - 1)), (-4, with_(C=2**40)), (-4, with_(Tb=2**31 - 1)), (-4, with_(t0=2**31 - 1 - T)),
             (-4, with_(t0=2**40)), (-1, with_(Tb=0)), (-1, with_(C=0)), (-1, with_(t0=-1)), (-1, with_(match=-1)), (-1, with_(G=0)),
             (-1, with_(grp=None, G=2)), (-1, with_(G2=0)), (-1, with_(R=0)), (-1, with_(sgrp=None)), (-1, with_(cls=None)),
             (-1, with_(sec_cnt=None)), (-1, with_(x=None)), (-1, with_(cell_cnt=None)), (-1, with_(status=None))]
    for code, args in cases:  # refused by the library before any launch
        with pytest.raises(ProcessingError, match=rf"{fn} failed \(code {code}\)"):
            hot.call(fn, *args)
    hot.sync()
    assert not cnt.any() and not runs.any() and not sec.any() and not st.any()
    for args in (ok, with_(grp=None), with_(run_state=None), with_(sgrp=None, cls=None, sec_cnt=None, G2=0, R=0)):  # all nullable
        hot.call(fn, *args)
    hot.sync()
    assert int(cnt.sum().item()) == 4 * int((x > 0).sum().item()) and not st.any()


def test_row_offsets_past_32_bits(hot):
    """A uint8 field of 5 x (2^30 - 3) cells: the rows 2 .. 4 start near 2^31, past 2^31 and near 2^32 bytes.  No run
    statistics, so the field and the counts take about 10 GB."""
    T, C = 5, 2**30 - 3
    x = torch.zeros((T, C), dtype=torch.uint8, device=hot.device)
    cells = [(2, 0), (2, 5), (2, 6), (2, C - 1), (3, 0), (3, 2**29), (3, C - 1), (4, 0), (4, 11), (4, 12), (4, 2**29), (4, C - 1)]
    for t, c in cells:
        x[t, c] = 1
    r = hot.occurrence(x, runs=False, finish=False)["acc"]
    cnt = r["cell_cnt"]
    assert int(cnt.sum(dtype=torch.int64).item()) == len(cells) and r["status"].cpu().tolist() == [0, 0]
    want = {}
    for _, c in cells:
        want[c] = want.get(c, 0) + 1
    for c, n in want.items():
        assert int(cnt[0, c].item()) == n, c
    assert int(x.sum(dtype=torch.int64).item()) == len(cells)
    del x, cnt, r
    torch.cuda.empty_cache()


# ------------------------------------------------------------------ the public API on the reference's data
def same(a, b):
    assert list(a.data_vars) == list(b.data_vars)
    for k in a.data_vars:
        assert np.asarray(a[k].values).tobytes() == np.asarray(b[k].values).tobytes(), k
        assert tuple(a[k].dims) == tuple(b[k].dims)


def host_and_device(hot, da, **kw):
    """The call on the host array and on a resident copy, whole and in windows: one Dataset."""
    t = torch.from_numpy(np.ascontiguousarray(da.values)).to(hot.device)
    dev = DataArray(t, dims=tuple(da.dims), coords={k: (tuple(v.dims), np.asarray(v.values)) for k, v in da.coords.items()})
    first = None
    for f in (da, dev):
        for b in (None, 7, "auto"):
            ds = marex_amd.event_occurrence(f, block_steps=b, **kw)
            if first is None:
                first = ds
            else:
                same(first, ds)
    return first


_fx = {}


def gridded():
    if not _fx:
        p = os.path.join(FIX, "extremes_gridded.zarr")
        ev = zarr_io.read_array(os.path.join(p, "extreme_events")).astype(bool)
        tm = zarr_io.decode_cf_time(zarr_io.read_array(os.path.join(p, "time")), zarr_io.array_attrs(os.path.join(p, "time")))
        lat, lon = zarr_io.read_array(os.path.join(p, "lat")), zarr_io.read_array(os.path.join(p, "lon"))
        mask = zarr_io.read_array(os.path.join(p, "mask")).astype(bool)
        tm = np.asarray(tm).astype("datetime64[ns]")
        _fx.update(ev=ev, tm=tm, lat=lat, lon=lon, mask=mask,
                   da=DataArray(ev, dims=("time", "lat", "lon"), coords={"time": ("time", tm), "lat": ("lat", lat), "lon": ("lon", lon)}))
    return _fx


def group_mean(p, lab, G):
    """``p[lab == g].mean(axis=0)`` per group; NaN for a group without a step (what xarray's groupby leaves out)."""
    out = np.full((G,) + p.shape[1:], np.nan)
    for g in range(G):
        if (lab == g).any():
            out[g] = p[lab == g].mean(axis=0)
    return out


def test_frequency_and_seasons_on_the_reference_extremes(hot):
    f = gridded()
    ev, tm = f["ev"], f["tm"]
    T = ev.shape[0]
    ds = host_and_device(hot, f["da"], by="season")
    assert np.array_equal(ds["frequency"].values, ev.mean(axis=0)) and ds["frequency"].values.dtype == np.float64
    assert np.array_equal(ds["occurrence"].values, ev.sum(axis=0)) and tuple(ds["frequency"].dims) == ("lat", "lon")
    month = tm.astype("datetime64[M]").astype(int) % 12 + 1
    lab = np.array([{12: 0, 1: 0, 2: 0, 3: 2, 4: 2, 5: 2, 6: 1, 7: 1, 8: 1}.get(int(m), 3) for m in month])
    assert np.array_equal(ds["frequency_by"].values, group_mean(ev, lab, 4), equal_nan=True)
    assert ds["steps_by"].values.tolist() == np.bincount(lab, minlength=4).tolist() and ds["steps_by"].values.sum() == T
    runs = oo.run_stats(ev[:, 90, :])
    assert np.array_equal(ds["n_runs"].values[90], runs[1]) and np.array_equal(ds["longest_run"].values[90], runs[2])
    assert np.array_equal(np.isnan(ds["mean_run"].values), ev.sum(axis=0) == 0)


@pytest.mark.parametrize("zonal_by", ["month", "dayofyear"])
def test_zonal_presence_on_the_reference_extremes(hot, zonal_by):
    f = gridded()
    ev, tm = f["ev"], f["tm"]
    nx = ev.shape[2]
    ds = host_and_device(hot, f["da"], zonal=True, zonal_by=zonal_by)
    if zonal_by == "month":
        mi = tm.astype("datetime64[M]").astype(int)
        lab, G2 = mi - mi.min(), int(mi.max() - mi.min()) + 1
    else:
        doy = (tm.astype("datetime64[D]") - tm.astype("datetime64[Y]").astype("datetime64[D]")).astype(int) + 1
        vals, lab = np.unique(doy, return_inverse=True)
        G2 = vals.size
        assert np.array_equal(ds["presence"].coords["zonal_dayofyear"].values, vals)
    cells = np.zeros((G2, ev.shape[1]), np.uint64)
    for t in range(ev.shape[0]):
        cells[lab[t]] += ev[t].sum(axis=1).astype(np.uint64)
    steps = np.bincount(lab, minlength=G2)
    assert np.array_equal(ds["presence_cells"].values, cells) and ds["presence_cells"].values.dtype == np.uint64
    assert np.array_equal(ds["presence"].values, oo.ratio(cells, steps[:, None] * nx), equal_nan=True)
    assert ds["class_cells"].values.tolist() == [nx] * ev.shape[1] and tuple(ds["presence"].dims) == ("zonal_" + zonal_by, "lat")
    # the notebook's mean of means agrees to rounding
    zm = group_mean(ev.mean(axis=2), lab, G2)
    assert np.allclose(ds["presence"].values, zm, rtol=1e-12, atol=0, equal_nan=True)


def test_local_durations_of_the_tracked_reference_events(hot):
    f = gridded()
    trk = marex_amd.tracker(f["da"], DataArray(f["mask"], dims=("lat", "lon")), R_fill=4, T_fill=2, area_filter_quartile=0.5,
                            allow_merging=False, quiet=True)
    events = trk.run()
    ids = np.asarray(events["ID_field"].values)
    N = int(ids.max())
    assert N >= 5 and ids.dtype == np.int32
    dur = np.array([(ids == k).any(axis=(1, 2)).sum() for k in range(1, N + 1)])
    longest = (np.argsort(-dur, kind="stable")[:5] + 1).tolist()
    ds = host_and_device(hot, events["ID_field"], event_ids=longest)
    assert np.array_equal(ds["local_duration"].values, np.stack([(ids == k).sum(axis=0) for k in longest]))
    assert np.array_equal(ds["occurrence"].values, (ids > 0).sum(axis=0)) and ds["local_duration"].values.dtype == np.uint32
    assert np.asarray(ds["local_duration"].coords["event"].values).tolist() == longest
    same(ds, trk.event_occurrence(events, event_ids=longest, block_steps=7))


@pytest.mark.parametrize("edges", [np.arange(-90.0, 91.0, 1.0), 39.0 + 0.05 * np.arange(21)], ids=["1 degree", "0.05 degrees"])
def test_latitude_bins_on_the_reference_mesh(hot, edges):
    """1-degree bins as in the notebooks; the store's cells lie between 39 and 40 degrees north, so finer bins as well."""
    p = os.path.join(FIX, "extremes_unstructured.zarr")
    ev = zarr_io.read_array(os.path.join(p, "extreme_events")).astype(bool)
    lat = zarr_io.read_array(os.path.join(p, "lat"))
    T, C = ev.shape
    R = edges.size - 1
    da = DataArray(ev, dims=("time", "ncells"), coords={"time": ("time", np.arange(T)), "lat": ("ncells", lat)})
    ds = host_and_device(hot, da, zonal=True, zonal_by="step", lat=lat, lat_bins=edges)
    la = np.asarray(lat, np.float64)
    cells = np.zeros((T, R), np.uint64)
    size = np.zeros(R, np.int64)
    for r in range(R):  # the bin rule restated: right-closed intervals
        inside = (la > edges[r]) & (la <= edges[r + 1])
        size[r] = inside.sum()
        cells[:, r] = ev[:, inside].sum(axis=1)
    assert np.array_equal(ds["presence_cells"].values, cells) and np.array_equal(ds["class_cells"].values, size)
    assert np.array_equal(ds["presence"].values, oo.ratio(cells, size[None, :]), equal_nan=True)
    assert np.array_equal(ds["frequency"].values, ev.mean(axis=0)) and tuple(ds["occurrence"].dims) == ("ncells",)
    assert cells.sum() == ev.sum() > 0 and (size == 0).any() == bool(np.isnan(ds["presence"].values).any())
    assert (size > 0).sum() == (1 if R == 180 else 20)
