"""GPU parity: per-cell Hobday events (``marex_cell_events_u8`` through ``HotPath.call``, ``HotPath.cell_events`` and
``marex_amd.cell_events``) against the two NumPy restatements of tests/cell_events_oracle.py.  Against the row loop of the
state machine every output -- counts, sums, maxima, the mask, the records -- compares byte for byte; against the direct
definition the integers and maxima are exact and a sum lies within the bound of sequential summation.  Shapes on both
layouts, hand-built columns, the state carried across windows, non-finite anomalies, identities with ``event_occurrence``
and ``local_intensity``, labels by the start step, the guards, and mask addresses past 32 bits."""
import math
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
import cell_events_oracle as co  # noqa: E402

pytestmark = pytest.mark.gpu
FIX = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "ref_fixtures")
F = np.float32
NAN, INF = np.nan, np.inf
RULES = [(1, 0), (2, 0), (3, 1), (5, 2), (2, 4)]
ACC = ("events", "event_days", "duration_max", "sum", "vmax", "invalid")
REC = ("off", "start", "end", "vmax", "tmax", "sum", "invalid")


def col(s):
    return np.array([ch == "#" for ch in s], np.uint8)


def to_dev(hot, a, misaligned=False):
    """A copy of ``a`` on the device; ``misaligned``: a contiguous uint8 view that starts one byte past an aligned address."""
    a = np.array(a, order="C")
    if not misaligned:
        return torch.from_numpy(a).to(hot.device)
    assert a.dtype == np.uint8
    buf = torch.zeros(a.size + 16, dtype=torch.uint8, device=hot.device)
    v = buf[1:1 + a.size].view(a.shape)
    v.copy_(torch.from_numpy(a))
    assert v.data_ptr() % 4 == 1 and v.is_contiguous()
    return v


def random_case(T, C, dens, seed=0, exact=False):
    rng = np.random.default_rng(seed + 1000 * T + C + int(100 * dens))
    x = (rng.random((T, C)) < dens).astype(np.uint8)
    if exact:
        a = (rng.integers(-8192, 8193, (T, C)) / 1024).astype(F)  # multiples of 2^-10 in [-8, 8]
    else:
        a = (rng.normal(0.5, 2.0, (T, C)) * 10.0 ** rng.integers(-6, 7, (T, C))).astype(F)
        a[rng.random((T, C)) < 0.03] = NAN
    return x, a


def device_run(hot, x, a, D, gap, grp=None, G=1, B=None, misaligned=False, records=True):
    """Both passes of the engine over windows of ``B`` steps: the host results, ``mask`` and ``rec``."""
    T, C = x.shape
    B = T if B is None else B
    mask = torch.empty((T, C), dtype=torch.uint8, device=hot.device).fill_(0xCD)
    kw = dict(min_duration=D, max_gap=gap, grp=grp, G=G)
    r = acc = None
    for t0 in range(0, T, B):
        r = hot.cell_events(to_dev(hot, x[t0:t0 + B], misaligned), None if a is None else to_dev(hot, a[t0:t0 + B]), t0=t0, mask=mask,
                            acc=acc, finish=t0 + B >= T, **kw)
        acc = r["acc"]
    r["mask"] = mask.cpu().numpy()
    if records:
        rec = hot.cell_event_records(acc)
        r2 = acc = None
        for t0 in range(0, T, B):
            r2 = hot.cell_events(to_dev(hot, x[t0:t0 + B], misaligned), None if a is None else to_dev(hot, a[t0:t0 + B]), t0=t0,
                                 records=rec, acc=acc, finish=t0 + B >= T, **kw)
            acc = r2["acc"]
        r["rec"] = r2["rec"]
    return r


def assert_same_as_walk(got, x, a, D, gap, grp=None, G=1, what=None):
    """Every output of the device equals the row loop of the state machine, byte for byte."""
    mask = np.zeros(x.shape, np.uint8)
    want = co.finish(co.walk(x, a, 0, D, gap, grp, G, mask))
    assert got["mask"].tobytes() == mask.tobytes(), what
    for k in ACC[:3 if a is None else 6]:
        assert got[k].dtype == want[k].dtype and got[k].tobytes() == want[k].tobytes(), (k, what)
    for k in REC[:3 if a is None else 7]:
        assert got["rec"][k].dtype == want["rec"][k].dtype and got["rec"][k].tobytes() == want["rec"][k].tobytes(), (k, what)
    return want


@pytest.mark.parametrize("C", [1, 3, 64, 700, 1028])
@pytest.mark.parametrize("T", [1, 7, 23])
def test_shapes_rules_and_densities_equal_the_state_machine(hot, T, C):
    """C = 3 and 1028: one cell per lane (1028 is a multiple of 4, its base is misaligned), with several workgroups; 64 and
    700: one wave and a ragged last block, and without anomalies four cells per lane (with them the library takes one)."""
    events = 0
    for D, gap in RULES:
        for dens in (0.3, 0.6, 0.85):
            x, a = random_case(T, C, dens)
            grp = (np.arange(T) // 3 % 4).astype(np.int32)
            mis = C in (3, 1028)
            what = (T, C, D, gap, dens)
            w = assert_same_as_walk(device_run(hot, x, a, D, gap, grp, 5, misaligned=mis), x, a, D, gap, grp, 5, what)
            events += int(w["events"].sum())
            assert not w["events"][4].any()  # a group no step uses
            assert_same_as_walk(device_run(hot, x, None, D, gap, grp, 5, misaligned=mis), x, None, D, gap, grp, 5, what)
            if C == 1028:  # aligned: four cells per lane without anomalies
                assert_same_as_walk(device_run(hot, x, None, D, gap, grp, 5), x, None, D, gap, grp, 5, what)
    assert events > 0 or T < 5


HAND = {"a run of D - 1": ("....##.............", []),
        "a run of exactly D": ("....###............", [(4, 6)]),
        "gap of G joins": ("###..###...........", [(0, 7)]),
        "gap of G + 1 does not": ("###...###..........", [(0, 2), (6, 8)]),
        "a short run in a gap of G + 2 bridges nothing": (".###.##.###........", [(1, 3), (8, 10)]),
        "a chain of three joins": ("###.####..###.###..", [(0, 16)]),
        "a run at step 0": ("####...............", [(0, 3)]),
        "an event open at T - 1": ("..........###..####", [(10, 18)]),
        "all present": ("###################", [(0, 18)]),
        "all absent": ("...................", [])}


def test_hand_built_columns(hot):
    D, gap, T = 3, 2, 19
    x = np.stack([col(s) for s, _ in HAND.values()] * 2, 1)  # twenty columns: four cells per lane
    rng = np.random.default_rng(5)
    a = rng.integers(-8192, 8193, x.shape).astype(F) / F(1024)
    plain = device_run(hot, x, None, D, gap)  # without anomalies: four cells per lane
    assert_same_as_walk(plain, x, None, D, gap)
    for mis in (False, True):
        got = device_run(hot, x, a, D, gap, misaligned=mis)
        assert_same_as_walk(got, x, a, D, gap)
        assert all(got["rec"][k].tobytes() == plain["rec"][k].tobytes() for k in REC[:3])
        for c, (name, (s, ev)) in enumerate(HAND.items()):
            lo, hi = got["rec"]["off"][c], got["rec"]["off"][c + 1]
            assert list(zip(got["rec"]["start"][lo:hi].tolist(), got["rec"]["end"][lo:hi].tolist())) == ev == co.spans(col(s), D, gap), name
            assert got["events"][0, c] == len(ev) and got["event_days"][0, c] == sum(e - b + 1 for b, e in ev), name
            want = np.zeros(T, np.uint8)
            for b, e in ev:
                want[b:e + 1] = 1
            assert got["mask"][:, c].tolist() == want.tolist(), name
            for k, (b, e) in enumerate(ev):  # the intensity covers the whole span, gap steps included
                assert got["rec"]["sum"][lo + k] == a[b:e + 1, c].astype(np.float64).sum(), name
                assert got["rec"]["vmax"][lo + k] == a[b:e + 1, c].max(), name


def test_windows_carry_the_state(hot):
    """T = 23, D = 3, gap = 2, in windows of 1, 2, 5 and 23 steps.  For the windows of 5 (boundaries before 5, 10, 15, 20):
    column 0 has a boundary inside a run before it qualifies (4, 5, 6), column 1 on the qualifying step (8, 9, 10), column 2
    inside a gap (run to 13, gap 14 15, run from 16: the mask rows 14 and 15 are filled from the next window), column 3 on the
    closing step (end 7, closed at 10); the windows of 1 put a boundary everywhere.  Every output, the last bit of the sums
    and the mask included, equals that of the single window."""
    T, C, D, gap = 23, 64, 3, 2
    x, a = random_case(T, C, 0.6, seed=9)
    x[:, 0] = col("....###................")
    x[:, 1] = col("........###............")
    x[:, 2] = col("...........###..###....")
    x[:, 3] = col(".....###...............")
    grp = (np.arange(T) >= 10).astype(np.int32)
    whole = device_run(hot, x, a, D, gap, grp, 2)
    w = assert_same_as_walk(whole, x, a, D, gap, grp, 2)
    assert w["events"][:, :4].tolist() == [[1, 1, 0, 1], [0, 0, 1, 0]] and whole["mask"][14:16, 2].tolist() == [1, 1]
    for mis in (False, True):
        for B in (1, 2, 5, 23):
            got = device_run(hot, x, a, D, gap, grp, 2, B=B, misaligned=mis)
            assert got["mask"].tobytes() == whole["mask"].tobytes(), (B, mis)
            for k in ACC:
                assert got[k].tobytes() == whole[k].tobytes(), (k, B, mis)
            for k in REC:
                assert got["rec"][k].tobytes() == whole["rec"][k].tobytes(), (k, B, mis)
    plain = device_run(hot, x, None, D, gap, grp, 2)  # without anomalies: four cells per lane
    assert_same_as_walk(plain, x, None, D, gap, grp, 2)
    for B in (1, 2, 5):
        got = device_run(hot, x, None, D, gap, grp, 2, B=B)
        assert got["mask"].tobytes() == plain["mask"].tobytes() == whole["mask"].tobytes(), B
        assert all(got[k].tobytes() == plain[k].tobytes() for k in ACC[:3]), B
        assert all(got["rec"][k].tobytes() == plain["rec"][k].tobytes() for k in REC[:3]), B


@pytest.mark.parametrize("D,gap", RULES)
def test_exact_sums_equal_the_direct_definition(hot, D, gap):
    """Anomalies that are multiples of 2^-10 in [-8, 8]: every float64 sum is exact, so counts, sums and maxima equal np.sum
    and np.max over the spans of the direct definition bit for bit; a tie takes the earliest step."""
    T, C = 23, 700
    x, a = random_case(T, C, 0.7, exact=True)
    a[:, :40] = np.round(a[:, :40])  # few distinct values: ties
    grp = (np.arange(T) % 3).astype(np.int32)
    got = device_run(hot, x, a, D, gap, grp, 3)
    d, r = co.direct_summary(x, a, D, gap, grp, 3), co.direct_records(x, a, D, gap)
    assert r["cell"].size > 50 and np.array_equal(got["mask"].astype(bool), co.direct_mask(x, D, gap))
    for k in ACC:
        assert np.array_equal(got[k], d[k], equal_nan=True), k
    assert np.array_equal(np.repeat(np.arange(C), np.diff(got["rec"]["off"])), r["cell"])
    for k in ("start", "end", "vmax", "tmax", "sum", "invalid"):
        assert np.array_equal(got["rec"][k], r[k], equal_nan=True), k
    ties = sum(int((a[s:e + 1, c] == v).sum() > 1) for c, s, e, v in zip(r["cell"], r["start"], r["end"], r["vmax"]))
    assert ties > 10


def test_random_float32_sums_lie_within_the_sequential_bound(hot):
    T, C, D, gap = 23, 700, 3, 1
    x, a = random_case(T, C, 0.7, seed=4)
    got = device_run(hot, x, a, D, gap)
    assert_same_as_walk(got, x, a, D, gap)
    r = co.direct_records(x, a, D, gap)
    assert r["cell"].size > 100 and r["invalid"].sum() > 0
    for k in ("start", "end", "vmax", "tmax", "invalid"):
        assert np.array_equal(got["rec"][k], r[k], equal_nan=True), k
    n = (r["end"].astype(np.int64) - r["start"] + 1).astype(np.float64)
    bound = n * 2.0 ** -53 * r["abs"]  # sequential summation of n terms against the exact sum
    err = np.abs(got["rec"]["sum"] - r["fsum"])
    print("largest error / bound", float(np.max(err / np.where(bound > 0, bound, 1.0))))
    assert (err <= bound).all()
    d = co.direct_summary(x, a, D, gap)
    for k in ("events", "event_days", "duration_max", "vmax", "invalid"):
        assert np.array_equal(got[k], d[k], equal_nan=True), k


def same(a, b):
    assert list(a.data_vars) == list(b.data_vars)
    for k in a.data_vars:
        va, vb = (v.cpu().numpy() if isinstance(v, torch.Tensor) else np.asarray(v) for v in (a[k].data, b[k].data))
        assert va.astype(vb.dtype).tobytes() == vb.tobytes(), k
        assert tuple(a[k].dims) == tuple(b[k].dims)


def test_non_finite_anomalies_and_the_public_path(hot):
    """NaN and +-inf under a present step, in a gap, at start - 1 and at end + 1: invalid_steps and the rates; host and resident
    inputs, whole and in windows, give one Dataset."""
    x = np.stack([col(".###.###....")] * 8, 1)  # D = 3, gap = 1: the event (1, 7) with its gap at 4
    base = np.array([0, 1, 2, 1, 0.5, 1, 3, 1, 0, 0, 0, 0], F)
    a = np.stack([base] * 8, 1)
    spots = [(2, NAN, 1, False, False), (4, INF, 1, False, False), (0, -INF, 0, True, False), (8, NAN, 0, False, True),
             (1, NAN, 1, True, False), (7, INF, 1, False, True), (5, -INF, 1, False, False), (11, NAN, 0, False, False)]
    for c, (t, v, *_) in enumerate(spots):
        a[t, c] = v
    first = None
    for fx, fa in ((x.astype(bool), a), (to_dev(hot, x).view(torch.bool), to_dev(hot, a))):
        for b in (None, 1, 5):
            ds = marex_amd.cell_events(fx, fa, min_duration=3, max_gap=1, records=True, return_mask=True, block_steps=b)
            if first is None:
                first = ds
            else:
                same(ds, first)
    m = to_dev(hot, x).view(torch.bool)
    res = marex_amd.cell_events(m, to_dev(hot, a), min_duration=3, max_gap=1, return_mask=True)["hobday_events"].data
    assert isinstance(res, torch.Tensor) and res.dtype == torch.bool and res.device == hot.device
    ds = first
    assert ds["start"].values.tolist() == [1] * 8 and ds["end"].values.tolist() == [7] * 8 and ds["record_offsets"].values.tolist() == list(range(9))
    assert ds["invalid_steps"].values.tolist() == [s[2] for s in spots] == ds["record_invalid_steps"].values.tolist()
    assert np.isnan(ds["rate_onset"].values).tolist() == [s[3] for s in spots]
    assert np.isnan(ds["rate_decline"].values).tolist() == [s[4] for s in spots]
    assert ds["intensity_max"].values.tolist() == [3.0] * 8 and ds["time_of_max"].values.tolist() == [6] * 8
    rec = {k: ds[v].values for k, v in dict(cell="cell", start="start", end="end", vmax="record_intensity_max", tmax="time_of_max").items()}
    on, off = co.rates(rec, a, 12)
    assert np.array_equal(on, ds["rate_onset"].values, equal_nan=True) and np.array_equal(off, ds["rate_decline"].values, equal_nan=True)
    assert ds["rate_onset"].values[7] == (3.0 - 0.5) / 5.5 and ds["rate_decline"].values[7] == (3.0 - 0.5) / 1.5
    for c in range(8):
        fin = a[1:8, c][np.isfinite(a[1:8, c])].astype(np.float64)
        assert ds["intensity_cumulative"].values[c] == fin.sum() and ds["intensity_mean"].values[c] == fin.sum() / fin.size
    assert np.array_equal(ds["hobday_events"].values, np.stack([col(".#######....")] * 8, 1).astype(bool))


_fx = {}


def gridded():
    if not _fx:
        p = os.path.join(FIX, "extremes_gridded.zarr")
        _fx["ev"] = zarr_io.read_array(os.path.join(p, "extreme_events")).astype(bool)
    return _fx["ev"]


@pytest.mark.parametrize("which", ["random 23 x 700", "reference extremes"])
def test_identities_with_occurrence_and_local_intensity(hot, which):
    if which == "random 23 x 700":
        x, a = random_case(23, 700, 0.7, seed=2)
        x = x.astype(bool)
    else:
        x = gridded()
        rng = np.random.default_rng(1)
        a = rng.normal(1, 1, x.shape).astype(F)
        a[rng.random(x.shape) < 0.02] = NAN
    xd, ad = to_dev(hot, x), to_dev(hot, a)
    one = marex_amd.cell_events(xd, min_duration=1, max_gap=0, return_mask=True)
    occ = marex_amd.event_occurrence(xd)
    assert np.array_equal(one["events"].values, occ["n_runs"].values) and one["events"].values.sum() > 0
    assert np.array_equal(one["duration_max"].values, occ["longest_run"].values)
    assert np.array_equal(one["event_days"].values, occ["occurrence"].values)
    assert torch.equal(one["hobday_events"].data, xd)
    hob = marex_amd.cell_events(xd, ad, min_duration=5, max_gap=2, return_mask=True)
    li = marex_amd.local_intensity(hob["hobday_events"], ad)
    assert hob["events"].values.sum() > 0 and hob["invalid_steps"].values.sum() > 0
    assert np.array_equal(li["days"].values.astype(np.int64) + li["invalid_steps"].values, hob["event_days"].values)
    assert np.array_equal(li["intensity_max"].values, hob["intensity_max"].values, equal_nan=True)


def test_labels_by_the_start_step(hot):
    """Three years of days; the event of cell 0 straddles New Year 2001 / 2002 and counts in 2001 only, whole."""
    tv = (np.datetime64("2000-01-01") + np.arange(1096)).astype("datetime64[ns]")
    x = np.zeros((1096, 4), np.uint8)
    s = int(np.flatnonzero(tv == np.datetime64("2001-12-28"))[0])
    x[s:s + 9, 0] = 1        # 2001-12-28 .. 2002-01-05
    x[10:16, 1] = 1          # 2000
    x[s + 10:s + 20, 1] = 1  # 2002
    x[1090:, 2] = 1          # open at the record's end
    ds = marex_amd.cell_events(DataArray(x, dims=("time", "cells"), coords={"time": ("time", tv)}), by="year", block_steps=400)
    assert ds["year"].values.tolist() == [2000, 2001, 2002] and tuple(ds["events"].dims) == ("year", "cells")
    assert ds["events"].values.tolist() == [[0, 1, 0, 0], [1, 0, 0, 0], [0, 1, 1, 0]]
    assert ds["event_days"].values.tolist() == [[0, 6, 0, 0], [9, 0, 0, 0], [0, 10, 6, 0]]
    lab = (np.arange(1096) // 100 % 3).astype(np.int64)
    got = marex_amd.cell_events(to_dev(hot, x), by=lab)
    want = co.finish(co.walk(x, None, 0, 5, 2, lab, 3))
    assert np.array_equal(got["events"].values, want["events"]) and tuple(got["events"].dims) == ("group", "cells")
    assert got["events"].values[lab[s], 0] == 1


def test_return_codes(hot):
    """Refused before any launch: nothing is written; Tb = 0 does nothing; a start label out of range adds to status[0] and
    addresses nothing (one spare group behind the accumulators as a canary)."""
    T, C, fn = 8, 700, "marex_cell_events_u8"
    x = to_dev(hot, np.ones((T, C), np.uint8))
    an = to_dev(hot, np.ones((T, C), F))
    i32 = lambda *s: torch.zeros(s, dtype=torch.int32, device=hot.device)  # noqa: E731
    f64 = lambda *s: torch.zeros(s, dtype=torch.float64, device=hot.device)  # noqa: E731
    sti, stf, st = i32(10, C), f64(2, C), torch.zeros(2, dtype=torch.int64, device=hot.device)
    acc = [i32(3, C), i32(3, C), i32(3, C), f64(3, C), i32(3, C), i32(3, C)]
    mask = torch.zeros((T, C), dtype=torch.uint8, device=hot.device)
    off = torch.arange(C + 1, dtype=torch.int64, device=hot.device)
    rec = [off, i32(C), i32(C), i32(C), i32(C), f64(C), i32(C)]
    grp = to_dev(hot, np.array([0, 0, 0, 0, 1, 1, 1, 1], np.int32))
    names = ("x", "anom", "t0", "Tb", "C", "D", "gap", "finish", "grp", "G", "sti", "stf", "events", "event_days", "duration_max", "sum",
             "vmax", "invalid", "mask", "rec_off", "rec_start", "rec_end", "rec_vmax", "rec_tmax", "rec_sum", "rec_invalid", "status")
    ok = (x, an, 0, T, C, 3, 1, 1, grp, 2, sti, stf, *acc, mask, *rec, st)
    assert len(names) == len(ok)

    def with_(**kw):
        return tuple(kw.get(k, v) for k, v in zip(names, ok))

    odd = torch.zeros(8 * C + 8, dtype=torch.uint8, device=hot.device)[1:]
    cases = [(-1, with_(x=None)), (-1, with_(sti=None)), (-1, with_(status=None)), (-1, with_(stf=None)), (-1, with_(D=0)),
             (-1, with_(gap=-1)), (-1, with_(D=-3)), (-1, with_(t0=-1)), (-1, with_(Tb=-1)), (-1, with_(C=0)), (-1, with_(G=0)),
             (-1, with_(grp=None)), (-1, with_(events=None)), (-1, with_(sum=None)), (-1, with_(rec_off=None)), (-1, with_(rec_sum=None)),
             (-1, with_(stf=odd)), (-1, with_(sti=odd)), (-1, with_(sum=odd)), (-1, with_(rec_off=odd)), (-1, with_(anom=odd)),
             (-1, with_(anom=None)),  # the anomaly members of the accumulators without anomalies
             (-4, with_(C=2**31 - 1)), (-4, with_(Tb=2**31 - 1)), (-4, with_(t0=2**31 - 1 - T)), (-4, with_(t0=2**40))]
    for code, args in cases:
        with pytest.raises(ProcessingError, match=rf"{fn} failed \(code {code}\)"):
            hot.call(fn, *args)
    hot.call(fn, *with_(Tb=0))  # does nothing
    hot.sync()
    touched = [sti, stf, st, mask] + acc + rec[1:]
    assert not any(bool(t.any()) for t in touched)
    hot.call(fn, *ok)  # every cell: one event (0, 7) of group 0
    hot.call(fn, *with_(anom=None, stf=None, sum=None, vmax=None, invalid=None, mask=None, rec_off=None, rec_start=None, rec_end=None,
                        rec_vmax=None, rec_tmax=None, rec_sum=None, rec_invalid=None, sti=i32(4, C), grp=None, G=1))  # all nullable
    hot.sync()
    assert acc[0].cpu().tolist() == [[2] * C, [0] * C, [0] * C] and acc[3][0].cpu().tolist() == [8.0] * C and not st.any()
    assert bool(mask.all()) and rec[2].cpu().tolist() == [7] * C and rec[5].cpu().tolist() == [8.0] * C
    # a start label outside 0 .. G - 1: counted in status[0]; a second event of a cell finds no room: status[1]
    sti.zero_(), stf.zero_()
    before = [t.clone() for t in acc]
    bad = to_dev(hot, np.array([2, 0, 0, 0, -1, 1, 1, 1], np.int32))
    hot.call(fn, *with_(grp=bad, mask=None))
    x2 = to_dev(hot, np.tile(col("###.###.")[:, None], (1, C)))
    sti.zero_(), stf.zero_()
    hot.call(fn, *with_(x=x2, gap=0, mask=None))
    hot.sync()
    assert st.cpu().tolist() == [C, C] and all(torch.equal(a[2], b[2]) for a, b in zip(acc, before))
    assert acc[0][0].cpu().tolist() == [3] * C and acc[0][1].cpu().tolist() == [1] * C and rec[1].cpu().tolist() == [0] * C


def test_mask_addresses_past_32_bits(hot):
    """A mask of 4099 x 2^20 bytes and a window that starts at step 4097: t0 C exceeds 2^32, and the run that qualifies in
    the window's second row fills its first.  Two rows of the field are touched; the mask takes 4.3 GB."""
    C, t0, T = 2**20, 4097, 4099
    mask = torch.empty((T, C), dtype=torch.uint8, device=hot.device)
    mask[t0 - 1:].fill_(7)
    x = torch.zeros((2, C), dtype=torch.uint8, device=hot.device)
    cells = [0, 5, 6, 2**19, C - 1]
    for c in cells:
        x[:, c] = 1
    x[1, 77] = 1  # a run of one: nothing
    r = hot.cell_events(x, t0=t0, min_duration=2, max_gap=0, mask=mask)
    assert t0 * C > 2**32 and r["events"].sum() == len(cells) and r["event_days"].sum() == 2 * len(cells)
    rows = mask[t0:].cpu().numpy()
    assert rows.sum() == 2 * len(cells) and rows[:, cells].all() and bool((mask[t0 - 1] == 7).all())
    del mask, x, r
    torch.cuda.empty_cache()
