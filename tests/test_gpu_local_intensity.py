"""GPU parity: per-cell intensity and severity categories (``marex_local_intensity_u8`` / ``marex_local_intensity_i32``
through ``HotPath.call``, ``HotPath.local_intensity`` and ``marex_amd.local_intensity``) against the NumPy oracle of
tests/local_intensity_oracle.py.  Every output is an integer, a float32 maximum or a float64 sum in one fixed order, so
everything compares with ``array_equal`` and the sums byte for byte: shapes and types, both layouts and unroll depths, the
accumulators carried across windows and revisited groups, the category rule on the exact multiples of the threshold, the
sections, the guards, 64-bit row offsets, and the public API on the output of ``preprocess_data`` for the reference's SST
fixtures."""
import os
import sys

import numpy as np
import pytest
import torch

import marex_amd
from marex_amd import calendar, zarr_io
from marex_amd.exceptions import DataValidationError, ProcessingError
from marex_amd.intensity import float_key
from marex_amd.xr_compat import DataArray

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import local_intensity_oracle as lo  # noqa: E402

pytestmark = pytest.mark.gpu
FIX = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "ref_fixtures")
F = np.float32
NAN, INF = np.nan, np.inf
U1, U4 = 8, 4  # LI_U1, LI_U4 of marex_local_intensity.hip: rows loaded together at one and at four cells per lane
H_SET = np.array([0.1, 0.7, 1.3, 1.0, 0.3, 2.2], F)  # 3 h rounds in float32 for 0.1, 0.7, 1.3, 0.3, 2.2


def case(T, C, dtype, seed=0, n_doy=3, negatives=True):
    """``x`` (IDs 0..6, half of the cells present, column 0 throughout; int32 with a few negative cells), anomalies of
    magnitudes 1e8 and 1e-3 alternating along time (so that the sums depend on the order) with NaN, +-inf and -0.0 under
    present cells and, in a third of the cells, values exactly on h, 2 h, 3 h, 4 h and one ulp to either side; thresholds
    from H_SET with columns of NaN, 0, a negative value and +inf; the row of the thresholds of every step."""
    rng = np.random.default_rng(seed + 1000 * T + C)
    x = np.where(rng.random((T, C)) < 0.5, rng.integers(1, 7, (T, C)), 0).astype(np.int32)
    x[:, 0] = 1
    if dtype == np.int32 and negatives:
        x[rng.random((T, C)) < 0.02] = -3
    doy = rng.integers(0, n_doy, T).astype(np.int32)
    thr = H_SET[rng.integers(0, H_SET.size, (n_doy, C))]
    for k, v in enumerate((NAN, 0.0, -0.5, INF, -0.0)):
        thr[:, (5 + k) % C::11] = v
    an = (rng.uniform(1, 2, (T, C)) * np.where(np.arange(T) % 2 == 0, 1e8, 1e-3)[:, None] * rng.choice([-1, 1], (T, C))).astype(F)
    h = thr[doy]
    with np.errstate(invalid="ignore", over="ignore"):
        edge = (F(1) + rng.integers(0, 4, (T, C)).astype(F)) * h  # h, 2 h, 3 h, 4 h: one float32 multiply each
        step = rng.integers(-1, 2, (T, C))
        edge = np.where(step < 0, np.nextafter(edge, F(-INF)), np.where(step > 0, np.nextafter(edge, F(INF)), edge)).astype(F)
    on_edge = (rng.random((T, C)) < 0.35) & np.isfinite(edge)
    an = np.where(on_edge, edge, an).astype(F)
    for v in (NAN, INF, -INF, -0.0, 0.0):
        an[rng.random((T, C)) < 0.03] = v
    return x.astype(dtype), an, thr, doy


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


def tab(hot, v, dt=np.int32):
    return None if v is None else torch.from_numpy(np.ascontiguousarray(v, dtype=dt)).to(hot.device)


def kernel(hot, x, an, t0=0, match=0, grp=None, G=1, thr=None, doy=None, sgrp=None, G2=0, cls=None, R=0, bufs=None):
    """One library call on buffers of the test's own, zeroed once, one spare group behind every accumulator as a canary."""
    Tb, C = x.shape
    if bufs is None:
        z = lambda shape, dt: torch.zeros(shape, dtype=dt, device=hot.device)  # noqa: E731
        bufs = {"days": z((G + 1, C), torch.int32), "invalid": z((G + 1, C), torch.int32), "sum": z((G + 1, C), torch.float64),
                "vmax": z((G + 1, C), torch.int32), "tmax": z((G + 1, C), torch.int32),
                "cat_days": z((G + 1, 6, C), torch.int32) if thr is not None else None,
                "sec_cnt": z((G2 + 1, R, 6), torch.int64) if sgrp is not None else None, "status": z((2,), torch.int64),
                "grp": tab(hot, grp), "thr": tab(hot, thr, F), "doy": tab(hot, doy), "sgrp": tab(hot, sgrp), "cls": tab(hot, cls)}
    fn = "marex_local_intensity_i32" if x.dtype == torch.int32 else "marex_local_intensity_u8"
    n_doy = 0 if bufs["thr"] is None else int(bufs["thr"].shape[0])
    hot.call(fn, x, an, t0, Tb, C, match, bufs["grp"], G, bufs["thr"], bufs["doy"], n_doy, bufs["sgrp"], G2, bufs["cls"], R,
             bufs["days"], bufs["invalid"], bufs["sum"], bufs["vmax"], bufs["tmax"], bufs["cat_days"], bufs["sec_cnt"], bufs["status"])
    return bufs


VIEWS = {"days": np.uint32, "invalid": np.uint32, "sum": np.float64, "vmax": np.uint32, "tmax": np.int32, "cat_days": np.uint32,
         "sec_cnt": np.uint64}


def read(bufs):
    out = {}
    for k, dt in VIEWS.items():
        if bufs[k] is None:
            out[k] = None
            continue
        a = bufs[k].cpu().numpy()
        assert not a[-1].view(np.uint8).any(), k  # the canary group
        out[k] = a[:-1].view(dt)
    out["status"] = bufs["status"].cpu().numpy().tolist()
    return out


def equal_oracle(r, s, what):
    """The kernel's accumulators against an oracle state: the key and the raw step of the maximum, the sum byte for byte."""
    for k, o in (("days", "days"), ("invalid", "invalid"), ("vmax", "key"), ("tmax", "tmax"), ("cat_days", "cat_days"),
                 ("sec_cnt", "sec_cnt")):
        if s[o] is None:
            assert r[k] is None, (k, what)
        else:
            assert r[k].dtype == s[o].dtype and np.array_equal(r[k], s[o]), (k, what)
    assert r["sum"].tobytes() == s["sum"].tobytes(), ("sum", what)
    assert r["status"] == s["status"], ("status", r["status"], s["status"], what)


def check(hot, x_h, an_h, misaligned=False, **kw):
    """The kernel on the fields against the oracle, twice: equal bytes, inputs unmodified."""
    outs = []
    for _ in range(2):
        x, an = to_dev(hot, x_h, misaligned), to_dev(hot, an_h)
        bufs = kernel(hot, x, an, 0, **kw)
        r = read(bufs)
        assert x.cpu().numpy().tobytes() == x_h.tobytes() and an.cpu().numpy().tobytes() == an_h.tobytes()
        if kw.get("thr") is not None:
            assert bufs["thr"].cpu().numpy().tobytes() == np.ascontiguousarray(kw["thr"], F).tobytes()
        outs.append(b"".join(v.tobytes() for k, v in r.items() if v is not None and k != "status"))
    assert outs[0] == outs[1]
    equal_oracle(r, lo.accumulate(x_h, an_h, 0, kw.get("grp"), kw.get("G", 1), kw.get("thr"), kw.get("doy"), kw.get("sgrp"),
                                  kw.get("G2", 0), kw.get("cls"), kw.get("R", 0), kw.get("match", 0)),
                 (x_h.shape, x_h.dtype, misaligned, sorted(kw)))
    return r


def mesh_classes(C, R, seed=3):
    """A shuffled class table with cells at -1 and at R (both counted nowhere)."""
    rng = np.random.default_rng(seed)
    cls = rng.integers(0, R, C).astype(np.int32)
    cls[rng.random(C) < 0.1] = -1
    cls[C - 1] = R
    return cls


KINDS = [(np.uint8, False), (np.uint8, True), (np.int32, False)]
KIND_IDS = ["u8", "u8-misaligned", "i32"]


@pytest.mark.parametrize("dtype,misaligned", KINDS, ids=KIND_IDS)
@pytest.mark.parametrize("C", [1, 63, 64, 65, 257, 1024, 1028])
def test_shapes_and_types_equal_the_oracle(hot, C, dtype, misaligned):
    """Fewer cells than a wave, partial waves and workgroups, several workgroups; uint8 at four cells per lane (C = 64, 1024,
    1028, aligned, no thresholds) and at one (the other sizes, the misaligned view, every call with thresholds)."""
    T = 11
    x, an, thr, doy = case(T, C, dtype)
    grp = np.arange(T, dtype=np.int32) % 4        # cyclic, G = 5: group 4 has no step
    cls = mesh_classes(C, 9)
    r = check(hot, x, an, misaligned, grp=grp, G=5)
    assert not r["days"][4].any() and r["days"].sum() > 0 and (r["invalid"].sum() > 0 or C < 63)
    r = check(hot, x, an, misaligned, grp=grp, G=5, thr=thr, doy=doy)
    assert r["cat_days"].sum() == r["days"].sum() and not r["cat_days"][4].any()
    r = check(hot, x, an, misaligned, grp=grp, G=5, thr=thr, doy=doy, sgrp=np.arange(T, dtype=np.int32) // 2, G2=6, cls=cls, R=9)
    assert r["sec_cnt"].sum() == r["cat_days"][:, :, (cls >= 0) & (cls < 9)].sum()
    if C >= 257:
        assert all(r["cat_days"][:, k].any() for k in range(6))
    if dtype == np.int32:
        assert r["status"][0] == (x < 0).sum() > 0 or C < 63


@pytest.mark.parametrize("dtype,misaligned", KINDS, ids=KIND_IDS)
def test_row_counts_around_both_unroll_depths(hot, dtype, misaligned):
    """Tb = 1, U - 1, U, U + 1 and 2 U + 3 for U = 4 (four cells per lane) and U = 8 (one), with and without thresholds."""
    C = 1028
    for Tb in sorted({1, U1 - 1, U1, U1 + 1, 2 * U1 + 3, U4 - 1, U4, U4 + 1, 2 * U4 + 3}):
        x, an, thr, doy = case(Tb, C, dtype, seed=Tb)
        grp = (np.arange(Tb, dtype=np.int32) // 3) % 2
        check(hot, x, an, misaligned, grp=grp, G=2)
        check(hot, x, an, misaligned, grp=grp, G=2, thr=thr, doy=doy, sgrp=np.zeros(Tb, np.int32), G2=1,
              cls=np.arange(C, dtype=np.int32) // 200, R=6)


def run_windows(hot, x_h, an_h, cuts, misaligned=False, **kw):
    bufs = None
    for a, b in zip(cuts[:-1], cuts[1:]):
        bufs = kernel(hot, to_dev(hot, x_h[a:b], misaligned), to_dev(hot, an_h[a:b]), a, bufs=bufs, **kw)
    return read(bufs)


def same_bytes(a, b, what):
    for k in list(VIEWS) + ["status"]:
        if a[k] is None:
            assert b[k] is None
        elif k == "status":
            assert a[k] == b[k], (k, what)
        else:
            assert a[k].tobytes() == b[k].tobytes(), (k, what)


@pytest.mark.parametrize("dtype,misaligned", KINDS, ids=KIND_IDS)
def test_windows_continue_the_accumulators(hot, dtype, misaligned):
    """The windows [0, 5) [5, 6) [6, T), every split into two and the split into single rows give the bytes of one call --
    the sums included, whose terms of 1e8 and 1e-3 make every other association visible; group 1 spans the cuts at 5 and
    6, the section label changes inside and at the cuts."""
    T, C = 13, 1028
    x, an, thr, doy = case(T, C, dtype, seed=7)
    grp = np.array([0, 0, 0, 1, 1, 1, 1, 1, 2, 2, 0, 0, 1], np.int32)
    sgrp = np.array([0, 0, 1, 1, 1, 2, 2, 2, 2, 0, 0, 3, 3], np.int32)
    cls = np.arange(C, dtype=np.int32) // 100
    for kw in (dict(grp=grp, G=3), dict(grp=grp, G=3, thr=thr, doy=doy, sgrp=sgrp, G2=4, cls=cls, R=11)):
        whole = check(hot, x, an, misaligned, **kw)
        for cuts in [[0, 5, 6, T], list(range(T + 1))] + [[0, s, T] for s in range(1, T)]:
            same_bytes(run_windows(hot, x, an, cuts, misaligned, **kw), whole, (cuts, sorted(kw)))


def test_the_sum_is_sequential_and_a_reassociated_sum_differs(hot):
    """What the bitwise comparison can see: on these fields the sum of the even rows plus the sum of the odd rows differs
    from the sequential sum in most cells, and the kernel gives the sequential one -- whole, in windows and per group."""
    T, C = 40, 1028
    rng = np.random.default_rng(5)
    an = (rng.uniform(1, 2, (T, C)) * np.where(np.arange(T) % 2 == 0, 1e8, 1e-3)[:, None]).astype(F)
    x = np.ones((T, C), np.uint8)
    seq = np.zeros(C)
    for t in range(T):
        seq += an[t].astype(np.float64)
    pair = an[::2].astype(np.float64).sum(axis=0) + an[1::2].astype(np.float64).sum(axis=0)
    assert (seq != pair).mean() > 0.5
    r = check(hot, x, an)
    assert r["sum"][0].tobytes() == seq.tobytes()
    same_bytes(run_windows(hot, x, an, [0, 5, 6, 23, T]), r, "windows")
    season = (np.arange(T, dtype=np.int32) // 3) % 4  # revisited groups: the stored partial sum is loaded, not added to
    g = check(hot, x, an, grp=season, G=4)
    for k in range(4):
        s = np.zeros(C)
        for t in np.flatnonzero(season == k):
            s += an[t].astype(np.float64)
        assert g["sum"][k].tobytes() == s.tobytes()


LABELS = {"years": [0] * 8 + [1] * 8 + [2] * 8, "seasons over three years": [0, 0, 1, 1, 2, 2, 3, 3] * 3,
          "every row": [0, 1] * 12, "non-monotone": [3, 3, 0, 0, 0, 2, 2, 3, 0, 0, 1, 3] * 2, "none": None}


@pytest.mark.parametrize("dtype", [np.uint8, np.int32], ids=["u8", "i32"])
@pytest.mark.parametrize("name", list(LABELS))
def test_step_labels(hot, name, dtype):
    """Contiguous, revisited, alternating and non-monotone labels, G = 1 with a null table; the same through the engine,
    whose fresh buffers are poisoned, so the zeroing shows."""
    T, C = 24, 1028
    x, an, thr, doy = case(T, C, dtype, negatives=False)
    grp = None if LABELS[name] is None else np.asarray(LABELS[name], np.int32)
    G = 1 if grp is None else 4
    cls = np.repeat(np.arange(C // 4, dtype=np.int32), 4)
    sgrp = np.arange(T, dtype=np.int32) // 5
    check(hot, x, an, grp=grp, G=G)
    check(hot, x, an, grp=grp, G=G, thr=thr, doy=doy, sgrp=sgrp, G2=5, cls=cls, R=C // 4)
    from marex_amd.engine import HotPath

    assert HotPath.POISON
    for cats in (False, True):
        kw = dict(thr=to_dev(hot, thr), doy=doy, sgrp=sgrp, G2=5, cls=cls, R=C // 4) if cats else {}
        e = hot.local_intensity(to_dev(hot, x), to_dev(hot, an), grp=grp, G=G, **kw)
        a = hot.local_intensity(to_dev(hot, x[:7]), to_dev(hot, an[:7]), grp=grp, G=G, finish=False, **kw)["acc"]
        w = hot.local_intensity(to_dev(hot, x[7:]), to_dev(hot, an[7:]), t0=7, grp=grp, G=G, acc=a, **kw)
        s = lo.finish(lo.accumulate(x, an, 0, grp, G, thr if cats else None, doy, sgrp if cats else None, 5, cls if cats else None, C // 4))
        for r in (e, w):
            for k in ("days", "invalid", "sum", "vmax", "tmax") + (("cat_days", "sec_cnt") if cats else ()):
                assert r[k].dtype == s[k].dtype and r[k].tobytes() == s[k].tobytes(), (k, cats)
            assert (r["cat_days"] is None and r["sec_cnt"] is None) or cats


def test_a_maximum_attained_twice_keeps_the_earliest_step(hot):
    """Within a call, across a window cut and across a revisit of the group; -0.0 lies below +0.0; a larger value later
    replaces the step, an equal one does not."""
    T, C = 12, 65
    x = np.ones((T, C), np.uint8)
    an = np.full((T, C), -1.0, F)
    an[2, 0] = an[9, 0] = 5.0           # twice, the cut at 5 between them
    an[3, 1] = an[4, 1] = 5.0           # twice in one window
    an[1, 2], an[8, 2] = 5.0, 5.5       # a larger one later
    an[:, 3] = -0.0
    an[7, 3] = 0.0                      # +0 above -0
    an[:, 4] = NAN                      # never finite: no maximum
    an[0, 5] = an[11, 5] = INF          # infinite: invalid, not a maximum
    grp = np.array([0, 0, 0, 1, 1, 1, 0, 0, 0, 0, 1, 1], np.int32)  # group 0 is revisited at step 6
    for kw in ({}, dict(grp=grp, G=2)):
        r = check(hot, x, an, **kw)
        same_bytes(run_windows(hot, x, an, [0, 5, 6, T], **kw), r, kw)
    assert r["tmax"][0, :6].tolist() == [2, 0, 8, 7, 0, 1] and r["tmax"][1, :6].tolist() == [3, 3, 3, 3, 0, 3]
    assert r["vmax"][0, :4].tolist() == float_key(np.array([5.0, -1.0, 5.5, 0.0], F)).tolist() and r["vmax"][0, 4] == 0
    assert r["invalid"][:, 4].tolist() == [7, 5] and r["invalid"][:, 5].tolist() == [1, 1]


def test_category_rule_on_the_exact_multiples(hot):
    """One cell per (threshold of H_SET, edge h .. 4 h, one ulp below / on / one ulp above): the class is the oracle's and
    the one written down here; thresholds of NaN, 0, -0, a negative value and +-inf are undefined."""
    hs, cells, want = [], [], []
    for h in H_SET:
        for k in (1, 2, 3, 4):
            e = F(k) * h
            for d, v in ((-1, np.nextafter(e, F(-INF))), (0, e), (1, np.nextafter(e, F(INF)))):
                hs.append(h), cells.append(v), want.append(k - 1 if d < 0 else k)
    for h in (NAN, 0.0, -0.0, -1.0, INF, -INF):
        hs.append(F(h)), cells.append(F(1.0)), want.append(5)
    C = len(hs)
    assert float(F(3) * F(0.1)) != 3 * float(F(0.1)) and C > 64
    thr, an = np.array(hs, F)[None], np.array(cells, F)[None]
    for dtype in (np.uint8, np.int32):
        r = check(hot, np.ones((1, C), dtype), an, thr=thr, doy=np.zeros(1, np.int32), sgrp=np.zeros(1, np.int32), G2=1,
                  cls=np.zeros(C, np.int32), R=1)
        assert np.argmax(r["cat_days"][0], axis=0).tolist() == want and (r["cat_days"][0].sum(axis=0) == 1).all()
        assert r["sec_cnt"][0, 0].tolist() == np.bincount(want, minlength=6).tolist()


@pytest.mark.parametrize("dtype,misaligned", KINDS, ids=KIND_IDS)
def test_sections(hot, dtype, misaligned):
    """One class per wave, 64 classes in one wave, grid rows that end inside waves, and classes -1 and R."""
    T = 9
    sgrp = np.array([0, 0, 1, 1, 1, 3, 0, 0, 3], np.int32)
    for C, cls, R in ((1028, np.arange(1028, dtype=np.int32) // 64, 17), (1028, np.arange(1028, dtype=np.int32) % 64, 64),
                      (11 * 100, np.repeat(np.arange(11, dtype=np.int32), 100), 11), (693, mesh_classes(693, 70), 70)):
        x, an, thr, doy = case(T, C, dtype)
        r = check(hot, x, an, misaligned, thr=thr, doy=doy, sgrp=sgrp, G2=4, cls=cls, R=R)
        assert not r["sec_cnt"][2].any() and r["sec_cnt"].sum() == r["cat_days"][:, :, (cls >= 0) & (cls < R)].sum() > 0


@pytest.mark.parametrize("dtype,misaligned", KINDS, ids=KIND_IDS)
def test_selected_id(hot, dtype, misaligned):
    T, C = 9, 1028
    x, an, thr, doy = case(T, C, dtype)
    for match in (4, 9, 1):  # a selected ID, one absent from the field, ID 1
        r = check(hot, x, an, misaligned, match=match)
        assert np.array_equal(r["days"][0] + r["invalid"][0], (x == match).sum(0))
        check(hot, x, an, misaligned, match=match, thr=thr, doy=doy)
    clean = np.where(x.astype(np.int64) < 0, 0, x).astype(dtype)
    e = hot.local_intensity(to_dev(hot, clean, misaligned), to_dev(hot, an), match=4)
    assert np.array_equal(e["days"], lo.accumulate(clean, an, match=4)["days"])


def test_guards(hot):
    T, C = 6, 693
    x, an, thr, doy = case(T, C, np.int32)
    neg = int((x < 0).sum())
    assert neg > 0
    with pytest.raises(DataValidationError, match="Object IDs must be non-negative"):
        marex_amd.local_intensity(x, an)
    with pytest.raises(DataValidationError, match="Object IDs must be non-negative"):
        marex_amd.local_intensity(to_dev(hot, x), to_dev(hot, an), block_steps=4)
    with pytest.raises(DataValidationError, match=f"{neg} negative cells"):
        hot.local_intensity(to_dev(hot, x), to_dev(hot, an))
    # labels outside their ranges handed straight to the library: counted, nothing corrupted (read() checks the spare group)
    clean = np.maximum(x, 0)
    p = clean > 0
    grp = np.array([0, 1, 2, 7, -1, 1], np.int32)
    bad_doy = np.array([0, 3, 1, 1, 2, -1], np.int32)
    sgrp = np.array([0, 5, 0, 0, -4, 0], np.int32)
    cls = np.repeat(np.arange(7, dtype=np.int32), 99)
    r = check(hot, clean, an, grp=grp, G=3)
    assert r["status"] == [0, int(p[3].sum() + p[4].sum())]
    r = check(hot, clean, an, grp=grp, G=3, thr=thr, doy=bad_doy, sgrp=sgrp, G2=1, cls=cls, R=7)
    assert r["status"][1] == int(p[1].sum() + p[3].sum() + p[4].sum() + p[5].sum())  # step 1 is lost to doy before sgrp is looked at
    with pytest.raises(ProcessingError, match=f"local_intensity: {int(p[3].sum() + p[4].sum())} present cells lie under"):
        hot.local_intensity(to_dev(hot, clean), to_dev(hot, an), grp=grp, G=3)
    xd, ad, td = to_dev(hot, clean), to_dev(hot, an), to_dev(hot, thr)
    for bad in (lambda: hot.local_intensity(xd.to(torch.int64), ad), lambda: hot.local_intensity(xd.t(), ad),
                lambda: hot.local_intensity(xd, ad.to(torch.float64)), lambda: hot.local_intensity(xd, ad[:-1]),
                lambda: hot.local_intensity(xd, ad, t0=-1), lambda: hot.local_intensity(xd, ad, G=2),
                lambda: hot.local_intensity(xd, ad, match=-1), lambda: hot.local_intensity(xd, ad, grp=grp[:3], G=8),
                lambda: hot.local_intensity(xd, ad, thr=td), lambda: hot.local_intensity(xd, ad, doy=doy),
                lambda: hot.local_intensity(xd, ad, thr=td[:, :-1], doy=doy), lambda: hot.local_intensity(xd, ad, thr=td.double(), doy=doy),
                lambda: hot.local_intensity(xd, ad, thr=td, doy=doy[:3]),
                lambda: hot.local_intensity(xd, ad, sgrp=sgrp, G2=6, cls=cls, R=7),  # sections without thresholds
                lambda: hot.local_intensity(xd, ad, thr=td, doy=doy, sgrp=sgrp, G2=6),
                lambda: hot.local_intensity(xd, ad, thr=td, doy=doy, cls=cls[:-1], sgrp=sgrp, G2=6, R=7),
                lambda: hot.local_intensity(xd, ad, G=1, acc=hot.local_intensity(xd, ad, grp=grp, G=8, finish=False)["acc"])):
        with pytest.raises(ProcessingError):
            bad()


@pytest.mark.parametrize("fn,dtype", [("marex_local_intensity_u8", np.uint8), ("marex_local_intensity_i32", np.int32)])
def test_return_codes(hot, fn, dtype):
    T, C = 6, 700
    x_h, an_h, thr_h, _ = case(T, C, dtype, negatives=False)
    x, an, thr = to_dev(hot, x_h), to_dev(hot, an_h), to_dev(hot, thr_h)
    lab, cls = tab(hot, np.zeros(T, np.int32)), tab(hot, np.zeros(C, np.int32))
    z = lambda shape, dt: torch.zeros(shape, dtype=dt, device=hot.device)  # noqa: E731
    days, inv, vm, tm = (z((1, C), torch.int32) for _ in range(4))
    sm, cat, sec, st = z((1, C), torch.float64), z((1, 6, C), torch.int32), z((1, 1, 6), torch.int64), z((2,), torch.int64)
    names = ("x", "anom", "t0", "Tb", "C", "match", "grp", "G", "thr", "doy", "n_doy", "sgrp", "G2", "cls", "R", "days", "invalid",
             "sum", "vmax", "tmax", "cat_days", "sec_cnt", "status")
    ok = (x, an, 0, T, C, 0, lab, 1, thr, lab, 3, lab, 1, cls, 1, days, inv, sm, vm, tm, cat, sec, st)

    def with_(**kw):
        return tuple(kw.get(k, v) for k, v in zip(names, ok))

    no_sec = dict(sgrp=None, cls=None, sec_cnt=None, G2=0, R=0)
    cases = [(-4, with_(C=2**31 - 1)), (-4, with_(C=2**40)), (-4, with_(Tb=2**31 - 1)), (-4, with_(t0=2**31 - 1 - T)),
             (-4, with_(t0=2**40)), (-1, with_(Tb=0)), (-1, with_(C=0)), (-1, with_(t0=-1)), (-1, with_(match=-1)), (-1, with_(G=0)),
             (-1, with_(grp=None, G=2)), (-1, with_(G2=0)), (-1, with_(R=0)), (-1, with_(sgrp=None)), (-1, with_(cls=None)),
             (-1, with_(sec_cnt=None)), (-1, with_(thr=None, **no_sec)), (-1, with_(doy=None, **no_sec)),
             (-1, with_(cat_days=None, **no_sec)), (-1, with_(n_doy=0, **no_sec)), (-1, with_(thr=None, doy=None, cat_days=None)),
             (-1, with_(x=None)), (-1, with_(anom=None)), (-1, with_(days=None)), (-1, with_(invalid=None)), (-1, with_(sum=None)),
             (-1, with_(vmax=None)), (-1, with_(tmax=None)), (-1, with_(status=None))]
    for code, args in cases:  # refused by the library before any launch
        with pytest.raises(ProcessingError, match=rf"{fn} failed \(code {code}\)"):
            hot.call(fn, *args)
    hot.sync()
    assert not any(bool(b.any()) for b in (days, inv, sm, vm, tm, cat, sec, st))
    for args in (ok, with_(grp=None), with_(**no_sec), with_(thr=None, doy=None, cat_days=None, n_doy=0, **no_sec)):  # all nullable
        hot.call(fn, *args)
    hot.sync()
    n = int(((x > 0) & torch.isfinite(an)).sum().item())
    assert int(days.sum().item()) == 4 * n and int(cat.sum().item()) == 3 * n and int(sec.sum().item()) == 2 * n and not st.any()


def test_row_offsets_past_32_bits(hot):
    """Fields of 8 x (2^28 + 4) cells, 2^31 + 32 in all, made on the device: a constant anomaly, a handful of cells set in
    the first and the last rows; the rows 2 .. 7 of the uint8 field start past 2^29 bytes, the rows 4 .. 7 of the anomalies
    past 2^32.  Four cells per lane without thresholds, one with; the oracle runs on the touched columns only."""
    T, C = 8, 2**28 + 4
    x = torch.zeros((T, C), dtype=torch.uint8, device=hot.device)
    an = torch.full((T, C), 0.25, dtype=torch.float32, device=hot.device)
    cols = [0, 5, 6, 2**27, 2**28 - 1, C - 4, C - 1]
    cells = [(0, 0), (0, 5), (0, C - 1), (1, 6), (1, 2**27), (6, 0), (6, 2**28 - 1), (7, 0), (7, 5), (7, 6), (7, C - 4), (7, C - 1)]
    x_s, an_s = np.zeros((T, len(cols)), np.uint8), np.full((T, len(cols)), 0.25, F)
    for n, (t, c) in enumerate(cells):
        v = 1.0 + n / 8 if n != 3 else NAN
        x[t, c] = 1
        an[t, c] = v
        x_s[t, cols.index(c)], an_s[t, cols.index(c)] = 1, v
    grp = np.array([0, 0, 0, 0, 1, 1, 1, 1], np.int32)
    thr = torch.full((1, C), 0.5, dtype=torch.float32, device=hot.device)
    for cats in (False, True):
        kw = dict(thr=thr, doy=np.zeros(T, np.int32)) if cats else {}
        acc = hot.local_intensity(x, an, grp=grp, G=2, finish=False, **kw)["acc"]
        s = lo.accumulate(x_s, an_s, 0, grp, 2, np.full((1, len(cols)), 0.5, F) if cats else None, np.zeros(T, np.int32))
        assert acc["status"].cpu().tolist() == [0, 0]
        for k, o in (("days", "days"), ("invalid", "invalid"), ("sum", "sum"), ("vmax", "key"), ("tmax", "tmax")):
            got = acc[k][:, cols].cpu().numpy()
            assert got.view(s[o].dtype).tobytes() == s[o].tobytes(), (k, cats)
        assert int(acc["days"].sum(dtype=torch.int64).item()) == len(cells) - 1 and int(acc["invalid"].sum(dtype=torch.int64).item()) == 1
        assert float(acc["sum"].sum().item()) == float(s["sum"].sum()) and int((acc["vmax"] != 0).sum().item()) == int((s["key"] != 0).sum())
        if cats:
            assert np.array_equal(acc["cat_days"][:, :, cols].cpu().numpy().view(np.uint32), s["cat_days"])
            assert int(acc["cat_days"].sum(dtype=torch.int64).item()) == len(cells) - 1
        del acc
        torch.cuda.empty_cache()
    assert int(x.sum(dtype=torch.int64).item()) == len(cells)
    del x, an, thr
    torch.cuda.empty_cache()


# ------------------------------------------------------------------ the public API on the output of preprocess_data
def same(a, b):
    assert list(a.data_vars) == list(b.data_vars)
    for k in a.data_vars:
        assert np.asarray(a[k].values).tobytes() == np.asarray(b[k].values).tobytes(), k
        assert tuple(a[k].dims) == tuple(b[k].dims)


def resident(hot, da):
    t = torch.from_numpy(np.ascontiguousarray(da.values)).to(hot.device)
    return DataArray(t, dims=tuple(da.dims), coords={k: (tuple(v.dims), np.asarray(v.values)) for k, v in da.coords.items()})


def end_to_end(hot, ds, space, **kw):
    """``local_intensity(by="year", zonal=True)`` on the host arrays and on resident copies of a ``preprocess_data``
    result, whole and in windows: one Dataset, equal to the oracle on the host copies.  Returns the oracle's variables."""
    ev, an, thr = ds["extreme_events"], ds["dat_anomaly"], ds["thresholds"]
    first = None
    for f, a, h in ((ev, an, thr), (resident(hot, ev), resident(hot, an), resident(hot, thr))):
        for b in (None, 4000):
            out = marex_amd.local_intensity(f, a, h, by="year", zonal=True, block_steps=b, **kw)
            if first is None:
                first = out
            else:
                same(first, out)
    tm = np.asarray(an.coords["time"].values)
    T = tm.size
    C = int(np.prod(space))
    year, doy = calendar._to_year_doy(tm)
    yv, ylab = np.unique(year, return_inverse=True)
    mi = tm.astype("datetime64[M]").astype(np.int64)
    hd = tuple(thr.dims)
    h = np.asarray(thr.values)
    h = (np.moveaxis(h, -1, 0) if hd[-1] == "dayofyear" else h).reshape(366, C)
    if len(space) == 2:
        cls, R, ccells = np.repeat(np.arange(space[0], dtype=np.int32), space[1]), space[0], np.full(space[0], space[1])
    else:
        import occurrence_oracle as oo

        cls = oo.lat_bin(kw["lat"], kw["lat_bins"])
        R = len(kw["lat_bins"]) - 1
        ccells = np.bincount(cls[cls >= 0], minlength=R)
    exp = lo.local_intensity(np.asarray(ev.values).reshape(T, C), np.asarray(an.values).reshape(T, C), tm, ylab.astype(np.int32), yv.size,
                             h, doy.astype(np.int32) - 1, (mi - mi.min()).astype(np.int32), int(mi.max() - mi.min()) + 1, cls, R, ccells)
    assert sorted(first.data_vars) == sorted(exp)
    for k, want in exp.items():
        got = np.asarray(first[k].values)
        got = got.reshape(want.shape) if k not in ("steps_by", "category_cells", "category_share", "class_cells") else got
        assert got.dtype == want.dtype and got.shape == want.shape, (k, got.dtype, want.dtype, got.shape, want.shape)
        assert got.tobytes() == np.asarray(want).tobytes(), k
    assert np.asarray(first["days"].coords["year"].values).tolist() == yv.tolist()
    assert exp["days"].sum() == np.asarray(ev.values).sum() - exp["invalid_steps"].sum() > 0
    print("category days of the oracle (below .. undefined):", exp["category_days"].sum(axis=(0, 2)).tolist(),
          "invalid steps:", int(exp["invalid_steps"].sum()))
    return exp


_sst = {}


def gridded_sst():
    if not _sst:
        p = os.path.join(FIX, "sst_gridded.zarr")
        x = zarr_io.read_array(os.path.join(p, "to")).copy()
        tm = zarr_io.decode_cf_time(zarr_io.read_array(os.path.join(p, "time")), zarr_io.array_attrs(os.path.join(p, "time")))
        x[:, 1, 1] = np.nan
        lat, lon = zarr_io.read_array(os.path.join(p, "lat")), zarr_io.read_array(os.path.join(p, "lon"))
        _sst["da"] = DataArray(x, dims=("time", "lat", "lon"), coords={"time": tm, "lat": lat, "lon": lon}, name="to")
    return _sst["da"]


@pytest.mark.parametrize("method_percentile", ["approximate", "exact"])
def test_end_to_end_on_the_gridded_sst_fixture(hot, method_percentile):
    """``preprocess_data`` (shifting baseline, Hobday thresholds by the approximate and by the exact percentile) on the
    reference's gridded SST fixture, then annual maps and monthly zonal category counts from its ``extreme_events``,
    ``dat_anomaly`` and ``thresholds``.  Under ``extreme_events`` the class "below" must be empty: the mask is
    ``anomaly >= threshold`` of the same day of the year.  It is: the oracle gives, as days below / moderate / strong /
    severe / extreme / undefined, 0 / 510 602 / 4 704 / 4 / 0 / 0 with the approximate percentile and 0 / 572 168 / 7 672 /
    93 / 0 / 0 with the exact one, no invalid step."""
    ds = marex_amd.preprocess_data(gridded_sst(), method_anomaly="shifting_baseline", method_extreme="hobday_extreme",
                                   threshold_percentile=95, window_year_baseline=5, smooth_days_baseline=11, window_days_hobday=3,
                                   method_percentile=method_percentile, dimensions={"time": "time", "x": "lon", "y": "lat"})
    exp = end_to_end(hot, ds, (20, 40))
    assert exp["category_days"][:, 0].sum() == 0 and exp["category_days"][:, 5].sum() == 0
    assert exp["category_days"][:, 1].sum() > exp["category_days"][:, 2].sum() > 0


def test_end_to_end_on_the_unstructured_sst_fixture(hot):
    """The same on the reference's unstructured SST fixture, with latitude bins of 30 degrees.  The oracle gives 0 days
    below, 284 595 moderate, 1 250 strong and none severe, extreme or undefined."""
    p = os.path.join(FIX, "sst_unstructured.zarr")
    x = zarr_io.read_array(os.path.join(p, "to")).copy()
    tm = zarr_io.decode_cf_time(np.round(zarr_io.read_array(os.path.join(p, "time")) * 60.0), {"units": "seconds since 1950-01-01"})
    x[:, 2] = np.nan
    n = x.shape[1]
    lat = np.linspace(-90, 90, n)
    da = DataArray(x, dims=("time", "ncells"), coords={"time": tm, "lat": ("ncells", lat), "lon": ("ncells", np.linspace(-180, 180, n))},
                   name="to")
    ds = marex_amd.preprocess_data(da, method_anomaly="shifting_baseline", method_extreme="hobday_extreme", threshold_percentile=95,
                                   window_year_baseline=5, smooth_days_baseline=5, window_days_hobday=3,
                                   dimensions={"time": "time", "x": "ncells"}, coordinates={"time": "time", "x": "lon", "y": "lat"})
    exp = end_to_end(hot, ds, (n,), lat=lat, lat_bins=np.arange(-90.0, 91.0, 30.0))
    assert exp["category_days"][:, 0].sum() == 0 and exp["category_days"][:, 5].sum() == 0
    assert exp["category_cells"].sum() == exp["category_days"][:, :, lat > -90].sum()
