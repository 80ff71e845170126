"""One-off measurement (not a pytest file): per-cell trends (``marex_trend_stats_f64``, ``marex_trend_select_f64``) of
``TRD_NY`` x ``TRD_NX`` cells (default 720 x 1440) with 30 % land, for G = 40 and G = 100 maps (``TRD_STEPS``), on two
kinds of maps: (days) Poisson counts as ``local_intensity(by="year")["days"]`` gives them, no sample missing, most slopes
coincide; (mean) float maps as its ``intensity_mean``, 15 % of the years missing.

(ks)  ``marex_trend_stats_f64`` alone;            (kq)  ``marex_trend_select_f64`` alone, four ranks per cell;
(r)   ``marex_amd.cell_trends`` on resident float64 maps;      (h)   the same from host maps (float32, uploaded);
(n)   baseline: the vectorised NumPy oracle of tests/trends_oracle.py (``stats`` and ``select`` at the same four ranks) on
      the first ``TRD_HOST_CELLS`` ocean cells (default 5000), SCALED to the field by the number of cells;
(s)   baseline: ``scipy.stats.theilslopes`` cell by cell on ``TRD_SCIPY_CELLS`` ocean cells (default 300), SCALED likewise
      (skipped without scipy).

Kernel times are the engine's launch timer (HIP events around the launch inside the library), wall times are host clocks
that end in a synchronise; medians of REPS after one warm-up.  The derived count of divisions is 64 steps x G (G - 1) / 2
pairs per cell of a wave that holds an ocean cell."""
import json
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import numpy as np
import torch

import marex_amd
import marex_amd.trends as mt
import trends_oracle as to
from marex_amd.detect import get_engine

REPS = int(os.environ.get("TRD_REPS", 3))
ny = int(os.environ.get("TRD_NY", 720))
nx = int(os.environ.get("TRD_NX", 1440))
STEPS = [int(k) for k in os.environ.get("TRD_STEPS", "40,100").split(",")]
HOST_CELLS = int(os.environ.get("TRD_HOST_CELLS", 5000))
SCIPY_CELLS = int(os.environ.get("TRD_SCIPY_CELLS", 300))
C = ny * nx
eng = get_engine(0)
print(json.dumps({"device": torch.cuda.get_device_name(0), "reps": REPS, "ny": ny, "nx": nx, "steps": STEPS}), flush=True)


def med(v):
    return {"ms_median": round(statistics.median(v), 3), "ms_min": round(min(v), 3), "ms_max": round(max(v), 3)}


def wall(fn):
    out = []
    for _ in range(REPS + 1):
        eng.sync()
        t0 = time.perf_counter()
        fn()
        eng.sync()
        out.append((time.perf_counter() - t0) * 1e3)
    return out[1:]


def kernel_ms(fn):
    out = []
    for _ in range(REPS + 1):
        eng.sync()
        eng.ctx.timing_reset()
        fn()
        eng.sync()
        out.append(eng.ctx.timing_get("morph")[0])
    return out[1:]


def maps(kind, G, seed):
    """float64 ``[G, C]`` on the host: land (30 %, in blocks of rows and columns as coasts are) all NaN."""
    rng = np.random.default_rng(seed)
    land = (rng.random((ny // 8 + 1, nx // 8 + 1)) < 0.3).repeat(8, axis=0).repeat(8, axis=1)[:ny, :nx].reshape(-1)
    if kind == "days":
        y = rng.poisson(20.0, (G, C)).astype(np.float64)
    else:
        y = rng.normal(1.5, 0.4, (G, C)) + np.arange(G)[:, None] * rng.normal(0, 0.01, (1, C))
        y[rng.random((G, C)) < 0.15] = np.nan
    y[:, land] = np.nan
    return y, land


for G in STEPS:
    x = np.arange(1982, 1982 + G, dtype=np.float64)
    for kind in ("days", "mean"):
        y_h, land = maps(kind, G, G)
        y = torch.from_numpy(y_h).to(eng.device)
        xd = torch.from_numpy(x).to(eng.device)
        ocean_waves = int((~land.reshape(-1))[: C // 64 * 64].reshape(-1, 64).any(axis=1).sum()) + (C % 64 > 0)
        head = {"G": G, "maps": kind, "land_share": round(float(land.mean()), 3)}
        eng.ctx.timing_enable(True)
        res = {}
        ks = kernel_ms(lambda: res.__setitem__("st", eng.trend_stats(y, xd)))
        st = {k: v.cpu().numpy() for k, v in res["st"].items()}
        ranks = torch.from_numpy(mt.slope_ranks(st["n"], st["ties"], 0.05)).to(eng.device)
        kq = kernel_ms(lambda: res.__setitem__("sel", eng.trend_select(y, xd, ranks)))
        eng.ctx.timing_enable(False)
        div = 64 * (G * (G - 1) // 2) * 64 * ocean_waves
        print(json.dumps(dict(head, variant="ks: marex_trend_stats_f64", **med(ks))), flush=True)
        print(json.dumps(dict(head, variant="kq: marex_trend_select_f64, 4 ranks", **med(kq), divisions_derived=div,
                              divisions_per_s=round(div / statistics.median(kq) * 1e3, -9))), flush=True)
        r = wall(lambda: res.__setitem__("r", marex_amd.cell_trends(y.view(G, ny, nx), x=x)))
        print(json.dumps(dict(head, variant="r: cell_trends, resident float64 maps", **med(r))), flush=True)
        y32 = y_h.astype(np.float32).reshape(G, ny, nx)
        h = wall(lambda: res.__setitem__("h", marex_amd.cell_trends(y32, x=x)))
        print(json.dumps(dict(head, variant="h: cell_trends, host float32 maps (uploaded)", **med(h))), flush=True)
        # (n) the NumPy oracle on a sample of ocean cells, scaled
        ocean = np.flatnonzero(~land)
        pick = ocean[:HOST_CELLS]
        sub = np.ascontiguousarray(y_h[:, pick])
        rk = ranks.cpu().numpy()[:, pick]
        nt = []
        for _ in range(2):
            t0 = time.perf_counter()
            o_st = to.stats(sub, x)
            o_sel = to.select(sub, x, rk)
            nt.append((time.perf_counter() - t0) * 1e3)
        for k in ("n", "s", "ties", "med", "sums"):
            np.testing.assert_array_equal(st[k][..., pick], o_st[k], err_msg=k)
        np.testing.assert_array_equal(res["sel"].cpu().numpy()[:, pick], o_sel)
        scaled = min(nt) / pick.size * ocean.size
        print(json.dumps(dict(head, variant="n: NumPy oracle (stats + select), SCALED from a sample to the ocean cells",
                              cells_timed=int(pick.size), ms_timed=round(min(nt), 1), ms_scaled=round(scaled, 0),
                              kernels_equal_oracle_on_sample=True,
                              resident_call_beats_it=bool(statistics.median(r) < scaled))), flush=True)
        assert statistics.median(r) < scaled, "the whole call from resident maps must beat the NumPy oracle"
        try:
            from scipy import stats as sps
        except ImportError:
            sps = None
        if sps is not None:
            some = ocean[:: max(1, ocean.size // SCIPY_CELLS)][:SCIPY_CELLS]
            t0 = time.perf_counter()
            for c in some:
                v = y_h[:, c]
                ok = np.isfinite(v)
                sps.theilslopes(v[ok], x[ok], 0.95)
            per = (time.perf_counter() - t0) * 1e3 / some.size
            print(json.dumps(dict(head, variant="s: scipy.stats.theilslopes per cell, SCALED from a sample to the ocean cells",
                                  cells_timed=int(some.size), ms_per_cell=round(per, 4), ms_scaled=round(per * ocean.size, 0))),
                  flush=True)
        del y, res, ranks
        torch.cuda.empty_cache()
