"""Per-cell trends of a series of maps: Theil-Sen slope with confidence bounds, Mann-Kendall test, least squares.

The annual maps of ``local_intensity``, ``cell_events``, ``event_occurrence`` and ``compound_events`` (``by="year"``) exist to
answer where a metric changes, by how much, and whether the change is significant (Oliver et al. 2018).  The robust
answer is O(G^2) per cell -- the median of all pairwise slopes, the sum of their signs -- and a host loop over a 0.25 degree
field takes minutes per metric.  Here two launches do it (``marex_trend_stats_f64``, ``marex_trend_select_f64``, DESIGN.md
section 4): the first gives the exact integers of the test, the medians and the least-squares sums, the second exact order
statistics of the pairwise slopes at the four ranks the host derives from those integers.  The maps stay on the device; the
small ``[k, cells]`` tables come to the host once.
"""
from __future__ import annotations

import math
from functools import partial
from statistics import NormalDist

import numpy as np

from . import _stream
from .exceptions import ConfigurationError, TrackingError, create_data_validation_error
from .track import _host, _tensor_of

MAX_STEPS = 256  # HotPath.TREND_MAX_STEPS
_I32_MAX = 2**31 - 1
#: torch has every conversion of these on the device; other real types (uint16/32/64, float16) become float64 on the host
_DEVICE_CONVERTS = ("float64", "float32", "int64", "int32", "int16", "int8", "uint8")


def device_bytes(G: int, C: int, copy: bool, upload_item: int) -> int:
    """What a call holds on the device at once: the float64 copy of the maps unless they are read in place, the maps as
    uploaded where they are converted there, the results of both launches and the ranks."""
    G, C = int(G), int(C)
    return (8 * G * C if copy else 0) + int(upload_item) * G * C + (3 * 4 + 7 * 8) * C + 4 * (4 + 8) * C + 8 * G + 32


def _plan(maps, x, alpha, var) -> dict:
    """Everything that can be refused or derived without a device."""
    if hasattr(maps, "data_vars"):
        if var is None:
            raise ConfigurationError("cell_trends: a Dataset needs var=<name of the variable to take>",
                                     details=f"the Dataset holds {sorted(maps.data_vars)}")
        if var not in maps.data_vars:
            raise ConfigurationError(f"cell_trends: the Dataset has no variable {var!r}",
                                     details=f"it holds {sorted(maps.data_vars)}")
        maps = maps[var]
    elif var is not None:
        raise ConfigurationError("cell_trends: var names a variable of a Dataset", details=f"maps is a {type(maps).__name__}")
    if isinstance(alpha, bool) or not isinstance(alpha, (int, float, np.floating)) or not 0.0 < float(alpha) < 1.0:
        raise ConfigurationError("alpha must lie strictly between 0 and 1", details=f"alpha={alpha!r}")
    if _tensor_of(maps) is None and not hasattr(maps, "shape"):
        maps = np.asarray(maps)
    shape = tuple(int(k) for k in maps.shape)
    if len(shape) not in (2, 3):
        raise create_data_validation_error("maps must be (group, y, x) or (group, cells)", details=f"got shape {shape}")
    if _stream._kind(maps) not in "if":
        raise create_data_validation_error("maps must hold real numbers", details=f"Found dtype {_stream._dtype_name(maps)}",
                                           data_info={"actual_dtype": _stream._dtype_name(maps)})
    G, C = shape[0], int(np.prod(shape[1:]))
    if not 2 <= G <= MAX_STEPS:
        raise create_data_validation_error(f"cell_trends takes 2 .. {MAX_STEPS} maps",
                                           details=f"maps has {G} along its leading dimension")
    if C >= _I32_MAX:
        raise TrackingError(f"cell_trends: a map of {C} cells reaches 2^31 - 1")
    gname, gv = _stream._time_of(maps, G)
    if x is not None:
        xv = np.asarray(_host(x))
    elif gv is not None and gv.dtype.kind in "iuf":
        xv = gv
    else:
        xv = np.arange(G)
    if xv.shape != (G,) or xv.dtype.kind not in "iuf":
        raise create_data_validation_error(f"x must hold one real number per map ({G})",
                                           details=f"got shape {xv.shape}, dtype {xv.dtype}")
    xv = xv.astype(np.float64)
    if not np.isfinite(xv).all() or not (np.diff(xv) > 0).all() or not np.isfinite(xv[-1] - xv[0]):
        raise create_data_validation_error("x must be finite and strictly increasing",
                                           details=f"x = {xv[:8]}{' ...' if G > 8 else ''}")
    dims = tuple(getattr(maps, "dims", ()) or ())
    sdims = dims[1:] if dims else (("y", "x") if len(shape) == 3 else ("cells",))
    coords = {}
    for k, c in (getattr(maps, "coords", None) or {}).items():
        cd = tuple(getattr(c, "dims", ()) or ())
        if cd and all(d in sdims for d in cd):
            coords[k] = (cd, np.asarray(_host(c)))
    return dict(maps=maps, shape=shape, G=G, C=C, x=xv, alpha=float(alpha), gname=gname, sdims=sdims, scoords=coords)


def slope_ranks(n, ties, alpha: float) -> np.ndarray:
    """int32 ``[4, C]``: the 0-based ranks of the lower and upper middle slope and of the confidence bounds among the
    ``P = n (n - 1) / 2`` sorted slopes, the rule of ``scipy.stats.theilslopes``."""
    n64 = np.asarray(n).astype(np.int64)
    P = n64 * (n64 - 1) // 2
    v18 = n64 * (n64 - 1) * (2 * n64 + 5) - np.asarray(ties).astype(np.int64)
    z = NormalDist().inv_cdf(alpha / 2.0)
    sigma = np.sqrt(v18 / 18.0)
    rl = np.maximum(np.round((P + z * sigma) / 2.0).astype(np.int64) - 1, 0)
    ru = np.minimum(np.round((P - z * sigma) / 2.0).astype(np.int64), P - 1)
    return np.stack([(P - 1) // 2, P // 2, rl, ru]).astype(np.int32)


def mann_kendall(n, s, ties):
    """``(mk_var, mk_z, mk_p)`` float64 from the exact integers; z and p once per distinct (S, v18)."""
    n64, s64 = np.asarray(n).astype(np.int64), np.asarray(s).astype(np.int64)
    v18 = n64 * (n64 - 1) * (2 * n64 + 5) - np.asarray(ties).astype(np.int64)
    key, inv = np.unique((s64 + (1 << 20)) * (1 << 32) + v18, return_inverse=True)  # |S| < 2^15, 0 <= v18 < 2^26
    zt, pt = np.empty(key.size, np.float64), np.empty(key.size, np.float64)
    for k, kv in enumerate(key.tolist()):
        S, v = (kv >> 32) - (1 << 20), kv & 0xFFFFFFFF
        var = v / 18.0
        z = 0.0 if S == 0 or var == 0.0 else (S - 1) / math.sqrt(var) if S > 0 else (S + 1) / math.sqrt(var)
        zt[k], pt[k] = z, math.erfc(abs(z) / math.sqrt(2.0))
    few = n64 < 2
    inv = inv.reshape(n64.shape)
    return v18 / 18.0, np.where(few, np.nan, zt[inv]), np.where(few, np.nan, pt[inv])


def _device_maps(eng, p):
    """``(get, copy, item)``: ``get()`` gives the maps as float64 ``[G, C]`` on the engine's device; ``copy``: that is a
    new tensor, not the caller's; ``item``: bytes per sample that the way there takes besides."""
    import torch

    maps, G, C = p["maps"], p["G"], p["C"]
    t = _tensor_of(maps)
    if t is None:
        h = np.asarray(maps.values if hasattr(maps, "values") else maps).reshape(G, C)
        if h.dtype.name not in _DEVICE_CONVERTS:
            h = h.astype(np.float64)
        return (lambda: torch.from_numpy(np.ascontiguousarray(h)).to(eng.device).to(torch.float64), True,
                0 if h.dtype == np.float64 else h.dtype.itemsize)
    if t.device == eng.device and t.dtype == torch.float64 and t.is_contiguous():
        return (lambda: t.reshape(G, C)), False, 0  # read in place
    return (lambda: t.to(eng.device).to(torch.float64).contiguous().reshape(G, C), True,
            0 if t.dtype == torch.float64 and t.is_contiguous() else t.element_size())


def _device_pass(p, device):
    """Both launches: the host copies of ``n``, ``s``, ``ties``, ``med``, ``sums`` and of the four selected slopes."""
    from .detect import get_engine

    G, C = p["G"], p["C"]
    if C == 0:
        zi, zf = np.zeros((C,), np.int32), lambda k: np.zeros((k, C), np.float64)  # noqa: E731
        return {"n": zi, "s": zi, "ties": zi, "med": zf(2), "sums": zf(5), "sel": zf(4)}
    import torch

    eng = get_engine(0 if device is None else device)
    get, copy, item = _device_maps(eng, p)
    need, free = device_bytes(G, C, copy, item), _stream._free_bytes(eng)
    if need > free:
        raise TrackingError(f"cell_trends: needs {need / 1e9:.3f} GB of device memory, {free / 1e9:.3f} GB are free",
                            details=f"{need} bytes: {8 * G * C if copy else 0} of the {G} x {C} maps as float64 (0 where they "
                                    f"are read in place), {item * G * C} of the maps as given, {68 * C} of statistics and "
                                    f"{48 * C} of ranks and slopes; {free} bytes are free",
                            suggestions=["Call cell_trends on blocks of cells", "Free device memory held by other results"])
    y = get()
    xd = torch.from_numpy(p["x"]).to(eng.device)
    st = eng.trend_stats(y, xd)
    r = {k: st[k].cpu().numpy() for k in ("n", "s", "ties", "med", "sums")}
    r["sel"] = eng.trend_select(y, xd, slope_ranks(r["n"], r["ties"], p["alpha"])).cpu().numpy()
    return r


def cell_trends(maps, x=None, alpha=0.05, var=None, device=None):
    """Where a metric changes, by how much, and whether the change is significant: per cell the Theil-Sen slope with its
    confidence bounds, the Mann-Kendall test and the least-squares line of a series of maps, on the device.

    ``maps``: ``[G, y, x]`` or ``[G, cells]``, ``2 <= G <= 256`` -- a DataArray, an array or a device tensor of any real
    dtype (converted to float64 on the device; integer counts and float32 convert exactly), on the host or device
    resident; the ``by="year"`` outputs of ``local_intensity``, ``cell_events``, ``event_occurrence`` and
    ``compound_events`` fit as they are.  A Dataset is taken by ``var=`` (:class:`ConfigurationError` without).  A sample
    that is not finite is a missing sample of its cell (``intensity_mean`` of a year without extreme days); a cell
    without a valid sample is land.

    ``x``: the abscissae, one per map; by default the leading dimension's coordinate where it is numeric (``year``),
    else ``arange(G)``.  They must be finite and strictly increasing as float64 (:class:`DataValidationError`
    otherwise); irregular spacing is fine.  ``0 < alpha < 1``.  Every refusal comes before any device work; a call that
    does not fit the free device memory raises :class:`TrackingError` with the byte counts.

    Returns a Dataset over the spatial dimensions of the maps, with ``n`` the valid samples of a cell, ``P = n (n - 1) / 2``
    and the slopes ``((y_j - y_i) / (x_j - x_i)) + 0.0`` of its pairs ``i < j`` of valid samples:

    * exact integers: ``n`` (int32), ``mk_s`` (int32, the sum of ``sign(y_j - y_i)``), ``mk_var`` (float64 ``v18 / 18.0``,
      ``v18 = n (n - 1)(2 n + 5)`` less ``t (t - 1)(2 t + 5)`` per group of ``t`` equal samples);
    * from them in float64 on the host: ``mk_z`` (``(S - 1) / sqrt(var)``, ``(S + 1) / sqrt(var)`` or 0 for positive,
      negative, zero ``S``; 0 where ``var`` is 0), ``mk_p`` (``erfc(|z| / sqrt(2))``), ``significant`` (bool,
      ``mk_p < alpha``);
    * exact selections among the sorted slopes: ``sen_slope`` (``0.5 * (s[(P - 1) // 2] + s[P // 2])``), ``sen_slope_lo``
      and ``sen_slope_hi`` (the ranks of ``scipy.stats.theilslopes`` at confidence ``1 - alpha``), ``sen_intercept``
      (``median(y) - sen_slope * median(x)`` over the valid samples, scipy's ``method="separate"``);
    * least squares from sums taken in ascending step order without fused multiply-add: ``ols_slope`` (``Sxy / Sxx``),
      ``ols_intercept``, ``ols_stderr`` (NaN for ``n < 3``).

    The Mann-Kendall and slope outputs are NaN where ``n < 2``."""
    from .xr_compat import Dataset

    p = _plan(maps, x, alpha, var)
    r = _device_pass(p, device)
    n, s, sel, (med_y, med_x), (xbar, ybar, sxx, sxy, syy) = r["n"], r["s"], r["sel"], r["med"], r["sums"]
    mk_var, mk_z, mk_p = mann_kendall(n, s, r["ties"])
    with np.errstate(invalid="ignore", divide="ignore"):
        sen = 0.5 * (sel[0] + sel[1])
        ols = sxy / sxx
        rad = (syy - sxy * sxy / sxx) / (n - 2) / sxx
        stderr = np.where(n < 3, np.nan, np.sqrt(np.where(rad < 0, 0.0, rad)))
        data = {"n": n, "mk_s": s, "mk_var": mk_var, "mk_z": mk_z, "mk_p": mk_p, "significant": mk_p < p["alpha"],
                "sen_slope": sen, "sen_slope_lo": sel[2], "sen_slope_hi": sel[3], "sen_intercept": med_y - sen * med_x,
                "ols_slope": ols, "ols_intercept": ybar - ols * xbar, "ols_stderr": stderr}
    space = partial(_stream.space, p)
    return Dataset({k: space(np.asarray(v)) for k, v in data.items()})
