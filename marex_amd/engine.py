"""Device pipeline of the hot path: torch owns HBM buffers and streams, the HIP library does the work.

``HotPath`` is the array-level engine underneath :func:`marex_amd.detect.preprocess_data`.  It takes
``[T, C]`` float32 device tensors (C-order ``(time, cells)`` exactly like the reference's
``(time, lat, lon)`` arrays) plus the host calendar / bin tables and calls the C ABI
(``include/marex_hip.h``) stage by stage.  No stage has a CPU implementation here.
"""

from __future__ import annotations

import ctypes as C
from dataclasses import dataclass
from typing import Dict, List, Optional, Tuple

import numpy as np
import torch

from . import _lib
from ._keys import key_float
from .binning import BinTable
from .calendar import N_DOY, CalendarPlan
from .exceptions import ConfigurationError, ProcessingError, TrackingError, create_data_validation_error
from .track_mesh import mesh_moments_finish


import logging

_log = logging.getLogger("marex_amd")
_noted: set = set()


def _note_path(msg: str) -> None:
    """INFO, once per distinct message: a call took a slower kernel family than the tuned one (same results; README "kernel
    families") -- so that a user with, say, smooth_days_baseline=31 sees why the anomaly stage runs at a quarter of the speed."""
    if msg not in _noted:
        _noted.add(msg)
        _log.info(msg)


def shifting_kernel_family(W: int, S: int, C: int, lists: bool) -> str:
    """Which anomaly kernel ``marex_shifting_baseline[_tails]_f32`` takes for a gap-free daily calendar (csrc/marex_shifting.hip:
    ``lean_instance`` / ``fast_ws``; irregular calendars send single chunks to the general kernel on top of this)."""
    fast_w = W in (3, 4, 5, 6, 7, 10, 13, 15)
    fast = fast_w if S == 21 else (S in (11, 15) and W in (5, 10, 15))
    if S == 21 and W in (5, 15) and C >= 4 and C % 4 == 0:
        return "lean"
    return "fast" if fast else "general"


#: cells one marex_label3d_i32 call takes (int32 parents, 2^31 - 1 refused): the default and the largest labelling block
LABEL_BLOCK_CELLS = 2**31 - 2


def plan_time_blocks(T: int, C: int, max_block_cells: Optional[int] = None) -> List[Tuple[int, int]]:
    """Contiguous time blocks ``[(t0, t1), ...]`` covering ``[0, T)`` for the blocked labelling of a ``[T, C]`` field:
    every block holds as many whole timesteps as fit ``max_block_cells`` cells (default and upper limit 2^31 - 2), the
    last one what remains.  :class:`TrackingError` when a single timestep does not fit.  Needs no GPU."""
    T, C = int(T), int(C)
    if T <= 0 or C <= 0:
        raise TrackingError(f"cannot plan labelling blocks for an empty field ({T} steps of {C} cells)")
    if max_block_cells is not None and int(max_block_cells) <= 0:
        raise TrackingError(f"max_block_cells must be positive, got {max_block_cells}")
    limit = LABEL_BLOCK_CELLS if max_block_cells is None else min(int(max_block_cells), LABEL_BLOCK_CELLS)
    if C > limit:
        raise TrackingError(f"one timestep of {C} cells exceeds the labelling block of {limit} cells",
                            details="a block is at least one timestep; a single slice must stay below 2^31 - 1 cells")
    steps = limit // C
    return [(t0, min(T, t0 + steps)) for t0 in range(0, T, steps)]


def _key_to_float(key: int) -> float:
    """Inverse of the order-preserving uint32 key used for the device-side min / max of thresholds."""
    return float(key_float([key])[0])


def label_tables(what: str, specs) -> Dict[str, Optional[np.ndarray]]:
    """``{name: int32 vector or None}`` of the ``(name, values or None, length or None)`` in ``specs``; anything but an
    integer vector of that length with values inside int32 is refused.  Needs no device."""
    tabs = {}
    for name, v, n in specs:
        if v is None:
            tabs[name] = None
            continue
        h = np.asarray(v)
        if h.ndim != 1 or h.dtype.kind not in "iu" or (n is not None and h.size != n) or \
                (h.size and (int(h.min()) < -2**31 or int(h.max()) > 2**31 - 1)):
            raise ProcessingError(f"{what}: {name} must be a vector of int32 values" + (f" of length {n}" if n else ""),
                                  details=f"got {h.dtype} {h.shape}")
        tabs[name] = h.astype(np.int32)
    return tabs


def _linear_percentile(values: torch.Tensor, q: float) -> float:
    """``np.percentile(values, 100 q)`` ("linear") of a non-empty 1-D device tensor: two order statistics from a device
    sort, then NumPy's own lerp on the host -- from the lower value below g = 0.5, from the upper one above: that is what
    makes the result equal NumPy's to the bit."""
    n = int(values.numel())
    srt = torch.sort(values).values
    virt = (n - 1) * float(np.float64(q * 100.0) / 100.0)
    lo = int(np.floor(virt))
    g = virt - lo
    hi = min(lo + 1, n - 1)
    a, b = float(srt[lo].item()), float(srt[hi].item())
    return a + (b - a) * g if g < 0.5 else b - (b - a) * (1.0 - g)


def check_pool_caps(nb: int, max_bucket: int, wd: int, K: int, C: Optional[int] = None) -> None:
    """What the pooled threshold kernel (``neighbour_rings_hobday``) takes: the list kernels' table and bucket sizes, and a
    pooled window of at most 65535 samples (its 16-bit packed counters; the gridded kernel's cap with ``K`` for ``ws * ws``)."""
    if nb <= 511 and 1 <= max_bucket <= 128 and max_bucket * wd * K <= 65535 and (C is None or C <= (1 << 24)):
        return
    raise ConfigurationError(
        "neighbour_rings_hobday is not supported for this configuration",
        details=f"The pooled threshold kernel takes at most 511 bins (here {nb}), day-of-year buckets of at most 128 rows "
                f"(here {max_bucket}) and pooled windows of at most 65535 samples (here {max_bucket} x {wd} days x {K} cells).",
        suggestions=["Use a smaller window_days_hobday or fewer neighbour rings", "Use a coarser precision or a smaller max_anomaly",
                     "Remove the neighbour_rings_hobday parameter"],
        context={"bins": nb, "max_bucket": max_bucket, "window_days_hobday": wd, "pool_members": K},
    )


@dataclass
class DeviceCalendar:
    """Calendar tables resident on the device."""

    tindex: torch.Tensor
    year_plan: torch.Tensor
    out_index: torch.Tensor
    rowb_index: torch.Tensor
    doy_start: torch.Tensor
    doy_rows: torch.Tensor
    plan: CalendarPlan


def pair_table_cap(runs: int) -> int:
    """Entries of the overlap pair table for ``runs`` runs of equal pairs: a power of two of at least 64 with a load
    factor <= 1/2 even if every run were a distinct pair."""
    return max(64, 1 << (2 * runs - 1).bit_length())


class HotPath:
    def __init__(self, device: int | torch.device = 0, own_stream: bool = False):
        if not torch.cuda.is_available():
            raise ProcessingError(
                "marex_amd needs a HIP device (torch.cuda.is_available() is False)",
                details="the hot path has no CPU implementation",
            )
        self.device = torch.device("cuda", device if isinstance(device, int) else (device.index or 0))
        self.ctx = _lib.Context(self.device.index)
        self.lib = self.ctx.lib
        self._tables: Dict[tuple, tuple] = {}
        #: None = choose per configuration (tails_plan); "tails" / "bins" force the representation of the dayofyear
        #: histograms behind the approximate Hobday thresholds (same results either way; tests use it)
        self.hobday_path: Optional[str] = None
        #: a stream of its own (engines that share a device with another engine run under ``torch.cuda.stream(self.stream)``)
        self.stream = torch.cuda.Stream(self.device) if own_stream else None
        self._bind_stream()

    #: tests set this: fresh output buffers are filled with a byte pattern, so that an element a kernel forgets to write
    #: shows up as garbage instead of as the zeros a fresh allocation often holds
    POISON = False

    @staticmethod
    def _buf(wsp: Optional[dict], name: str, shape, dtype, device) -> torch.Tensor:
        """Output buffer: fresh when ``wsp`` is None, otherwise cached in the workspace dict and reused
        (no allocator traffic in the steady state, outputs of the previous call are overwritten)."""
        if wsp is None:
            t = torch.empty(shape, dtype=dtype, device=device)
            if HotPath.POISON and t.numel():
                t.view(torch.uint8).fill_(0xCD)
            return t
        n = 1
        for d in shape:
            n *= int(d)
        flat = wsp.get(name)
        if flat is None or flat.dtype != dtype or flat.numel() < n:
            flat = torch.empty((max(n, 1),), dtype=dtype, device=device)  # grows to the largest request, then stays
            wsp[name] = flat
        return flat[:n].view(shape)

    # ------------------------------------------------------------------ plumbing
    def _bind_stream(self) -> None:
        self.ctx.set_stream(torch.cuda.current_stream(self.device).cuda_stream)

    def call(self, name: str, *args) -> None:
        """The one way to a context-taking ``marex_*`` function: launches on torch's current stream of this device,
        passes the context handle first and every tensor as its address (``None`` is NULL), and raises
        :class:`ProcessingError` naming ``name`` when the library returns an error code.  A tensor has to be contiguous and
        on this engine's device -- anything else would hand the kernel a valid-looking address of the wrong bytes -- and is
        refused before the library is reached; ``argument k`` counts as in include/marex_hip.h with the context as 0."""
        self._bind_stream()
        argv = []
        for k, a in enumerate(args, 1):
            if isinstance(a, torch.Tensor):
                if a.device != self.device or not a.is_contiguous():
                    raise ProcessingError(f"{name}: argument {k} must be a contiguous tensor on {self.device}",
                                          details=f"got {a.dtype} {tuple(a.shape)} with strides {a.stride()} on {a.device}")
                a = a.data_ptr()
            argv.append(a)
        self.ctx.check(getattr(self.lib, name)(self.ctx.handle, *argv), name)

    def _dev(self, a: np.ndarray, dtype=None) -> torch.Tensor:
        t = torch.from_numpy(np.ascontiguousarray(a if dtype is None else a.astype(dtype)))
        return t.to(self.device, non_blocking=False)

    def upload_calendar(self, cal: CalendarPlan) -> DeviceCalendar:
        return DeviceCalendar(
            tindex=self._dev(cal.tindex, np.int32),
            year_plan=self._dev(cal.year_plan(), np.int32),
            out_index=self._dev(cal.out_index, np.int32),
            rowb_index=self._dev(cal.rowb_index, np.int32),
            doy_start=self._dev(cal.doy_start, np.int32),
            doy_rows=self._dev(cal.doy_rows, np.int32),
            plan=cal,
        )

    def sync(self) -> None:
        self.ctx.sync()

    def ctx_opt(self, name: str, default: int) -> int:
        """Python-side view of a context option set through ``ctx.options`` / ``set_option`` (host-side switches)."""
        return int(self.ctx.py_opts.get(name, default))

    @staticmethod
    def bins_shape(T_out: int, C: int):
        """Shape of the blocked bin matrix: ``[ceil(C/16), T_out, 16]`` (include/marex_hip.h)."""
        return ((C + 15) // 16, T_out, 16)

    @staticmethod
    def bins_to_rows(binsb: torch.Tensor, C: int) -> torch.Tensor:
        """Blocked bin matrix -> plain ``[T_out, C]`` (dayofyear-sorted rows); for tests / inspection."""
        nblk, T_out, _ = binsb.shape
        return binsb.permute(1, 0, 2).reshape(T_out, nblk * 16)[:, :C]

    def bin_tables(self, bins: BinTable):
        """(edges, centres) of a bin table on the device, uploaded once per table CONTENT (callers build a fresh BinTable
        per call; a handful of distinct tables at most stay resident)."""
        key = (float(bins.precision), float(bins.max_anomaly), int(bins.nb), bins.edges.tobytes())
        if key not in self._tables:
            if len(self._tables) >= 8:
                self._tables.pop(next(iter(self._tables)))
            self._tables[key] = (self._dev(bins.edges, np.float32), self._dev(bins.centres, np.float32))
        return self._tables[key]

    # ------------------------------------------------------------------ synthetic field
    def synth_field(self, tab, cell_base: int = 0, out: Optional[torch.Tensor] = None) -> torch.Tensor:
        """Device evaluation of :func:`marex_amd.synth.synth_field` (bit-identical)."""
        T, Cn = tab.T, tab.C
        if out is None:
            out = torch.empty((T, Cn), dtype=torch.float32, device=self.device)
        bufs = [
            self._dev(tab.mean, np.float32), self._dev(tab.amp, np.float32), self._dev(tab.hemi, np.uint8),
            self._dev(tab.land, np.uint8), self._dev(tab.seas, np.float32), self._dev(tab.trend, np.float32),
        ]
        self.call("marex_synth_sst_f32", *bufs, tab.seed, int(cell_base), T, Cn, out)
        self.sync()  # the small tables above must outlive the kernel
        return out

    # ------------------------------------------------------------------ what the anomaly kernels share
    @staticmethod
    def _check_shifting_input(x: torch.Tensor, cal: CalendarPlan) -> None:
        assert x.dtype == torch.float32 and x.dim() == 2
        if cal.T != x.shape[0]:
            raise ProcessingError("calendar length does not match the time axis of x")
        if cal.has_duplicates:
            raise ConfigurationError(
                "shifting_baseline needs at most one timestep per (year, dayofyear)",
                details="sub-daily time axes are not supported by the device path",
            )

    def _anomaly_buffers(self, wsp: Optional[dict], name: str, T_out: int, Cn: int, second_stage: bool = False):
        """``(out [T_out, Cn] float32 named name, mask [Cn] uint8, invalid [Cn] int32)`` of an anomaly kernel."""
        out = self._buf(wsp, name, (T_out, Cn), torch.float32, self.device)
        mask = self._buf(wsp, "mask2" if second_stage else "mask", (Cn,), torch.uint8, self.device)
        invalid = self._buf(wsp, "invalid2" if second_stage else "invalid", (Cn,), torch.int32, self.device)
        return out, mask, invalid

    def _reference_rows(self, cal: CalendarPlan, reference_period) -> Optional[torch.Tensor]:
        """uint8 ``[T]``: 1 for the timesteps of the years ``reference_period = (first, last)``; None without a period."""
        if reference_period is None:
            return None
        return self._dev(((cal.year >= reference_period[0]) & (cal.year <= reference_period[1])).astype(np.uint8))

    # ------------------------------------------------------------------ stage a3+a5+a6+a7 (+a10 binning)
    def shifting_baseline(
        self,
        x: torch.Tensor,
        dcal: DeviceCalendar,
        W: int,
        S: int,
        bins: Optional[BinTable] = None,
        write_clim: bool = False,
        wsp: Optional[dict] = None,
    ) -> Dict[str, torch.Tensor]:
        cal = dcal.plan
        self._check_shifting_input(x, cal)
        T, Cn = x.shape
        T_out = cal.T_out
        out, mask, invalid = self._anomaly_buffers(wsp, "anom", T_out, Cn)
        if write_clim:
            out.fill_(float("nan"))
        invalid.zero_()
        edges = binsb = None
        if bins is not None and not write_clim:
            edges = self.bin_tables(bins)[0]
            binsb = self._buf(wsp, "bins", self.bins_shape(T_out, Cn), torch.int16, self.device)
        self.call("marex_shifting_baseline_f32", x, T, Cn, dcal.year_plan, cal.n_cal_years, int(W), int(S), int(write_clim),
                  edges, bins.nb if edges is not None else 0, T_out, out, binsb, mask, invalid)
        res = {"out": out, "mask": mask, "invalid_count": invalid, "_keep": edges}
        if binsb is not None:
            res["bins"] = binsb
        return res

    # ------------------------------------------------------------------ stage a10/a11
    def hobday_thresholds(
        self,
        binsb: torch.Tensor,
        first_anom: torch.Tensor,
        dcal: DeviceCalendar,
        bins: BinTable,
        q: float,
        wd: int,
        ws: int,
        ny: int,
        nx: int,
        rows: Optional[tuple] = None,
        wsp: Optional[dict] = None,
    ) -> Dict[str, object]:
        """``rows=(row0, row1)`` restricts the output to the grid rows a latitude shard owns."""
        T_out, Cn = binsb.shape[1], first_anom.shape[-1]
        row0, row1 = rows if rows is not None else (0, max(ny, 1))
        thr, stats = self._threshold_buffers(wsp, Cn)
        centres = self.bin_tables(bins)[1]
        self.call("marex_hobday_thresholds_f32", binsb, T_out, Cn, int(ny), int(nx), dcal.doy_start, dcal.plan.max_bucket,
                  first_anom, centres, bins.nb, float(q), int(wd), int(ws), float(bins.lower_bound), float(bins.upper_bound),
                  int(row0), int(row1), thr, stats)
        return {"thr_doy_major": thr, "stats_dev": stats, "_keep": centres}

    def _threshold_buffers(self, wsp: Optional[dict], Cn: int):
        """``(thr_doy_major [366, Cn] float32, thr_stats)`` of the dayofyear threshold kernels, the statistics reset."""
        thr = self._buf(wsp, "thr_doy_major", (N_DOY, Cn), torch.float32, self.device)
        stats = self._buf(wsp, "thr_stats", (8,), torch.int32, self.device)  # marex_thr_stats: 8 x uint32
        stats.zero_()
        stats[0:1].fill_(-1)  # min_key = 0xFFFFFFFF (a fill kernel: `stats[0] = -1` would be a blocking host-to-device copy)
        return thr, stats

    @staticmethod
    def decode_thr_stats(stats_dev: torch.Tensor) -> Dict[str, float]:
        s = stats_dev.cpu().numpy().view(np.uint32)
        kmin, kmax = int(s[0]), int(s[1])
        if len(s) > 4 and int(s[4]):  # the straggler-pass limit of the list threshold kernel tripped (marex_tails.hip): never a result
            raise ProcessingError(
                f"threshold kernel left {int(s[4])} outputs unresolved (written as NaN)",
                details="internal error of the day-of-year threshold stage: the band search ran out of passes",
                suggestions=["force the bin-matrix kernels (engine.hobday_path = 'bins') and report the input"],
            )
        return {
            "min": _key_to_float(kmin) if kmin != 0xFFFFFFFF else float("nan"),
            "max": _key_to_float(kmax) if kmax != 0 else float("nan"),
            "n_too_low": int(s[2]),
            "n_too_high": int(s[3]),
        }

    # ------------------------------------------------------------------ stage a10/a11 on tails (default)
    #: rows per sorted list: what the extraction kernel writes / what the shifting-baseline kernel emits itself
    LIST_ROWS_EXTRACT = 32
    LIST_ROWS_SHIFT = 15

    def tails_plan(self, dcal: DeviceCalendar, bins: BinTable, q: float, wd: int, ws: int, C: Optional[int] = None) -> Optional[int]:
        """Rows of the largest dayofyear bucket when the tail kernels take this configuration, else None (bin-matrix
        kernels).  Results are identical on both paths (include/marex_hip.h, TAILS)."""
        if self.hobday_path == "bins":
            return None
        nd = dcal.plan.max_bucket
        if not (bins.nb <= 511 and 1 <= nd <= 128 and ws <= 7 and nd * wd * ws * ws <= 65535 and (C is None or C <= (1 << 24))):
            return None
        if self.hobday_path != "tails" and nd < 24 and ws > 1:
            return None  # short buckets with spatial pooling (cfg2): the bin-matrix kernels are the faster ones
        if self.hobday_path != "tails" and q < 0.5:
            return None  # the lists are read from the top: a low quantile walks most of every list (the public API stops at 60 %)
        return nd  # ws == 1: the per-cell threshold kernel (no tiles), any record length

    def fused_tails_ok(self, dcal: DeviceCalendar, bins: BinTable) -> bool:
        """The fixed-baseline kernels (plain and behind the detrend fit) can emit the key lists of their own output for buckets
        of at most 128 rows and tables of at most 511 bins.  Option FIXED_TAILS: 1 (default) = for buckets of at most 48 rows
        -- the 48-row register kernel keeps four waves per SIMD with the sorting networks in it; the 128-row one drops to two and
        measured SLOWER than kernel + extraction pass on the 100-yr field (27.9 vs 21.0 ms per band, profiles/r04_experiments.md)
        --, 2 = whenever possible, 0 = never (the extraction pass makes the lists)."""
        nd = dcal.plan.max_bucket
        mode = self.ctx_opt("FIXED_TAILS", 1)
        return bool(mode) and bool(self.ctx_opt("FIXED_REG", 1)) and 1 <= nd <= (128 if mode == 2 else 48) and bins.nb <= 511

    def _tail_buffers(self, nd: int, list_rows: int, Cn: int, edges: torch.Tensor, wsp: Optional[dict]) -> Dict[str, object]:
        """The tail-list record the threshold / mask kernels take, its lists still to be written (``edges``: the table the
        keys are made with, kept alive with the record)."""
        nper = (nd + list_rows - 1) // list_rows
        nch = 2 if list_rows <= 16 else 4
        lists = self._buf(wsp, "tails", (N_DOY, nper, nch, Cn, 8), torch.int16, self.device)
        aux = self._buf(wsp, "tails_aux", (N_DOY, Cn), torch.int32, self.device)
        return {"tails": lists, "aux": aux, "max_bucket": nd, "list_rows": list_rows, "_keep": edges}

    def tail_extract(self, anom: torch.Tensor, dcal: DeviceCalendar, bins: BinTable, wsp: Optional[dict] = None,
                     list_rows: Optional[int] = None):
        """Sorted key lists of every (dayofyear, cell) bucket of ``anom`` (include/marex_hip.h, TAILS)."""
        T_out, Cn = anom.shape
        edges = self.bin_tables(bins)[0]
        nd = dcal.plan.max_bucket
        tl = self._tail_buffers(nd, int(list_rows or self.LIST_ROWS_EXTRACT), Cn, edges, wsp)
        self.call("marex_tail_extract_f32", anom, T_out, Cn, dcal.doy_start, dcal.doy_rows, nd, edges, bins.nb,
                  tl["list_rows"], tl["tails"], tl["aux"])
        return tl

    def shifting_tails_ok(self, dcal: DeviceCalendar) -> bool:
        """The anomaly kernel emits its own tails for buckets of at most 6 lists of 15 rows (option SHIFT_TAILS=0: never)."""
        return bool(self.ctx_opt("SHIFT_TAILS", 1)) and dcal.plan.max_bucket <= 6 * self.LIST_ROWS_SHIFT

    def shifting_baseline_tails(self, x: torch.Tensor, dcal: DeviceCalendar, W: int, S: int, bins: BinTable,
                                wsp: Optional[dict] = None) -> Dict[str, object]:
        """Anomaly stage emitting the sorted key lists (TAILS) of its own output: no bin matrix, no extraction pass."""
        cal = dcal.plan
        self._check_shifting_input(x, cal)
        T, Cn = x.shape
        T_out = cal.T_out
        out, mask, invalid = self._anomaly_buffers(wsp, "anom", T_out, Cn)
        invalid.zero_()
        edges = self.bin_tables(bins)[0]
        nd = cal.max_bucket
        tl = self._tail_buffers(nd, self.LIST_ROWS_SHIFT, Cn, edges, wsp)
        self.call("marex_shifting_baseline_tails_f32", x, T, Cn, dcal.year_plan, cal.n_cal_years, int(W), int(S), edges,
                  bins.nb, T_out, out, mask, invalid, dcal.doy_start, dcal.doy_rows, nd, tl["tails"], tl["aux"])
        return {"out": out, "mask": mask, "invalid_count": invalid, "_keep": edges, "tails": tl}

    def hobday_thresholds_tails(self, tl: dict, anom: torch.Tensor, dcal: DeviceCalendar, bins: BinTable, q: float, wd: int,
                                ws: int, ny: int, nx: int, rows: Optional[tuple] = None, wsp: Optional[dict] = None):
        """Day-of-year thresholds from the key lists.  Option THR_LEAN (default 1): lists of 6 x 2 chunks on 1024-thread tiles
        take the lean instance of the kernel, 0 = the general body for every geometry (same bits)."""
        T_out, Cn = anom.shape
        row0, row1 = rows if rows is not None else (0, max(ny, 1))
        thr, stats = self._threshold_buffers(wsp, Cn)
        centres = self.bin_tables(bins)[1]
        self.call("marex_hobday_thresholds_tails_f32", tl["tails"], tl["aux"], int(tl["list_rows"]), anom, T_out, Cn,
                  int(ny), int(nx), int(tl["max_bucket"]), centres, bins.nb, float(q), int(wd), int(ws),
                  float(bins.lower_bound), float(bins.upper_bound), int(row0), int(row1), thr, stats)
        return {"thr_doy_major": thr, "stats_dev": stats, "_keep": centres}

    # ------------------------------------------------------------------ pooling over mesh neighbour rings
    #: most members a pool can have: the cell, three neighbours, their three neighbours each
    POOL_MAX_MEMBERS = 13

    @staticmethod
    def pool_table(neighbours_1based, rings: int) -> np.ndarray:
        """The pools of ``neighbour_rings_hobday`` as the int32 table ``[K, C]`` the pooled threshold kernel reads
        (include/marex_hip.h): row 0 is the cell, the other rows its further members in ascending order, ``-1`` = empty slot,
        no member twice, ``K`` = size of the largest pool.  ``neighbours_1based`` is ``[nv <= 3, C]``, 1-based, 0 = none; only
        listed links count (a link listed from one end is one-way) and ``pool(c, r)`` is what ``r`` steps along listed links
        reach from ``c``, ``c`` included.  Host NumPy: built once per run."""
        nbr = np.asarray(neighbours_1based)
        if nbr.ndim != 2 or nbr.shape[0] > 3 or nbr.shape[0] < 1:
            raise ValueError("neighbours must be [nv <= 3, cells]")
        if rings not in (1, 2):
            raise ValueError("rings must be 1 or 2")
        Cn = nbr.shape[1]
        n0 = nbr.astype(np.int64) - 1  # 0-based, -1 = none
        if n0.size and (n0.min() < -1 or n0.max() >= Cn):
            raise ValueError("neighbours entries must lie in 0..cells")
        cand = [n0[a] for a in range(n0.shape[0])]
        if rings == 2:
            for a in range(n0.shape[0]):
                via = n0[a]
                for b in range(n0.shape[0]):
                    cand.append(np.where(via >= 0, n0[b][np.maximum(via, 0)], -1))
        big = np.int64(Cn)  # sorts behind every cell
        m = np.stack(cand) if cand else np.empty((0, Cn), np.int64)
        m = np.where((m < 0) | (m == np.arange(Cn, dtype=np.int64)[None, :]), big, m)
        m = np.sort(m, axis=0)
        dup = np.zeros(m.shape, dtype=bool)
        dup[1:] = m[1:] == m[:-1]
        m = np.sort(np.where(dup, big, m), axis=0)
        k_more = int((m < big).sum(axis=0).max()) if m.size else 0
        tab = np.full((1 + k_more, Cn), -1, dtype=np.int32)
        tab[0] = np.arange(Cn, dtype=np.int32)
        tab[1:] = np.where(m[:k_more] < big, m[:k_more], -1).astype(np.int32)
        return tab

    def pool_plan(self, dcal: DeviceCalendar, bins: BinTable, q: float, wd: int, K: int, C: Optional[int] = None) -> int:
        """Rows of the largest dayofyear bucket when the pooled threshold kernel takes this configuration with pools of ``K``
        members; raises the ``ConfigurationError`` of ``neighbour_rings_hobday`` otherwise (pooling needs the key lists)."""
        check_pool_caps(bins.nb, dcal.plan.max_bucket, int(wd), int(K), C)
        nd = self.tails_plan(dcal, bins, q, wd, 1, C)
        if nd is None:
            raise ConfigurationError(
                "neighbour_rings_hobday needs the sorted key lists of the day-of-year histograms",
                details=f"this configuration takes the bin-matrix threshold kernels (hobday_path={self.hobday_path!r}, q={q})",
                suggestions=["Remove the neighbour_rings_hobday parameter", "Leave engine.hobday_path at None or 'tails'"],
            )
        return nd

    def hobday_thresholds_pool(self, tl: dict, anom: torch.Tensor, dcal: DeviceCalendar, bins: BinTable, q: float, wd: int,
                               pool: torch.Tensor, cells: Optional[tuple] = None, wsp: Optional[dict] = None):
        """Day-of-year thresholds from the key lists, the histogram of a cell summed over its pool (``pool``: int32 ``[K, C]``
        on the device, :meth:`pool_table`); written for ``cells=(c0, c1)`` only.  Options THR_POOL_RING (1 / 0: the first
        chunks wait in LDS / are read from global memory at every probe) and THR_POOL_BLOCKS; same bits on either path
        (DESIGN.md section 4)."""
        T_out, Cn = anom.shape
        if pool.dtype != torch.int32 or pool.dim() != 2 or pool.shape[1] != Cn:
            raise ProcessingError("hobday_thresholds_pool: the pool table must be int32 [K, cells]",
                                  details=f"got {pool.dtype} {tuple(pool.shape)} for {Cn} cells")
        c0, c1 = cells if cells is not None else (0, Cn)
        thr, stats = self._threshold_buffers(wsp, Cn)
        centres = self.bin_tables(bins)[1]
        self.call("marex_hobday_thresholds_pool_f32", tl["tails"], tl["aux"], int(tl["list_rows"]), anom, T_out, Cn,
                  int(tl["max_bucket"]), pool, int(pool.shape[0]), int(c0), int(c1), centres, bins.nb, float(q), int(wd),
                  float(bins.lower_bound), float(bins.upper_bound), thr, stats)
        return {"thr_doy_major": thr, "stats_dev": stats, "_keep": (centres, pool)}

    def _extreme_buffers(self, wsp: Optional[dict], T_out: int, Cn: int):
        """``(extreme [T_out, Cn] uint8, n_true [1] int64 = 0)`` of the compare kernels."""
        ext = self._buf(wsp, "extreme", (T_out, Cn), torch.uint8, self.device)
        n_true = self._buf(wsp, "n_true", (1,), torch.int64, self.device)
        n_true.zero_()
        return ext, n_true

    def mask_ge_doy_tails(self, tl: dict, anom: torch.Tensor, thr_doy_major: torch.Tensor, dcal: DeviceCalendar,
                          bins: BinTable, cells: Optional[tuple] = None, wsp: Optional[dict] = None):
        T_out, Cn = anom.shape
        c0, c1 = cells if cells is not None else (0, Cn)
        ext, n_true = self._extreme_buffers(wsp, T_out, Cn)
        edges = self.bin_tables(bins)[0]
        self.call("marex_mask_ge_doy_tails_f32", tl["tails"], tl["aux"], int(tl["list_rows"]), int(tl["max_bucket"]),
                  anom, edges, bins.nb, thr_doy_major, dcal.doy_start, dcal.doy_rows, T_out, Cn, int(c0), int(c1), ext, n_true)
        return {"extreme": ext, "n_true": n_true}

    def hobday_approx(self, anom: torch.Tensor, dcal: DeviceCalendar, bins: BinTable, q: float, wd: int, ws: int, ny: int,
                      nx: int, rows: Optional[tuple] = None, cells: Optional[tuple] = None, wsp: Optional[dict] = None,
                      binsb: Optional[torch.Tensor] = None, tails: Optional[dict] = None,
                      pool: Optional[torch.Tensor] = None) -> Dict[str, object]:
        """Approximate Hobday thresholds + extreme mask of an anomaly field (detect.py:1957-2004): through tails when
        ``tails_plan`` takes the configuration, else through the bin matrix (``binsb``, made here when missing).
        ``pool`` (int32 ``[K, C]``, :meth:`pool_table`): thresholds pooled over mesh neighbour rings, for ``cells`` only."""
        if pool is not None:
            self.pool_plan(dcal, bins, q, wd, int(pool.shape[0]), anom.shape[1])
            tl = tails if tails is not None else self.tail_extract(anom, dcal, bins, wsp=wsp)
            t = self.hobday_thresholds_pool(tl, anom, dcal, bins, q, wd, pool, cells=cells, wsp=wsp)
            m = self.mask_ge_doy_tails(tl, anom, t["thr_doy_major"], dcal, bins, cells=cells, wsp=wsp)
            return {"thr_doy_major": t["thr_doy_major"], "stats_dev": t["stats_dev"], "extreme": m["extreme"], "n_true": m["n_true"],
                    "path": "tails", "_keep": (tl, t["_keep"])}
        K = self.tails_plan(dcal, bins, q, wd, ws, anom.shape[1])
        if K is not None:
            tl = tails if tails is not None else self.tail_extract(anom, dcal, bins, wsp=wsp)
            t = self.hobday_thresholds_tails(tl, anom, dcal, bins, q, wd, ws, ny, nx, rows=rows, wsp=wsp)
            m = self.mask_ge_doy_tails(tl, anom, t["thr_doy_major"], dcal, bins, cells=cells, wsp=wsp)
            keep = (tl, t["_keep"])
        else:
            if binsb is None:
                binsb = self.digitize(anom, dcal, bins, wsp=wsp)
            t = self.hobday_thresholds(binsb, anom, dcal, bins, q, wd, ws, ny, nx, rows=rows, wsp=wsp)
            m = self.mask_ge_doy(anom, t["thr_doy_major"], dcal, cells=cells, wsp=wsp, binned=(binsb, bins))
            keep = (binsb, t["_keep"])
        return {"thr_doy_major": t["thr_doy_major"], "stats_dev": t["stats_dev"], "extreme": m["extreme"], "n_true": m["n_true"],
                "path": "tails" if K is not None else "bins", "_keep": keep}

    # ------------------------------------------------------------------ stage a3 verdict
    def validation_summary(self, mask: torch.Tensor, invalid_count: torch.Tensor, cells: Optional[tuple] = None,
                           wsp: Optional[dict] = None) -> torch.Tensor:
        """Device int64 ``[n_ocean, invalid_total, invalid_cells, max_invalid]`` over the (owned) cells: the numbers of
        ``_validate_data_values`` (detect.py:205-279) from the per-cell outputs of the anomaly kernels, one launch."""
        Cn = mask.shape[-1]
        c0, c1 = cells if cells is not None else (0, Cn)
        out = self._buf(wsp, "validation_summary", (4,), torch.int64, self.device)
        self.call("marex_validation_summary", mask, invalid_count, int(c0), int(c1), out)
        return out

    # ------------------------------------------------------------------ stage a9 compare
    def mask_ge_doy(
        self, anom: torch.Tensor, thr_doy_major: torch.Tensor, dcal: DeviceCalendar, cells: Optional[tuple] = None,
        wsp: Optional[dict] = None, binned: Optional[tuple] = None,
    ) -> Dict[str, torch.Tensor]:
        """``cells=(c0, c1)`` restricts compare / write / count to the owned cells of a shard.  ``binned=(bin matrix,
        BinTable)`` of these anomalies lets the kernel decide most samples from their 2-byte bin (same result)."""
        T_out, Cn = anom.shape
        c0, c1 = cells if cells is not None else (0, Cn)
        ext, n_true = self._extreme_buffers(wsp, T_out, Cn)
        if binned is not None and binned[0] is not None:
            edges = self.bin_tables(binned[1])[0]
            self.call("marex_mask_ge_doy_bins_f32", anom, binned[0], edges, int(binned[1].nb), thr_doy_major, dcal.doy_start,
                      dcal.doy_rows, T_out, Cn, int(c0), int(c1), ext, n_true)
        else:
            self.call("marex_mask_ge_doy_f32", anom, thr_doy_major, dcal.doy_start, dcal.doy_rows, T_out, Cn, int(c0), int(c1),
                      ext, n_true)
        return {"extreme": ext, "n_true": n_true}

    def transpose(self, a: torch.Tensor, wsp: Optional[dict] = None, name: str = "transposed") -> torch.Tensor:
        rows, cols = a.shape
        out = self._buf(wsp, name, (cols, rows), torch.float32, self.device)
        self.call("marex_transpose_f32", a, rows, cols, out)
        return out

    # ------------------------------------------------------------------ whole path (shifting + hobday approx)
    def shifting_hobday(
        self,
        x: torch.Tensor,
        dcal: DeviceCalendar,
        *,
        W: int,
        S: int,
        bins: BinTable,
        q: float,
        wd: int,
        ws: int,
        ny: int,
        nx: int,
        transpose_thresholds: bool = True,
        own_rows: Optional[tuple] = None,
        workspace: Optional[dict] = None,
    ) -> Dict[str, object]:
        """validation + anomaly + thresholds + mask for ``shifting_baseline`` / ``hobday_extreme`` (approximate).

        ``own_rows=(row0, row1)``: the field is a latitude shard with overlap rows; thresholds and the
        mask are produced for the owned rows only (:mod:`marex_amd.dist`).
        """
        K = self.tails_plan(dcal, bins, q, wd, ws, x.shape[1])
        fam = shifting_kernel_family(int(W), int(S), int(x.shape[1]), K is not None)
        if fam != "lean":
            _note_path(f"shifting_baseline: window_year_baseline={W}, smooth_days_baseline={S}, {x.shape[1]} cells take the "
                       f"'{fam}' anomaly kernel (tuned path: smooth_days_baseline=21, window_year_baseline in (5, 15), cells a "
                       "multiple of 4; same results)")
        if K is None:
            _note_path(f"hobday_extreme: dayofyear buckets of {dcal.plan.max_bucket} rows with window_spatial_hobday={ws}, q={q} take the bin-matrix "
                       "threshold kernels (sorted key lists need >= 24 rows per bucket or no spatial pooling; same results)")
        if K is not None and self.shifting_tails_ok(dcal):
            a = self.shifting_baseline_tails(x, dcal, W, S, bins, wsp=workspace)
        else:
            a = self.shifting_baseline(x, dcal, W, S, bins if K is None else None, wsp=workspace)
        cells = None if own_rows is None else (own_rows[0] * nx, own_rows[1] * nx)
        h = self.hobday_approx(a["out"], dcal, bins, q, wd, ws, ny, nx, rows=own_rows, cells=cells, wsp=workspace,
                               binsb=a.get("bins"), tails=a.get("tails"))
        res = {
            "dat_anomaly": a["out"],
            "mask": a["mask"],
            "invalid_count": a["invalid_count"],
            "thr_doy_major": h["thr_doy_major"],
            "stats_dev": h["stats_dev"],
            "extreme_events": h["extreme"],
            "n_true": h["n_true"],
            "path": h["path"],
            "_keep": (a["_keep"], h["_keep"]),
        }
        if transpose_thresholds:
            res["thresholds"] = self.transpose(h["thr_doy_major"], wsp=workspace, name="thresholds")
        return res

    # ------------------------------------------------------------------ stage a13 (fixed baseline)
    def fixed_baseline(
        self,
        x: torch.Tensor,
        dcal: DeviceCalendar,
        reference_period=None,
        bins: Optional[BinTable] = None,
        count_invalid: bool = True,
        wsp: Optional[dict] = None,
        sub: Optional[torch.Tensor] = None,
        second_stage: bool = False,
        tails_bins: Optional[BinTable] = None,
    ) -> Dict[str, torch.Tensor]:
        """``x - nanmean_doy(x)`` for all timesteps (detect.py:2299-2397); ``dcal`` must be an untrimmed calendar.
        ``sub`` ``[C]``: a per-cell value taken off ``x`` on load (the deferred residual mean of :meth:`detrend`).
        ``second_stage``: called on the output of :meth:`detrend` with a shared workspace -- its mask / count buffers get
        names of their own, so that the first stage's validation outputs (the RAW field's) survive.
        ``tails_bins``: also leave the sorted key lists of the output (``"tails"``, 32 rows per list: what
        :meth:`tail_extract` would make of it) when the register kernel takes the shape -- see :meth:`fused_tails_ok`."""
        T, Cn = x.shape
        cal = dcal.plan
        assert cal.T == T and cal.T_out == T, "fixed_baseline needs an untrimmed calendar"
        if sub is not None:
            assert sub.dtype == torch.float32 and sub.numel() == Cn
        use = self._reference_rows(cal, reference_period)
        out, mask, invalid = self._anomaly_buffers(wsp, "anom", T, Cn, second_stage)
        invalid.zero_()
        counts = invalid if count_invalid else None
        nd = cal.max_bucket
        res = {"out": out, "mask": mask, "invalid_count": invalid}
        if tails_bins is not None and bins is None and self.fused_tails_ok(dcal, tails_bins):
            edges = self.bin_tables(tails_bins)[0]
            tl = res["tails"] = self._tail_buffers(nd, self.LIST_ROWS_EXTRACT, Cn, edges, wsp)
            self.call("marex_fixed_baseline_tails_f32", x, sub, nd, T, Cn, dcal.doy_start, dcal.doy_rows, use, edges,
                      tails_bins.nb, out, mask, counts, tl["tails"], tl["aux"])
        else:
            edges = binsb = None
            if bins is not None:
                edges = self.bin_tables(bins)[0]
                binsb = res["bins"] = self._buf(wsp, "bins", self.bins_shape(T, Cn), torch.int16, self.device)
            self.call("marex_fixed_baseline_sub_f32", x, sub, nd, T, Cn, dcal.doy_start, dcal.doy_rows, use, edges,
                      bins.nb if bins is not None else 0, out, binsb, mask, counts)
        if use is not None:
            self.sync()  # the small table must outlive the kernel
        return res

    # ------------------------------------------------------------------ stage a10 binning on its own
    def digitize(self, anom: torch.Tensor, dcal: DeviceCalendar, bins: BinTable, wsp: Optional[dict] = None) -> torch.Tensor:
        """Dayofyear-sorted bin matrix of an anomaly field (rows with ``rowb_index < 0`` are skipped)."""
        T, Cn = anom.shape
        edges = self.bin_tables(bins)[0]
        binsb = self._buf(wsp, "bins", self.bins_shape(dcal.plan.T_out, Cn), torch.int16, self.device)
        self.call("marex_digitize_f32", anom, T, Cn, dcal.rowb_index, edges, bins.nb, dcal.plan.T_out, binsb)
        return binsb

    # ------------------------------------------------------------------ stage a12 (detrend)
    def detrend(
        self,
        x: torch.Tensor,
        model: np.ndarray,
        pmodel: np.ndarray,
        force_zero_mean: bool,
        bins_and_cal=None,
        count_invalid: bool = True,
        wsp: Optional[dict] = None,
        defer_mean: bool = False,
    ) -> Dict[str, torch.Tensor]:
        """Residual of the least-squares fit of ``model`` (detect.py:2143-2224); optional binning of the result.
        ``defer_mean`` (with ``force_zero_mean``): ``out`` keeps its mean and ``res["mean"]`` ``[C]`` is the value still to be
        subtracted -- :meth:`fixed_baseline` takes it as ``sub`` and saves a pass over the field."""
        T, Cn = x.shape
        n_coef = int(model.shape[0])
        pm = self._dev(np.ascontiguousarray(pmodel, dtype=np.float64))
        mt = self._dev(np.ascontiguousarray(model.T, dtype=np.float64))
        out, mask, invalid = self._anomaly_buffers(wsp, "detrended", T, Cn)
        mean = None
        if defer_mean and force_zero_mean:
            mean = self._buf(wsp, "detrend_mean", (Cn,), torch.float32, self.device)
            self.call("marex_detrend_deferred_mean_f32", x, T, Cn, pm, mt, n_coef, out, mean, mask, invalid)
        else:
            self.call("marex_detrend_f32", x, T, Cn, pm, mt, n_coef, int(bool(force_zero_mean)), out, mask, invalid)
        self.sync()  # pm / mt must outlive the kernel
        res = {"out": out, "mask": mask, "invalid_count": invalid}
        if mean is not None:
            res["mean"] = mean
        if bins_and_cal is not None and bins_and_cal[0] is not None:
            res["bins"] = self.digitize(out, bins_and_cal[1], bins_and_cal[0], wsp=wsp)
        return res

    def detrend_fixed_baseline(self, x: torch.Tensor, model: np.ndarray, pmodel: np.ndarray, force_zero_mean: bool,
                               dcal: DeviceCalendar, reference_period=None, wsp: Optional[dict] = None,
                               tails_bins: Optional[BinTable] = None) -> Dict[str, torch.Tensor]:
        """``detrend_fixed_baseline`` (detect.py:2400-2462): residual of the fit minus its daily climatology.  One chain on the
        device when the model has at most 5 terms and dayofyear buckets at most 128 rows (the residual field is never
        materialised: 3 reads and 1 write of the field), otherwise the two stages one after the other.  Same bits either way."""
        T, Cn = x.shape
        cal = dcal.plan
        n_coef = int(model.shape[0])
        nd = cal.max_bucket
        if n_coef > 5 or nd > 128 or not self.ctx_opt("DETREND_FUSED", 1):
            d = self.detrend(x, model, pmodel, bool(force_zero_mean), None, count_invalid=True, wsp=wsp, defer_mean=True)
            r = self.fixed_baseline(d["out"], dcal, reference_period, None, count_invalid=False, wsp=wsp, sub=d.get("mean"),
                                    second_stage=True, tails_bins=tails_bins)
            res = {"out": r["out"], "mask": d["mask"], "invalid_count": d["invalid_count"]}
            if "tails" in r:
                res["tails"] = r["tails"]
            return res
        assert x.dtype == torch.float32 and cal.T == T and cal.T_out == T
        pm = self._dev(np.ascontiguousarray(pmodel, dtype=np.float64))
        mt_host = np.ascontiguousarray(model.T, dtype=np.float64)
        mt = self._dev(mt_host)
        mts = self._dev(np.ascontiguousarray(mt_host[cal.doy_rows]))  # model rows in dayofyear-sorted row order
        use = self._reference_rows(cal, reference_period)
        out, mask, invalid = self._anomaly_buffers(wsp, "anom", T, Cn)
        res = {"out": out, "mask": mask, "invalid_count": invalid}
        fit = (x, T, Cn, pm, mt, mts, n_coef, int(bool(force_zero_mean)), dcal.doy_start, dcal.doy_rows, use, nd)
        if tails_bins is not None and self.fused_tails_ok(dcal, tails_bins):
            edges = self.bin_tables(tails_bins)[0]
            tl = res["tails"] = self._tail_buffers(nd, self.LIST_ROWS_EXTRACT, Cn, edges, wsp)
            self.call("marex_detrend_fixed_baseline_tails_f32", *fit, edges, tails_bins.nb, out, mask, invalid,
                      tl["tails"], tl["aux"])
        else:
            self.call("marex_detrend_fixed_baseline_f32", *fit, out, mask, invalid)
        self.sync()  # pm / mt / use must outlive the kernels
        return res

    # ------------------------------------------------------------------ stage a9 exact Hobday
    def std_normalise(self, anom: torch.Tensor, dcal: DeviceCalendar, window: int = 30,
                      wsp: Optional[dict] = None) -> Dict[str, torch.Tensor]:
        """``dat_stn`` and ``STD`` of the std_normalise branch (detect.py:2257-2278): day-of-year standard deviation,
        wrapped ``window``-day rolling RMS of it, anomaly / STD.  ``STD`` is returned dayofyear-major ``[366, C]``."""
        T, Cn = anom.shape
        std_day = self._buf(wsp, "std_day", (N_DOY, Cn), torch.float32, self.device)
        std_roll = self._buf(wsp, "std_roll", (N_DOY, Cn), torch.float32, self.device)
        out = self._buf(wsp, "dat_stn", (T, Cn), torch.float32, self.device)
        self.call("marex_std_rolling_doy_f32", anom, T, Cn, dcal.doy_start, dcal.doy_rows, int(window), std_day, std_roll)
        self.call("marex_div_doy_f32", anom, std_roll, dcal.doy_start, dcal.doy_rows, T, Cn, out)
        return {"dat_stn": out, "STD": std_roll}

    # ------------------------------------------------------------------ tracker pre-processing
    def fill_holes(self, data_bin: torch.Tensor, mask: torch.Tensor, ny: int, nx: int, R_fill: int,
                   regional_mode: bool = False, wsp: Optional[dict] = None, name: str = "filled") -> torch.Tensor:
        """Binary closing + opening with a disk of radius ``R_fill`` per timestep, land masked (track.py:1520-1676).
        ``data_bin``: uint8 ``[T, ny*nx]`` (0/1), ``mask``: uint8 ``[ny*nx]``."""
        T, Cn = data_bin.shape
        assert Cn == ny * nx
        out = self._buf(wsp, name, (T, Cn), torch.uint8, self.device)
        self.call("marex_fill_holes_u8", data_bin, mask, T, int(ny), int(nx), int(R_fill), int(bool(regional_mode)), out)
        return out

    def time_closing(self, x: torch.Tensor, T_fill: int, wsp: Optional[dict] = None) -> torch.Tensor:
        """Binary closing of uint8 ``[T, C]`` along time over ``T_fill + 1`` steps (first half of track.py:1678-1726), grid or mesh alike."""
        T, Cn = x.shape
        out = self._buf(wsp, "time_closed", (T, Cn), torch.uint8, self.device)
        self.call("marex_time_closing_u8", x, T, Cn, int(T_fill), out)
        return out

    def fill_time_gaps(self, data_bin: torch.Tensor, mask: torch.Tensor, ny: int, nx: int, R_fill: int, T_fill: int,
                       regional_mode: bool = False, wsp: Optional[dict] = None) -> torch.Tensor:
        """Temporal closing over ``T_fill + 1`` steps, then ``fill_holes(R_fill // 2)`` (track.py:1678-1726)."""
        if T_fill == 0:
            return data_bin
        tmp = self.time_closing(data_bin, T_fill, wsp=wsp)
        return self.fill_holes(tmp, mask, ny, nx, int(R_fill) // 2, regional_mode, wsp=wsp, name="gap_filled")

    def label_objects_2d(self, data_bin: torch.Tensor, ny: int, nx: int, wrap_x: bool = True,
                         wsp: Optional[dict] = None) -> Dict[str, torch.Tensor]:
        """Per-timestep 8-connected components (track.py:2013-2031): ``labels`` int32 ``[T, C]`` (1 + smallest linear
        index of the component, 0 = background) and ``areas`` int32 ``[T, C]`` (cell count, stored at the root cell)."""
        T, Cn = data_bin.shape
        labels = self._buf(wsp, "labels", (T, Cn), torch.int32, self.device)
        areas = self._buf(wsp, "areas", (T, Cn), torch.int32, self.device)
        self.call("marex_label2d_i32", data_bin, T, int(ny), int(nx), int(bool(wrap_x)), labels, areas)
        return {"labels": labels, "areas": areas}

    def label_objects_3d(self, data_bin: torch.Tensor, ny: int, nx: int, wrap_x: bool = True, connect_t: bool = True,
                         wsp: Optional[dict] = None, max_block_cells: Optional[int] = None) -> Dict[str, torch.Tensor]:
        """26-connected components in (time, y, x) (track.py:2006-2048, ``time_connectivity=True``; ``connect_t=False``:
        one labelling per timestep).  ``ids`` int32 ``[T, C]``: IDs 1..N numbered by the component's first cell in C order,
        0 = background; ``areas`` int32 (cells of ID ``k`` at ``k - 1``, the first N entries); ``n`` int32 ``[1]`` = N.

        A field of more than 2^31 - 2 cells, or any field when ``max_block_cells`` is given, is labelled in time blocks
        of at most that many cells (:func:`plan_time_blocks`) and stitched across the seams: the same ``ids`` and ``n``
        as one call would give, ``areas`` int64 ``[N]`` (one event may exceed 2^31 cells there).  Refused with
        :class:`TrackingError`: a single slice of 2^31 - 1 cells or more, more than 2^31 - 2 objects before stitching."""
        T, Cn = data_bin.shape
        assert Cn == ny * nx
        if max_block_cells is not None or T * Cn > LABEL_BLOCK_CELLS:
            return self._label_objects_3d_blocked(data_bin, ny, nx, wrap_x, connect_t, wsp, max_block_cells)
        ids = self._buf(wsp, "ids3d", (T, Cn), torch.int32, self.device)
        areas = self._buf(wsp, "areas3d", (T * Cn,), torch.int32, self.device)
        n = self._buf(wsp, "n3d", (1,), torch.int32, self.device)
        self.call("marex_label3d_i32", data_bin, T, int(ny), int(nx), int(bool(wrap_x)), int(bool(connect_t)), ids, areas, n)
        return {"ids": ids, "areas": areas, "n": n}

    def _label_objects_3d_blocked(self, data_bin: torch.Tensor, ny: int, nx: int, wrap_x: bool, connect_t: bool,
                                  wsp: Optional[dict], max_block_cells: Optional[int]) -> Dict[str, torch.Tensor]:
        """:meth:`label_objects_3d` in time blocks: label every block into its slice of ``ids``,
        stitch the seams in a parent table over the provisional IDs, rank its roots, map every block through the table.
        The scratch (the blocks' int32 areas here, the rank array inside the library) has the size of the largest
        block; one host read of ``n_k`` per block sizes the table."""
        T, Cn = data_bin.shape
        blocks = plan_time_blocks(T, Cn, max_block_cells)
        ids = self._buf(wsp, "ids3d", (T, Cn), torch.int32, self.device)
        areas_blk = self._buf(wsp, "areas3d_block", (max(b - a for a, b in blocks) * Cn,), torch.int32, self.device)
        n = self._buf(wsp, "n3d", (1,), torch.int32, self.device)
        wrap, ct = int(bool(wrap_x)), int(bool(connect_t))
        offs, counts, parts = [], [], []
        n_prov = 0
        for t0, t1 in blocks:
            self.call("marex_label3d_i32", data_bin[t0:t1], t1 - t0, int(ny), int(nx), wrap, ct, ids[t0:t1], areas_blk, n)
            nk = int(n.item())
            offs.append(n_prov)
            counts.append(nk)
            parts.append(areas_blk[:nk].clone())  # the next block overwrites areas_blk
            n_prov += nk
            if n_prov > LABEL_BLOCK_CELLS:
                raise TrackingError(f"more than 2^31 - 2 provisional objects ({n_prov} after the block of steps {t0}..{t1 - 1})",
                                    details="block labels are int32; smaller blocks do not help, the field has too many objects")
        if n_prov == 0:  # nothing set anywhere: ids is all background already
            return {"ids": ids, "areas": torch.zeros((0,), dtype=torch.int64, device=self.device), "n": n}
        table = torch.arange(n_prov + 1, dtype=torch.int32, device=self.device)
        if ct:
            for k in range(len(blocks) - 1):
                if counts[k] and counts[k + 1]:  # an empty block has no ID to join
                    seam = blocks[k][1]
                    self.call("marex_label_seam_union_i32", ids[seam - 1], ids[seam], int(ny), int(nx), wrap, offs[k], counts[k],
                              offs[k + 1], counts[k + 1], table, n_prov + 1)
        areas = self._buf(wsp, "areas3d_i64", (n_prov,), torch.int64, self.device)
        self.call("marex_label_table_resolve_i32", table, n_prov, torch.cat(parts), areas, n)
        # block 0 goes through the table too: two of its events joined only through block 1 collapse into the smaller ID
        for (t0, t1), off, nk in zip(blocks, offs, counts):
            if nk:
                self.call("marex_label_apply_table_i32", ids[t0:t1], (t1 - t0) * Cn, table, n_prov + 1, off)
        return {"ids": ids, "areas": areas[:int(n.item())], "n": n}

    # ------------------------------------------------------------------ object properties and overlaps (track.py:2109-2504)
    def ids_minmax(self, ids: torch.Tensor) -> tuple:
        """``(min, max)`` of an int32 ID field (synchronises)."""
        mm = self._buf(None, "ids_minmax", (2,), torch.int32, self.device)
        self.call("marex_ids_minmax_i32", ids, ids.numel(), mm)
        lo, hi = (int(v) for v in mm.cpu().numpy())
        if lo < 0:
            raise create_data_validation_error("Object IDs must be non-negative", details=f"smallest ID {lo}; 0 is background",
                                               data_info={"min_id": lo, "max_id": hi})
        return lo, hi

    def _check_fits(self, nbytes: int, what: str, details: str) -> None:
        """Raise instead of allocating past the free device memory (buffers are sized up front, never truncated)."""
        free, _ = torch.cuda.mem_get_info(self.device)
        if nbytes > free:
            raise ProcessingError(f"{what}: needs {nbytes / 1e9:.3f} GB of device memory, {free / 1e9:.3f} GB are free",
                                  details=details)

    def _ids_check(self, ids: torch.Tensor) -> tuple:
        if ids.dtype != torch.int32 or ids.dim() != 2 or not ids.is_contiguous() or ids.device != self.device:
            raise ProcessingError("object IDs must be a contiguous int32 [T, C] tensor on the engine's device",
                                  details=f"got {ids.dtype} {tuple(ids.shape)} on {ids.device}")
        return tuple(int(k) for k in ids.shape)

    def _object_spans(self, ids: torch.Tensor, T: int, Cn: int, hi: int, what: str, details: str):
        """Per ID 0..hi of ``ids`` on the device: ``tmin`` / ``tmax`` int32 (first / last timestep, INT_MAX / -1 when
        absent), ``off`` int64 (first (timestep, ID) slot of the ID when every ID gets one per step of its span) and
        ``total`` int64 ``[1]`` (all slots).  ``what`` / ``details`` word the error when the tables do not fit."""
        nid = hi + 1
        ntiles = (nid + 4095) // 4096
        self._check_fits(16 * nid + 16 * ntiles, what, details)
        tmin = self._buf(None, "obj_tmin", (nid,), torch.int32, self.device)
        tmax = self._buf(None, "obj_tmax", (nid,), torch.int32, self.device)
        off = self._buf(None, "obj_off", (nid,), torch.int64, self.device)
        work = self._buf(None, "obj_work", (2 * ntiles,), torch.int64, self.device)
        total = self._buf(None, "obj_total", (1,), torch.int64, self.device)
        self.call("marex_object_spans_i32", ids, T, Cn, hi, tmin, tmax, off, work, total)
        return tmin, tmax, off, total

    def object_moments(self, ids: torch.Tensor, ny: int, nx: int, wrap: bool = True) -> Dict[str, np.ndarray]:
        """Area and centroid of every ID in every timestep of ``ids`` int32 ``[T, ny * nx]`` (values <= 0: background):
        ``t``, ``id`` (int64), ``area`` (float64 cells) and ``centroid`` (float64 ``[2, n]``: mean row, mean column), rows in
        (t, id) order.  With ``wrap`` the column mean of an object with cells in both the first and the last 100 columns
        is taken with the columns x > nx // 2 shifted by -nx, and nx is added when that mean is negative
        (calculate_centroid, track.py:2050-2107).  The device accumulates integer sums; the division is NumPy's float64."""
        T, Cn = self._ids_check(ids)
        if Cn != ny * nx:
            raise ProcessingError(f"object_moments: {Cn} cells per slice, ny * nx = {ny * nx}")
        _, hi = self.ids_minmax(ids)
        out = {"t": np.zeros(0, np.int64), "id": np.zeros(0, np.int64), "area": np.zeros(0, np.float64),
               "centroid": np.zeros((2, 0), np.float64)}
        if hi <= 0:
            return out
        tmin, _, off, total = self._object_spans(
            ids, T, Cn, hi, "object properties",
            f"per-ID first / last timestep and slot offsets for IDs 0..{hi}; renumber sparse IDs densely")
        n_slots = int(total.item())
        self._check_fits(88 * n_slots, "object properties",
                         f"{n_slots} (timestep, ID) slots between each ID's first and last timestep, 88 bytes each")
        acc = self._buf(None, "obj_acc", (n_slots, 5), torch.int64, self.device)
        self.call("marex_object_moments_i32", ids, T, int(ny), int(nx), tmin, off, n_slots, acc)
        n_out = self._buf(None, "obj_n", (1,), torch.int64, self.device)
        tid = self._buf(None, "obj_tid", (n_slots, 2), torch.int32, self.device)
        mom = self._buf(None, "obj_mom", (n_slots, 5), torch.int64, self.device)
        self.call("marex_object_compact", n_slots, hi, tmin, off, acc, n_out, tid, mom)
        n = int(n_out.item())
        if not 0 < n <= n_slots:
            raise ProcessingError(f"object_moments: {n} non-empty slots of {n_slots} (internal sizing error)")
        tid_h = tid[:n].cpu().numpy().astype(np.int64)
        mom_h = mom[:n].cpu().numpy()
        order = np.argsort((tid_h[:, 0] << 32) | tid_h[:, 1])  # (t, id) order: the device compacts in no particular order
        tid_h, mom_h = tid_h[order], mom_h[order]
        cnt, sy, sx, nr, fl = (mom_h[:, k] for k in range(5))
        c1 = sx / cnt
        if wrap:
            seam = fl == 3
            c = (sx[seam] - int(nx) * nr[seam]) / cnt[seam]
            c1[seam] = np.where(c < 0, c + nx, c)
        out.update(t=tid_h[:, 0], id=tid_h[:, 1], area=cnt.astype(np.float64), centroid=np.stack([sy / cnt, c1]))
        return out

    def overlap_pairs(self, ids: torch.Tensor) -> np.ndarray:
        """``(n, 3)`` int32 ``[id at t, id at t + 1, cells]`` over every t < T - 1 of ``ids`` int32 ``[T, C]``, summed over
        time and sorted lexicographically (check_overlap_slice / find_overlapping_objects, track.py:2396-2504)."""
        T, Cn = self._ids_check(ids)
        _, hi = self.ids_minmax(ids)
        empty = np.zeros((0, 3), np.int32)
        if T < 2 or hi <= 0:
            return empty
        stats = self._buf(None, "ovl_stats", (4,), torch.int64, self.device)
        self.call("marex_overlap_count_i32", ids, T, Cn, stats)
        runs = int(stats[1].item())
        if runs == 0:
            return empty
        cap = pair_table_cap(runs)
        self._check_fits(16 * cap + 16 * runs, "overlap pairs", f"a hash table of {cap} entries for {runs} runs of equal pairs")
        keys = self._buf(None, "ovl_keys", (cap,), torch.int64, self.device)
        counts = self._buf(None, "ovl_counts", (cap,), torch.int64, self.device)
        out_k = self._buf(None, "ovl_out_keys", (runs,), torch.int64, self.device)
        out_c = self._buf(None, "ovl_out_counts", (runs,), torch.int64, self.device)
        self.call("marex_overlap_pairs_i32", ids, T, Cn, cap, keys, counts, stats, runs, out_k, out_c)
        s = stats.cpu().numpy()
        n = int(s[3])
        if s[2] != 0 or not 0 < n <= runs:
            raise ProcessingError(f"overlap pairs: hash table overflow ({n} pairs, {runs} runs, {cap} entries)")
        k = out_k[:n].cpu().numpy()
        c = out_c[:n].cpu().numpy()
        order = np.argsort(k, kind="stable")
        k, c = k[order], c[order]
        if c.max() > np.iinfo(np.int32).max:
            raise ProcessingError("overlap pairs: a pair overlaps in 2^31 or more cells, which int32 cannot hold",
                                  details=f"largest overlap {int(c.max())} cells")
        return np.stack([k >> 32, k & 0xFFFFFFFF, c], axis=1).astype(np.int32)

    # ------------------------------------------------------------------ the same stages on a mesh (track.py:1947-2005, 2135-2323, 2431-2439)
    def _mesh_weights_check(self, q: torch.Tensor, Cn: int, what: str) -> None:
        if q.dtype != torch.int64 or tuple(q.shape) != (4, Cn) or not q.is_contiguous() or q.device != self.device:
            raise ProcessingError(f"{what}: the weight table must be a contiguous int64 [4, {Cn}] tensor on the engine's device",
                                  details=f"got {q.dtype} {tuple(q.shape)} on {q.device}")

    def label_objects_mesh(self, x: torch.Tensor, mask: torch.Tensor, nbr: torch.Tensor,
                           max_block_cells: Optional[int] = None) -> Dict[str, torch.Tensor]:
        """Connected components per timestep over the mesh edges, land excluded (track.py:1947-2005): ``ids`` int32
        ``[T, C]`` restarting at 1 in every timestep, numbered by each component's smallest cell index (scipy's
        ``connected_components`` order), 0 = background, and ``n_t`` int32 ``[T]``, the objects of every timestep.
        ``x`` uint8 ``[T, C]``, ``mask`` uint8 ``[C]``, ``nbr`` int32 ``[3, C]`` 0-based, -1 = none.  Timesteps are
        independent, so a field of 2^31 - 1 cells and more (or any field when ``max_block_cells`` is given) is labelled in
        time blocks (:func:`plan_time_blocks`) with no seam work."""
        T, Cn = (int(k) for k in x.shape)
        blocks = plan_time_blocks(T, Cn, max_block_cells)
        blk = max(b - a for a, b in blocks) * Cn
        self._check_fits(4 * T * Cn + 4 * T + 8 * blk, "mesh labelling",
                         f"int32 IDs of {T} x {Cn} cells, the int32 sizes and the union-find scratch of a block of {blk} cells")
        ids = self._buf(None, "ids_mesh", (T, Cn), torch.int32, self.device)
        n_t = self._buf(None, "n_t_mesh", (T,), torch.int32, self.device)
        work = self._buf(None, "areas_mesh_block", (blk,), torch.int32, self.device)
        for t0, t1 in blocks:
            self.call("marex_label_mesh_i32", x[t0:t1], mask, nbr, t1 - t0, Cn, ids[t0:t1], work)
            self.call("marex_label_mesh_rank_i32", ids[t0:t1], t1 - t0, Cn, work, ids[t0:t1], n_t[t0:t1])
        return {"ids": ids, "n_t": n_t}

    def unique_ids_in_time(self, ids: torch.Tensor) -> torch.Tensor:
        """``ids + (exclusive cumulative sum over time of the per-timestep maximum)`` where ``ids > 0`` (track.py:2762-2764):
        a new int32 ``[T, C]`` tensor.  :class:`TrackingError` when the largest new ID would exceed 2^31 - 2."""
        T, Cn = self._ids_check(ids)
        self._check_fits(4 * T * Cn + 8 * T, "unique IDs in time", f"an int32 copy of {T} x {Cn} IDs")
        rowmax = self._buf(None, "ids_rowmax", (T,), torch.int32, self.device)
        self.call("marex_ids_row_max_i32", ids, T, Cn, rowmax)
        csum = torch.cumsum(rowmax.to(torch.int64), 0)
        total = int(csum[-1].item())
        if total > LABEL_BLOCK_CELLS:
            raise TrackingError(f"more than 2^31 - 2 objects ({total}): unique IDs do not fit int32")
        off = (csum - rowmax).to(torch.int32)
        out = self._buf(None, "ids_unique", (T, Cn), torch.int32, self.device)
        self.call("marex_ids_add_row_offset_i32", ids, T, Cn, off, out)
        return out

    def mesh_object_moments(self, ids: torch.Tensor, q: torch.Tensor, e: int) -> Dict[str, np.ndarray]:
        """Area and centroid on the sphere of every ID in every timestep of ``ids`` int32 ``[T, C]`` (values <= 0:
        background), weighted by the fixed-point table ``q`` int64 ``[4, C]`` with exponent ``e``
        (:func:`marex_amd.track.mesh_weight_tables`): ``t``, ``id``, ``cells`` (int64), ``area`` (float32) and ``centroid``
        (float32 ``[2, n]``: latitude, longitude in degrees), rows in (t, id) order.  The device adds integers; the host
        divides in float64: ``area = float32(S0 / 2^e)``, the centroid is the direction of ``(S1, S2, S3)``."""
        T, Cn = self._ids_check(ids)
        self._mesh_weights_check(q, Cn, "mesh_object_moments")
        _, hi = self.ids_minmax(ids)
        out = {"t": np.zeros(0, np.int64), "id": np.zeros(0, np.int64), "cells": np.zeros(0, np.int64),
               "area": np.zeros(0, np.float32), "centroid": np.zeros((2, 0), np.float32)}
        if hi <= 0:
            return out
        tmin, _, off, total = self._object_spans(
            ids, T, Cn, hi, "mesh object properties",
            f"per-ID first / last timestep and slot offsets for IDs 0..{hi}; renumber sparse IDs densely")
        n_slots = int(total.item())
        self._check_fits(88 * n_slots, "mesh object properties",
                         f"{n_slots} (timestep, ID) slots between each ID's first and last timestep, 88 bytes each")
        acc = self._buf(None, "mobj_acc", (n_slots, 5), torch.int64, self.device)
        self.call("marex_mesh_object_moments_i64", ids, T, Cn, q, tmin, off, n_slots, acc)
        n_out = self._buf(None, "mobj_n", (1,), torch.int64, self.device)
        tid = self._buf(None, "mobj_tid", (n_slots, 2), torch.int32, self.device)
        mom = self._buf(None, "mobj_mom", (n_slots, 5), torch.int64, self.device)
        self.call("marex_object_compact", n_slots, hi, tmin, off, acc, n_out, tid, mom)
        n = int(n_out.item())
        if not 0 < n <= n_slots:
            raise ProcessingError(f"mesh_object_moments: {n} non-empty slots of {n_slots} (internal sizing error)")
        tid_h = tid[:n].cpu().numpy().astype(np.int64)
        mom_h = mom[:n].cpu().numpy()
        order = np.argsort((tid_h[:, 0] << 32) | tid_h[:, 1])  # (t, id) order: the device compacts in no particular order
        tid_h, mom_h = tid_h[order], mom_h[order]
        area, centroid = mesh_moments_finish(mom_h, e)
        out.update(t=tid_h[:, 0], id=tid_h[:, 1], cells=mom_h[:, 0].copy(), area=area, centroid=centroid)
        return out

    def mesh_event_rename(self, ids: torch.Tensor, lut, n_ev: int, q: torch.Tensor, e: int) -> Dict[str, np.ndarray]:
        """The device pass of cluster_rename_objects_and_props on a mesh (track.py:2908-2989, 3161-3210), in one kernel and
        in place: ``ids`` int32 ``[T, C]`` -> ``lut[id]`` for ``0 < id < len(lut)``, else 0 (``lut``: int32 event numbers
        0..n_ev); per (timestep, event) ``mom`` int64 ``[T, n_ev, 5]`` (cells and the sums of ``q[0..3]`` over the event's
        cells) and ``gid`` int32 ``[T, n_ev]`` (the largest original ID under the slot, 0 when the event is absent).
        ``q``, ``e``: the weight table and its exponent, as in every mesh call; the device adds integers and does not need
        ``e`` -- :func:`marex_amd.track_mesh.mesh_moments_finish` does, to turn ``mom`` into areas and centroids."""
        T, Cn = self._ids_check(ids)
        self._mesh_weights_check(q, Cn, "mesh_event_rename")
        n_ev, e = int(n_ev), int(e)
        lut_h = np.asarray(lut)
        if lut_h.dtype != np.int32 or lut_h.ndim != 1 or lut_h.size == 0:
            raise ProcessingError("mesh_event_rename: the table must be a non-empty int32 vector",
                                  details=f"got {lut_h.dtype} {lut_h.shape}")
        if n_ev <= 0 or int(lut_h.max()) > n_ev:
            raise ProcessingError("mesh_event_rename: the table must map to events 0..n_ev, n_ev > 0",
                                  details=f"largest entry {int(lut_h.max())}, n_ev={n_ev}")
        slots = T * n_ev
        self._check_fits(44 * slots + 4 * lut_h.size, "mesh event properties",
                         f"{T} x {n_ev} dense (timestep, event) slots of 44 bytes and a table of {lut_h.size} IDs")
        acc = self._buf(None, "mev_acc", (slots, 5), torch.int64, self.device)
        gid = self._buf(None, "mev_gid", (slots,), torch.int32, self.device)
        self.call("marex_mesh_event_rename_i64", ids, T, Cn, self._dev(lut_h), lut_h.size, n_ev, q, acc, gid)
        return {"mom": acc.cpu().numpy().reshape(T, n_ev, 5), "gid": gid.cpu().numpy().reshape(T, n_ev)}

    def mesh_overlap_pairs(self, ids: torch.Tensor, q: torch.Tensor, e: int) -> np.ndarray:
        """``(n, 3)`` float32 ``[id at t, id at t + 1, overlap area]`` over every t < T - 1 of ``ids`` int32 ``[T, C]``: the area
        of the cells a pair shares, summed over time as an integer of ``q[0]`` and returned as ``float32(S / 2^e)``, rows
        sorted lexicographically (check_overlap_slice / find_overlapping_objects on a mesh, track.py:2396-2504); ``S`` is exact
        even where a pair met in many timesteps adds up to more than 64 bits.  The IDs
        travel in float32 columns as the reference's do: :class:`TrackingError` for an ID of 2^24 or above."""
        T, Cn = self._ids_check(ids)
        self._mesh_weights_check(q, Cn, "mesh_overlap_pairs")
        _, hi = self.ids_minmax(ids)
        if hi >= 1 << 24:
            raise TrackingError(f"object IDs of 2^24 and above ({hi}) do not survive the float32 columns of the overlap list",
                                details="the reference stores [id, id, area] in one float32 array (track.py:2450)",
                                suggestions=["Renumber the IDs densely"])
        empty = np.zeros((0, 3), np.float32)
        if T < 2 or hi <= 0:
            return empty
        stats = self._buf(None, "ovl_stats", (4,), torch.int64, self.device)
        self.call("marex_overlap_count_i32", ids, T, Cn, stats)
        runs = int(stats[1].item())
        if runs == 0:
            return empty
        cap = pair_table_cap(runs)
        self._check_fits(24 * cap + 24 * runs, "mesh overlap pairs", f"a hash table of {cap} entries for {runs} runs of equal pairs")
        keys = self._buf(None, "movl_keys", (cap,), torch.int64, self.device)
        sums = self._buf(None, "movl_sums", (cap, 2), torch.int64, self.device)
        out_k = self._buf(None, "movl_out_keys", (runs,), torch.int64, self.device)
        out_s = self._buf(None, "movl_out_sums", (runs, 2), torch.int64, self.device)
        self.call("marex_mesh_overlap_pairs_i64", ids, T, Cn, q[0], cap, keys, sums, stats, runs, out_k, out_s)
        s = stats.cpu().numpy()
        n = int(s[3])
        if s[2] != 0 or not 0 < n <= runs:
            raise ProcessingError(f"mesh overlap pairs: hash table overflow ({n} pairs, {runs} runs, {cap} entries)")
        k = out_k[:n].cpu().numpy()
        a = out_s[:n].cpu().numpy().view(np.uint64)
        order = np.argsort(k, kind="stable")
        k, a = k[order], a[order]
        # the pair's sum S = a[:, 1] * 2^32 + a[:, 0] as a correctly rounded float64: through int64 below 2^63, else exactly
        # in Python integers (a pair that persists over many timesteps; few rows)
        hi, lo = a[:, 1] + (a[:, 0] >> np.uint64(32)), a[:, 0] & np.uint64(0xFFFFFFFF)
        small = hi < np.uint64(1 << 31)
        S = np.empty(n, np.float64)
        S[small] = ((hi[small] << np.uint64(32)) | lo[small]).astype(np.int64).astype(np.float64)
        for j in np.nonzero(~small)[0]:
            S[j] = float((int(hi[j]) << 32) + int(lo[j]))
        return np.stack([(k >> 32).astype(np.float32), (k & 0xFFFFFFFF).astype(np.float32),
                         np.ldexp(S, -int(e)).astype(np.float32)], axis=1)

    def mesh_area(self, x: torch.Tensor, q: torch.Tensor, e: int) -> np.ndarray:
        """float64 ``[T]``: the area of the cells set in every timestep of ``x`` uint8 ``[T, C]``, ``S / 2^e`` of the integer
        sum ``S`` of ``q[0]`` over them (compute_area on a mesh, track.py:1513-1514)."""
        if x.dtype != torch.uint8 or x.dim() != 2:
            raise ProcessingError("mesh_area: the field must be a uint8 [T, C] tensor", details=f"got {x.dtype} {tuple(x.shape)}")
        T, Cn = (int(k) for k in x.shape)
        self._mesh_weights_check(q, Cn, "mesh_area")
        self._check_fits(8 * T, "mesh area", f"one int64 sum per timestep, {T} timesteps")
        out = self._buf(None, "mesh_area", (T,), torch.int64, self.device)
        self.call("marex_mesh_area_i64", x, T, Cn, q[0], out)
        return np.ldexp(out.cpu().numpy().astype(np.float64), -int(e))

    # ------------------------------------------------------------------ merge tracker stages (track.py:2554-3802)
    def _i32(self, a) -> torch.Tensor:
        return self._dev(np.asarray(a, dtype=np.int32))

    def relabel(self, ids: torch.Tensor, vals: np.ndarray, keys: Optional[np.ndarray] = None) -> None:
        """In place: ``ids`` (contiguous int32 on the device) -> ``vals[j]`` where ``keys[j]`` equals the ID (``keys``
        strictly ascending, one value per key; IDs without an entry stay), or with ``keys=None`` -> ``vals[id]`` for
        ``0 < id < len(vals)``."""
        if ids.dtype != torch.int32 or not ids.is_contiguous() or ids.device != self.device:
            raise ProcessingError("relabel: ids must be a contiguous int32 tensor on the engine's device")
        vals = self._i32_table("relabel", "vals", vals)
        if keys is not None:
            keys = self._i32_table("relabel", "keys", keys)
            if keys.size != vals.size or np.any(np.diff(keys.astype(np.int64)) <= 0):
                raise ProcessingError("relabel: keys must ascend strictly and have one value each",
                                      details=f"{keys.size} keys, {vals.size} values")
        if ids.numel() == 0 or vals.size == 0:
            return
        self.call("marex_relabel_i32", ids, ids.numel(), self._i32(keys) if keys is not None else None, self._i32(vals),
                  int(vals.size))

    @staticmethod
    def _i32_table(what: str, name: str, a) -> np.ndarray:
        """A one-dimensional host table of integers that all fit int32 (a silent wrap would name another ID)."""
        a = np.asarray(a)
        if a.ndim != 1 or (a.size and a.dtype.kind not in "iu"):
            raise ProcessingError(f"{what}: {name} must be a one-dimensional table of integers",
                                  details=f"got {a.dtype} {a.shape}")
        a = a.astype(np.int64)
        if a.size and (a.min() < -2 ** 31 or a.max() > 2 ** 31 - 1):
            raise ProcessingError(f"{what}: {name} does not fit int32", details=f"range {a.min()} .. {a.max()}")
        return a.astype(np.int32)

    def _partition_check(self, what: str, slices, ny: int, nx: int, child_keys, off, lab, others) -> tuple:
        """The tables of a grid partition, refused before any library call when a kernel would read past a slice or a
        table, or search unsorted keys: ``slices`` are contiguous int32 ``ny * nx`` tensors on the device, ``child_keys``
        ascend strictly, ``off`` runs from 0 to ``len(lab)`` with at least one entry per child, and every table of
        ``others`` (name -> values) has one value per entry.  Returns ``(child_keys, off, lab)`` as int32 arrays."""
        ny, nx = int(ny), int(nx)
        for s in slices:
            if (not isinstance(s, torch.Tensor) or s.dtype != torch.int32 or not s.is_contiguous() or s.device != self.device
                    or ny <= 0 or nx <= 0 or s.numel() != ny * nx):
                got = f"{s.dtype} {tuple(s.shape)} on {s.device}" if isinstance(s, torch.Tensor) else type(s).__name__
                raise ProcessingError(f"{what}: a slice must be a contiguous int32 tensor of ny * nx = {ny} * {nx} cells on the "
                                      f"engine's device", details=f"got {got}")
        keys, off, lab = (self._i32_table(what, n, a) for n, a in (("child_keys", child_keys), ("off", off), ("lab", lab)))
        n_ent = lab.size
        if (keys.size == 0 or off.size != keys.size + 1 or np.any(np.diff(keys.astype(np.int64)) <= 0) or off[0] != 0
                or off[-1] != n_ent or np.any(np.diff(off) <= 0)):
            raise ProcessingError(f"{what}: child_keys must ascend strictly, off must run from 0 to len(lab) with at least one "
                                  f"entry per child", details=f"{keys.size} children, off {off.tolist()}, {n_ent} labels")
        for name, a in others.items():
            if np.ndim(a) != 1 or len(a) != n_ent:
                raise ProcessingError(f"{what}: {name} must have one value per entry of lab",
                                      details=f"{np.shape(a)} for {n_ent} labels")
        return keys, off, lab

    def partition_centroid(self, cur: torch.Tensor, ny: int, nx: int, child_keys, off, pcy, pcx, lab, wrap: bool) -> None:
        """In place on the slice ``cur`` (int32 ``ny * nx``): every cell of child ``child_keys[k]`` (strictly ascending)
        takes ``lab[j]`` of the nearest parent centroid ``(pcy[j], pcx[j])``, ``off[k] <= j < off[k + 1]`` (first
        minimum); ``off`` runs from 0 to ``len(lab)``."""
        pcy, pcx = np.array(pcy, np.float64), np.array(pcx, np.float64)
        keys, off, lab = self._partition_check("partition_centroid", (cur,), ny, nx, child_keys, off, lab,
                                               {"pcy": pcy, "pcx": pcx})
        self.call("marex_partition_centroid_i32", cur, int(ny), int(nx), self._i32(keys), int(keys.size), self._i32(off),
                  self._dev(pcy), self._dev(pcx), self._i32(lab), int(bool(wrap)))

    def partition_nn(self, cur: torch.Tensor, prev: torch.Tensor, ny: int, nx: int, child_keys, off, parents, pcy, pcx, lab,
                     maxd, wrap: bool) -> None:
        """In place on the slice ``cur``: every cell of child ``child_keys[k]`` takes ``lab[j]`` of the parent
        ``parents[j]`` (``off[k] <= j < off[k + 1]``) with the nearest cell in ``prev`` among its cells in the 3 x 3
        buckets of size ``max(2, maxd[j] // 4)`` around the child cell's bucket and within ``maxd[j]``
        (``1 <= maxd[j] <= INT32_MAX``), else of the nearest parent centroid (partition_nn_grid, track.py:4972-5113).
        The tables are checked as in :meth:`partition_centroid`."""
        pcy, pcx = np.array(pcy, np.float64), np.array(pcx, np.float64)
        parents, maxd = np.asarray(parents), np.asarray(maxd)
        child_keys, off, lab = self._partition_check("partition_nn", (cur, prev), ny, nx, child_keys, off, lab,
                                                     {"pcy": pcy, "pcx": pcx, "parents": parents, "maxd": maxd})
        parents = self._i32_table("partition_nn", "parents", parents)
        if maxd.dtype.kind not in "iu" or maxd.astype(np.int64).min() < 1 or maxd.astype(np.int64).max() > 2 ** 31 - 1:
            raise ProcessingError("partition_nn: maxd must be integers from 1 to INT32_MAX",
                                  details=f"got {maxd.dtype} {maxd.tolist()[:8]}")
        parents, maxd = parents.astype(np.int64), maxd.astype(np.int64)
        ny, nx = int(ny), int(nx)
        gs = np.maximum(2, maxd // 4)
        ngy, ngx = (ny + gs - 1) // gs, (nx + gs - 1) // gs
        nb = ngy * ngx
        base = np.concatenate([[0], np.cumsum(nb)[:-1]]).astype(np.int64)
        n_buckets = int(nb.sum())
        order = np.argsort(parents, kind="stable")
        par_keys, first = np.unique(parents[order], return_index=True)
        poff = np.append(first, len(parents)).astype(np.int32)
        t = {k: self._i32(v) for k, v in (("par", par_keys), ("poff", poff), ("pent", order), ("gs", gs), ("ngy", ngy),
                                           ("ngx", ngx), ("maxd", maxd), ("ck", child_keys), ("off", off), ("lab", lab))}
        base_d = self._dev(base)
        pcy_d, pcx_d = self._dev(pcy), self._dev(pcx)
        cnt = torch.empty(n_buckets, dtype=torch.int64, device=self.device)
        bstart = torch.empty(n_buckets + 1, dtype=torch.int64, device=self.device)
        self.call("marex_nn_bucket_count_i32", prev, int(ny), int(nx), t["par"], len(par_keys), t["poff"], t["pent"], t["gs"],
                  t["ngy"], t["ngx"], base_d, n_buckets, cnt, bstart)
        n_cells = int(bstart[n_buckets].item())
        if n_cells <= 0:
            raise ProcessingError("partition_nn: the parents have no cells in the previous slice")
        cells = torch.empty(n_cells, dtype=torch.int32, device=self.device)
        self.call("marex_partition_nn_i32", cur, prev, int(ny), int(nx), t["par"], len(par_keys), t["poff"], t["pent"], t["ck"],
                  int(child_keys.size), t["off"], pcy_d, pcx_d, t["lab"], t["gs"], t["ngy"], t["ngx"], t["maxd"], base_d, n_buckets,
                  bstart, cnt, cells, n_cells, int(bool(wrap)))

    # ------------------------------------------------------------------ the partitions of the merge stage on a mesh (track.py:5246-5419)
    def _mesh_partition_check(self, what: str, cur: torch.Tensor, u: torch.Tensor) -> int:
        if cur.dtype != torch.int32 or cur.dim() != 1 or not cur.is_contiguous() or cur.device != self.device:
            raise ProcessingError(f"{what}: the slice must be a contiguous int32 [C] tensor on the engine's device",
                                  details=f"got {cur.dtype} {tuple(cur.shape)} on {cur.device}")
        Cn = int(cur.numel())
        if u.dtype != torch.float64 or tuple(u.shape) != (3, Cn) or not u.is_contiguous() or u.device != self.device:
            raise ProcessingError(f"{what}: the cells' unit vectors must be a contiguous float64 [3, {Cn}] tensor on the engine's "
                                  f"device", details=f"got {u.dtype} {tuple(u.shape)} on {u.device}")
        return Cn

    def mesh_partition_centroid(self, cur: torch.Tensor, child_keys, off, parent_vectors, labels, u: torch.Tensor) -> None:
        """In place on the slice ``cur`` (int32 ``[C]``): every cell of child ``child_keys[k]`` (ascending) takes
        ``labels[j]`` of the parent entry ``off[k] <= j < off[k + 1]`` whose float64 unit vector ``parent_vectors[:, j]`` is
        nearest to the cell's, ``u[:, c]``: smallest ``((dx dx + dy dy) + dz dz)``, first minimum.  All children of a
        timestep go in one launch (their cells are disjoint, the new labels fresh)."""
        Cn = self._mesh_partition_check("mesh_partition_centroid", cur, u)
        keys, off = np.asarray(child_keys, np.int64), np.asarray(off, np.int64)
        pv = np.ascontiguousarray(np.asarray(parent_vectors, np.float64))
        n_ent = len(labels)
        if (keys.size == 0 or off.size != keys.size + 1 or np.any(np.diff(keys) <= 0) or off[0] != 0 or off[-1] != n_ent
                or np.any(np.diff(off) <= 0) or pv.shape != (3, n_ent)):
            raise ProcessingError("mesh_partition_centroid: child_keys must ascend, off must run from 0 to len(labels) with at "
                                  "least one entry per child, parent_vectors must be [3, len(labels)]",
                                  details=f"{keys.size} children, off {off.tolist()}, {n_ent} labels, vectors {pv.shape}")
        self._check_fits(4 * (2 * keys.size + 1 + n_ent) + 24 * n_ent, "mesh centroid partition",
                         f"the tables of {keys.size} children and {n_ent} parent entries")
        self.call("marex_mesh_partition_centroid_i32", cur, Cn, self._i32(keys), int(keys.size), self._i32(off), u, self._dev(pv),
                  n_ent, self._i32(labels))

    #: hops of the nearest-neighbour partition queued between two reads of its control block (the result does not depend on it)
    MESH_NN_HOPS_PER_READ = 8

    def mesh_partition_nn(self, cur: torch.Tensor, prev: torch.Tensor, nbr: torch.Tensor, child: int, parents, parent_vectors,
                          labels, max_hops: int, u: torch.Tensor, hops_per_read: Optional[int] = None) -> Dict[str, int]:
        """In place on the slice ``cur``: the cells of ``child`` are divided among ``parents`` (IDs in the slice ``prev``, at
        most 10) as partition_nn_unstructured_optimised does (track.py:5246-5353): the parents' cells seed frontiers that
        grow over the listed neighbours ``nbr`` (int32 ``[3, C]``, 0-based, negative = none) hop by hop -- per hop, parent
        ascending, direction 0, 1, 2, one launch each -- until no child cell is unclaimed, a hop claims no child cell or
        ``max_hops`` hops have run; child cells still unclaimed take the nearest of ``parent_vectors`` (float64 ``[3, k]``) as
        in :meth:`mesh_partition_centroid`.  A cell owned by parent ``j`` gets ``labels[j]``.  The stopping rule lives in a
        control block on the device; the host reads it every ``hops_per_read`` hops.  Returns ``hops`` (run), ``leftover``
        (cells resolved by the centroid rule), ``reason`` (1: no child cell left, 2: a hop claimed no child cell, 3: the
        cap), ``launches`` and ``reads``."""
        Cn = self._mesh_partition_check("mesh_partition_nn", cur, u)
        k = len(parents)
        pv = np.ascontiguousarray(np.asarray(parent_vectors, np.float64))
        max_hops = int(max_hops)
        per = int(self.MESH_NN_HOPS_PER_READ if hops_per_read is None else hops_per_read)
        if (prev.dtype != torch.int32 or tuple(prev.shape) != (Cn,) or nbr.dtype != torch.int32 or tuple(nbr.shape) != (3, Cn)
                or not prev.is_contiguous() or not nbr.is_contiguous() or prev.device != self.device or nbr.device != self.device):
            raise ProcessingError("mesh_partition_nn: prev must be a contiguous int32 [C] tensor and nbr a contiguous int32 "
                                  "[3, C] tensor on the engine's device",
                                  details=f"got {prev.dtype} {tuple(prev.shape)} on {prev.device} and {nbr.dtype} "
                                          f"{tuple(nbr.shape)} on {nbr.device}")
        if not 1 <= k <= 10 or len(labels) != k or pv.shape != (3, k) or int(child) <= 0 or max_hops < 0 or per < 1:
            raise ProcessingError("mesh_partition_nn: 1 to 10 parents with one label and one vector each, a positive child ID, "
                                  "max_hops >= 0", details=f"{k} parents, {len(labels)} labels, vectors {pv.shape}, child {child}")
        if max_hops * 3 * k >= 1 << 24:
            raise ProcessingError(f"mesh_partition_nn: {max_hops} hops of {3 * k} substeps do not fit the 24-bit substep stamp")
        self._check_fits(4 * Cn + 32 + 32 * k, "mesh nearest-neighbour partition", f"one 32-bit owner word per cell, {Cn} cells")
        word = self._buf(None, "mnn_word", (Cn,), torch.int32, self.device)
        ctl = self._buf(None, "mnn_ctl", (8,), torch.int32, self.device)
        lab_d, pv_d = self._i32(labels), self._dev(pv)
        self.call("marex_mesh_nn_seed_i32", cur, prev, Cn, int(child), self._i32(parents), k, word, ctl)
        done = reads = 0
        while done < max_hops:
            n = min(per, max_hops - done)
            self.call("marex_mesh_nn_hops_i32", cur, nbr, Cn, int(child), k, done, n, max_hops, word, ctl)
            done += n
            reads += 1
            if int(ctl[2].item()):
                break
        self.call("marex_mesh_nn_finish_i32", cur, Cn, int(child), u, pv_d, k, lab_d, word, ctl, max_hops)
        c = ctl.cpu().numpy()
        return {"hops": int(c[3]), "leftover": int(c[4]), "reason": int(c[5]), "launches": 3 + done * (3 * k + 1), "reads": reads}

    def id_spans(self, ids: torch.Tensor):
        """``(tmin, tmax)`` int32 host arrays over IDs 0..max of ``ids`` int32 ``[T, C]``: the first / last timestep of
        every ID (INT_MAX / -1 when absent); ``None`` when the field has no ID > 0."""
        T, Cn = self._ids_check(ids)
        _, hi = self.ids_minmax(ids)
        if hi <= 0:
            return None
        tmin, tmax, _, _ = self._object_spans(ids, T, Cn, hi, "ID spans", f"per-ID first / last timestep for IDs 0..{hi}")
        return tmin.cpu().numpy(), tmax.cpu().numpy()

    def event_moments(self, ev: torch.Tensor, orig: torch.Tensor, ny: int, nx: int, n_ev: int,
                      weights: Optional[torch.Tensor] = None) -> Dict[str, np.ndarray]:
        """Per (timestep, event) of the event field ``ev`` (int32 ``[T, ny * nx]``, events 1..n_ev): ``mom`` int64
        ``[T, n_ev, 5]`` (cells, sum y, sum x, sum of x shifted by -nx right of nx / 2, near-edge flags), ``gid`` int32
        ``[T, n_ev]`` (largest ID of ``orig`` under the slot) and, with float32 ``weights`` of a slice, ``wmom`` float64
        ``[T, n_ev, 4]`` (sums of w, w y, w x, w x_shifted)."""
        T, Cn = self._ids_check(ev)
        self._ids_check(orig)
        slots = T * int(n_ev)
        self._check_fits(slots * (40 + 4 + (32 if weights is not None else 0)), "event properties",
                         f"{T} x {n_ev} dense (timestep, event) slots")
        acc = torch.empty((slots, 5), dtype=torch.int64, device=self.device)
        gid = torch.empty(slots, dtype=torch.int32, device=self.device)
        wacc = torch.empty((slots, 4), dtype=torch.float64, device=self.device) if weights is not None else None
        self.call("marex_event_moments_i32", ev, orig, T, int(ny), int(nx), int(n_ev), weights, acc, wacc, gid)
        out = {"mom": acc.cpu().numpy().reshape(T, n_ev, 5), "gid": gid.cpu().numpy().reshape(T, n_ev)}
        if wacc is not None:
            out["wmom"] = wacc.cpu().numpy().reshape(T, n_ev, 4)
        return out

    def _presence_window(self, what: str, x: torch.Tensor):
        """``(x, Tb, Cn)`` of a presence window, a bool one viewed as uint8."""
        if x.dim() != 2 or not x.is_contiguous() or x.device != self.device or x.dtype not in (torch.uint8, torch.bool, torch.int32):
            raise ProcessingError(f"{what}: the field must be a contiguous uint8, bool or int32 [T, C] tensor on the engine's "
                                  "device", details=f"got {x.dtype} {tuple(x.shape)} on {x.device}")
        if x.dtype == torch.bool:
            x = x.view(torch.uint8)
        return x, int(x.shape[0]), int(x.shape[1])

    def _anomaly_window_check(self, what: str, anom: torch.Tensor, Tb: int, Cn: int) -> None:
        if anom.dtype != torch.float32 or tuple(anom.shape) != (Tb, Cn) or not anom.is_contiguous() or anom.device != self.device:
            raise ProcessingError(f"{what}: the anomalies must be a contiguous float32 [{Tb}, {Cn}] tensor on the "
                                  f"engine's device", details=f"got {anom.dtype} {tuple(anom.shape)} on {anom.device}")

    def _upload_tables(self, tabs: dict) -> dict:
        """The ``"len"`` and ``"tabs"`` entries of the accumulators: the tables of :func:`label_tables` on the device."""
        return {"len": {k: (None if v is None else int(v.size)) for k, v in tabs.items()},
                "tabs": {k: (None if v is None else self._dev(v)) for k, v in tabs.items()}}

    @staticmethod
    def _window_check(what: str, acc: dict, plan: tuple, step_tables, t0: int, Tb: int, Cn: int) -> None:
        """The accumulators were planned for this call, every step table reaches the window's end, the window is not empty."""
        if acc["plan"] != plan:
            raise ProcessingError(f"{what}: the accumulators were planned for another call",
                                  details=f"{acc['plan']} there, {plan} here")
        for name in step_tables:
            n = acc["len"][name]
            if n is not None and n < t0 + Tb:
                raise ProcessingError(f"{what}: {name} has {n} labels, the window ends at step {t0 + Tb}")
        if Tb == 0 or Cn == 0:
            raise ProcessingError(f"{what}: an empty window ({Tb} steps of {Cn} cells)")

    @staticmethod
    def _stream_status(what: str, acc: dict, passes: int, ranges: str) -> None:
        """The host read of ``status``: negative cells, counted in each of the ``passes`` over a window, and lost ones."""
        neg, lost = (int(v) for v in acc["status"].cpu().numpy())
        if neg:
            raise create_data_validation_error("Object IDs must be non-negative",
                                               details=f"{neg // passes} negative cells; 0 is background",
                                               data_info={"negative_cells": neg // passes})
        if lost:
            raise ProcessingError(f"{what}: {lost} present cells lie under a step label outside its range",
                                  details=f"{ranges}; the cells were counted, nothing was written out of range")

    @staticmethod
    def _host(t: Optional[torch.Tensor], dt):
        return None if t is None else t.cpu().numpy().view(dt)

    def _cell_vector(self, what: str, name: str, v, torch_dtype, n: int, upload=False, typ: Optional[str] = None, noun: str = "values"):
        """``v`` (None stays None) as the contiguous ``torch_dtype`` ``[n]`` tensor on the engine's device that a kernel reads:
        another dtype (``typ`` in the refusal), shape, layout or device is refused.  ``upload``: a host array of that dtype and
        shape (``n noun`` in its refusal) is uploaded; ``"later"``: only a host array is taken, and returned for the caller to upload."""
        kind = str(torch_dtype).replace("torch.", "")
        if v is None:
            return None
        if upload == "later" or (upload and not isinstance(v, torch.Tensor)):
            h = np.ascontiguousarray(v)
            if h.dtype != np.dtype(kind) or h.shape != (n,):
                raise ProcessingError(f"{what}: {name} must be {n} {kind} {noun}", details=f"got {h.dtype} {h.shape}")
            return h if upload == "later" else self._dev(h)
        if v.dtype != torch_dtype or tuple(v.shape) != (n,) or not v.is_contiguous() or v.device != self.device:
            raise ProcessingError(f"{what}: {name} must be a contiguous {typ or torch_dtype} [{n}] tensor on the engine's device",
                                  details=f"got {v.dtype} {tuple(v.shape)} on {v.device}")
        return v

    def _weights_check(self, what: str, weights: Optional[torch.Tensor], Cn: int) -> None:
        self._cell_vector(what, "the weights", weights, torch.float32, Cn, typ="float32")

    @staticmethod
    def _area_q_check(what: str, q, Cn: int) -> np.ndarray:
        """The host ``q``, contiguous: ``Cn`` non-negative int64 fixed-point areas whose sum, so any sum of them, is below 2^62."""
        qh = np.ascontiguousarray(q)
        if qh.dtype != np.int64 or qh.shape != (Cn,) or (qh < 0).any() or int(qh.max()) >= 2**62 or \
                (int((qh >> 32).sum()) << 32) + int((qh & 0xFFFFFFFF).sum()) >= 2**62:  # the exact sum, in halves
            raise ProcessingError(f"{what}: q must be {Cn} non-negative int64 areas whose sum stays below 2^62",
                                  details=f"got {qh.dtype} {qh.shape}")
        return qh

    def _thresholds_check(self, what: str, thr: Optional[torch.Tensor], doy, Cn: int, sentence: str) -> None:
        """``thr`` is float32 ``[n_doy, Cn]`` and ``doy`` comes with it; ``sentence`` is the refusal."""
        if thr is None or doy is None or thr.dim() != 2 or thr.dtype != torch.float32 or int(thr.shape[1]) != Cn or \
                int(thr.shape[0]) <= 0 or not thr.is_contiguous() or thr.device != self.device:
            raise ProcessingError(f"{what}: {sentence}",
                                  details="one of thr / doy is missing" if thr is None or doy is None else
                                  f"got {thr.dtype} {tuple(thr.shape)} on {thr.device}")

    @staticmethod
    def _sections_check(what: str, sgrp, cls, G2: int, R: int, cats: Optional[bool] = None) -> bool:
        """Whether the call counts sections: ``sgrp`` and ``cls`` given, together, with ``G2 > 0`` and ``R > 0`` -- and, where
        the caller says whether it has thresholds (``cats``), with them."""
        sect = sgrp is not None or cls is not None
        if sect and (sgrp is None or cls is None or G2 <= 0 or R <= 0 or cats is False):
            raise ProcessingError(f"{what}: the section counts need step labels, cell classes, G2 > 0"
                                  f"{' and R > 0' if cats is None else ', R > 0 and thresholds'} together",
                                  details=f"G2 = {G2}, R = {R}" +
                                  ("" if cats is None else f", thresholds {'given' if cats else 'missing'}"))
        return sect

    def _whole_output_check(self, what: str, name: str, out: Optional[torch.Tensor], Cn: int, end: int,
                            second: Optional[bool] = None, dtype=torch.uint8) -> None:
        """``out`` (the ``name`` of the refusal) is the whole ``dtype`` ``[T, Cn]`` output and reaches the window's end -- and,
        where the caller has two passes, this is not the ``second``."""
        if out is not None and (second or out.dtype != dtype or out.dim() != 2 or int(out.shape[1]) != Cn or
                                int(out.shape[0]) < end or not out.is_contiguous() or out.device != self.device):
            raise ProcessingError(f"{what}: the {name} must be the whole contiguous {str(dtype).replace('torch.', '')} [T, {Cn}] output on the engine's "
                                  f"device, T >= {end}{'' if second is None else ', and belongs to the summary pass'}",
                                  details=f"got {out.dtype} {tuple(out.shape)} on {out.device}")

    def _event_slots(self, what: str, ev_tmin, ev_tmax, t0: int) -> tuple:
        """``(tmin, n_ev, t0, off, n_slots, alloc)`` of the spans ``ev_tmin`` / ``ev_tmax``: the slots of
        :meth:`event_slot_plan`, and how many to allocate."""
        tmin_h, tmax_h = np.asarray(ev_tmin, dtype=np.int64), np.asarray(ev_tmax, dtype=np.int64)
        n_ev = int(tmin_h.size) - 1
        t0 = int(t0)
        if n_ev <= 0 or tmin_h.ndim != 1 or tmax_h.shape != tmin_h.shape or t0 < 0:
            raise ProcessingError(f"{what}: ev_tmin and ev_tmax must have one entry per event 0..n_ev, n_ev > 0, and t0 "
                                  "must not be negative", details=f"spans {tmin_h.shape} / {tmax_h.shape}, t0 = {t0}")
        off = self.event_slot_plan(tmin_h, tmax_h)
        n_slots = int(off[-1])
        return tmin_h, n_ev, t0, off, n_slots, max(n_slots, 1)  # no event has a step: one slot that nothing addresses

    def _slot_tables(self, tmin_h: np.ndarray, off: np.ndarray) -> dict:
        """The ``"tmin"``, ``"off"`` and ``"plan"`` entries of the accumulators over event slots."""
        return {"tmin": self._dev(np.clip(tmin_h, 0, 2**31 - 1).astype(np.int32)), "off": self._dev(off), "plan": off}

    @staticmethod
    def _slot_acc_check(what: str, acc: dict, slots: str, alloc: int, off, n_doy: Optional[int] = None, weighted: bool = False):
        """The accumulators ``acc`` (``slots``: their entry by slot) were planned for these spans, ``n_doy`` rows and weights."""
        there = int(acc[slots].shape[0])
        same = there == alloc and np.array_equal(acc["plan"], off)
        if n_doy is None and not same:
            raise ProcessingError(f"{what}: the accumulators were planned for other spans", details=f"{there} slots there, {alloc} here")
        if n_doy is not None and (not same or acc["n_doy"] != n_doy or (acc["area"] is not None) != weighted):
            raise ProcessingError(f"{what}: the accumulators were planned for another call",
                                  details=f"{there} slots and {acc['n_doy']} threshold rows there, {alloc} and {n_doy} here")

    @staticmethod
    def _slot_status(what: str, acc: dict, n_doy: Optional[int] = None) -> None:
        """The host read of ``status``: cells outside their event's declared span and, with ``n_doy``, under a lost step label."""
        status = [int(v) for v in acc["status"].cpu().numpy()]
        if status[0]:
            raise ProcessingError(f"{what}: {status[0]} cells belong to an event outside its declared span of timesteps",
                                  details="ev_tmin / ev_tmax do not cover the field; the cells were counted, not accumulated")
        if n_doy is not None and status[1]:
            raise ProcessingError(f"{what}: {status[1]} event cells lie under a step label outside its range",
                                  details=f"doy must hold 0 .. {n_doy - 1}; the cells were counted, nothing was read out of range")

    @staticmethod
    def _table_bytes(tabs: dict) -> int:
        return sum(4 * v.size for v in tabs.values() if v is not None)

    def _zeros(self, name: str, shape, dtype) -> torch.Tensor:
        """A zeroed accumulator."""
        return self._buf(None, name, shape, dtype, self.device).zero_()

    @staticmethod
    def _key_max(key: np.ndarray) -> np.ndarray:
        """The float32 maxima of the uint32 keys the device raised; key 0 (none) is NaN."""
        return np.where(key != 0, key_float(key), np.float32(np.nan))

    @staticmethod
    def _key_step(key: np.ndarray, tmax: np.ndarray) -> np.ndarray:
        """The steps of those maxima; -1 where there is none."""
        return np.where(key != 0, tmax, np.int32(-1))

    @staticmethod
    def event_slot_plan(ev_tmin, ev_tmax, T: Optional[int] = None) -> np.ndarray:
        """The compact (timestep, event) slots of :meth:`event_rename` and :meth:`event_intensity`: ``off`` int64
        ``[n_ev + 2]``, the exclusive scan of the span lengths ``ev_tmax[e] - ev_tmin[e] + 1`` over the events 0..n_ev (entry
        0 unused).  An event with ``tmax < tmin``, a negative ``tmin`` or (with ``T``) a ``tmax`` past the field is absent and
        gets no slot.  Needs no device."""
        tmin_h, tmax_h = np.asarray(ev_tmin, dtype=np.int64), np.asarray(ev_tmax, dtype=np.int64)
        ok = (tmax_h >= tmin_h) & (tmin_h >= 0)
        if T is not None:
            ok &= tmax_h < T
        length = np.where(ok, tmax_h - tmin_h + 1, 0)
        length[:1] = 0
        off = np.zeros(tmin_h.size + 1, np.int64)
        np.cumsum(length, out=off[1:])
        return off

    def event_intensity(self, ids: torch.Tensor, anom: torch.Tensor, ev_tmin, ev_tmax, weights: Optional[torch.Tensor] = None,
                        t0: int = 0, acc: Optional[dict] = None, finish: bool = True) -> Dict[str, object]:
        """Per (timestep, event) intensity sums of the rows ``t0 .. t0 + Tb - 1`` of a tracked field
        (``marex_event_intensity_f32``): ``ids`` int32 ``[Tb, C]`` (events 1..n_ev, anything else background) and ``anom``
        float32 ``[Tb, C]``.  ``ev_tmin`` / ``ev_tmax`` (``[n_ev + 1]``, entry 0 unused, global timesteps) declare the slots
        as in :meth:`event_rename` (:meth:`event_slot_plan`).  ``weights``: float32 ``[C]`` or None for unit weights.  The
        first block allocates zeroed accumulators; a later block passes the ``"acc"`` entry of the previous result and adds
        into the same slots, whatever the block length.  Returns ``off``, ``acc`` and -- unless ``finish`` is False, which
        defers them and the one host read to a later block -- ``cnt`` int64 ``[n, 2]`` (finite cells, non-finite cells),
        ``sums`` float64 ``[n, 2]`` (sum of w, sum of w a over the finite cells) and ``vmax`` float32 ``[n]`` (NaN: no finite
        cell).  A cell of an event outside its declared span raises :class:`ProcessingError` (it was counted, nothing was
        written out of range)."""
        Tb, Cn = self._ids_check(ids)
        self._anomaly_window_check("event_intensity", anom, Tb, Cn)
        self._weights_check("event_intensity", weights, Cn)
        tmin_h, n_ev, t0, off, n_slots, alloc = self._event_slots("event_intensity", ev_tmin, ev_tmax, t0)
        if acc is None:
            self._check_fits(36 * n_slots + 12 * (n_ev + 2), "event intensity",
                             f"{n_slots} (timestep, event) slots between each event's first and last timestep, 36 bytes each, "
                             f"and the tables of {n_ev} events")
            acc = {"cnt": self._zeros("int_cnt", (alloc, 2), torch.int64), "sums": self._zeros("int_sums", (alloc, 2), torch.float64),
                   "vmax": self._zeros("int_vmax", (alloc,), torch.int32), "status": self._zeros("int_status", (1,), torch.int64),
                   **self._slot_tables(tmin_h, off)}
        else:
            self._slot_acc_check("event_intensity", acc, "cnt", alloc, off)
        self.call("marex_event_intensity_f32", ids, anom, t0, Tb, Cn, n_ev, acc["tmin"], acc["off"], alloc, weights,
                  acc["cnt"], acc["sums"], acc["vmax"], acc["status"])
        out = {"off": off, "acc": acc}
        if not finish:
            return out
        self._slot_status("event_intensity", acc)
        out.update(cnt=acc["cnt"][:n_slots].cpu().numpy(), sums=acc["sums"][:n_slots].cpu().numpy(),
                   vmax=key_float(acc["vmax"][:n_slots].cpu().numpy().view(np.uint32)))  # key 0: a NaN
        return out

    def event_shapes(self, ids: torch.Tensor, ny: int, nx: int, ev_tmin, ev_tmax, regional: bool = False,
                     mask: Optional[torch.Tensor] = None, area_q: Optional[torch.Tensor] = None,
                     ns_q: Optional[torch.Tensor] = None, ew_q: Optional[torch.Tensor] = None, t0: int = 0,
                     acc: Optional[dict] = None, finish: bool = True) -> Dict[str, object]:
        """Per (timestep, event) shape sums of the rows ``t0 .. t0 + Tb - 1`` of a tracked, gridded field
        (``marex_event_shapes_i32``): ``ids`` int32 ``[Tb, ny * nx]`` (events 1..n_ev, anything else background), the slots
        declared by ``ev_tmin`` / ``ev_tmax`` as in :meth:`event_intensity`.  ``regional``: x is not periodic.  ``mask``:
        uint8 ``[ny * nx]`` (0: land) or None; ``area_q``: int64 ``[ny * nx]`` fixed-point areas or None; ``ns_q`` int64
        ``[ny + 1]`` and ``ew_q`` int64 ``[ny]``: fixed-point side lengths, together or None.  The first block allocates the
        accumulators; a later block passes the ``"acc"`` entry of the previous result, whatever the block length.  Returns
        ``off``, ``acc`` and -- unless ``finish`` is False -- ``mom`` int64 ``[n, 16]`` and ``box`` int32 ``[n, 6]`` (the
        layout of include/marex_hip.h).  A cell of an event outside its declared span raises :class:`ProcessingError`."""
        Tb, Cn = self._ids_check(ids)
        ny, nx = int(ny), int(nx)
        if Cn != ny * nx or ny <= 0 or nx <= 0:
            raise ProcessingError(f"event_shapes: {Cn} cells per slice, ny * nx = {ny * nx}")
        for name, v, dt, n in (("mask", mask, torch.uint8, Cn), ("area_q", area_q, torch.int64, Cn),
                               ("ns_q", ns_q, torch.int64, ny + 1), ("ew_q", ew_q, torch.int64, ny)):
            self._cell_vector("event_shapes", name, v, dt, n)
        if (ns_q is None) != (ew_q is None):
            raise ProcessingError("event_shapes: ns_q and ew_q come together")
        tmin_h, n_ev, t0, off, n_slots, alloc = self._event_slots("event_shapes", ev_tmin, ev_tmax, t0)
        if acc is None:
            self._check_fits(152 * n_slots + 12 * (n_ev + 2), "event shapes",
                             f"{n_slots} (timestep, event) slots between each event's first and last timestep, 152 bytes each, "
                             f"and the tables of {n_ev} events")
            box = self._buf(None, "shp_box", (alloc, 6), torch.int32, self.device)
            box[:, 0::2] = 2**31 - 1
            box[:, 1::2] = -1
            acc = {"mom": self._zeros("shp_mom", (alloc, 16), torch.int64), "box": box,
                   "status": self._zeros("shp_status", (1,), torch.int64), **self._slot_tables(tmin_h, off)}
        else:
            self._slot_acc_check("event_shapes", acc, "mom", alloc, off)
        self.call("marex_event_shapes_i32", ids, t0, Tb, ny, nx, int(bool(regional)), n_ev, acc["tmin"], acc["off"], alloc,
                  mask, area_q, ns_q, ew_q, acc["mom"], acc["box"], acc["status"])
        out = {"off": off, "acc": acc}
        if not finish:
            return out
        self._slot_status("event_shapes", acc)
        out.update(mom=acc["mom"][:n_slots].cpu().numpy(), box=acc["box"][:n_slots].cpu().numpy())
        return out

    def mesh_event_shapes(self, ids: torch.Tensor, nbr: torch.Tensor, q: torch.Tensor, ev_tmin, ev_tmax,
                          mask: Optional[torch.Tensor] = None, len_q: Optional[torch.Tensor] = None,
                          lat_k: Optional[torch.Tensor] = None, lon_k: Optional[torch.Tensor] = None, t0: int = 0,
                          acc: Optional[dict] = None, finish: bool = True) -> Dict[str, object]:
        """Per (timestep, event) shape sums of the rows ``t0 .. t0 + Tb - 1`` of a tracked field on a mesh
        (``marex_mesh_event_shapes_i64``): ``ids`` int32 ``[Tb, C]`` (events 1..n_ev, anything else background), the slots
        declared by ``ev_tmin`` / ``ev_tmax`` as in :meth:`event_intensity`.  ``nbr``: int32 ``[3, C]``, 0-based, -1 for no
        neighbour; ``q``: int64 ``[10, C]`` fixed-point weights; ``mask``: uint8 ``[C]`` (0: land) or None; ``len_q``: int64
        ``[3, C]`` fixed-point side lengths or None; ``lat_k`` / ``lon_k``: int32 ``[C]`` coordinate keys, together or None
        (``box`` then stays as it was filled).  The first block allocates the accumulators; a later block passes the
        ``"acc"`` entry of the previous result, whatever the block length.  Returns ``off``, ``acc`` and -- unless ``finish``
        is False -- ``mom`` int64 ``[n, 16]`` and ``box`` int32 ``[n, 6]`` (the layout of include/marex_hip.h).  A cell of an
        event outside its declared span raises :class:`ProcessingError`."""
        Tb, Cn = self._ids_check(ids)
        for name, v, dt in (("mask", mask, torch.uint8), ("lat_k", lat_k, torch.int32), ("lon_k", lon_k, torch.int32)):
            self._cell_vector("mesh_event_shapes", name, v, dt, Cn)
        for name, v, dt, rows in (("nbr", nbr, torch.int32, 3), ("q", q, torch.int64, 10), ("len_q", len_q, torch.int64, 3)):
            if v is not None and (v.dtype != dt or tuple(v.shape) != (rows, Cn) or not v.is_contiguous() or v.device != self.device):
                raise ProcessingError(f"mesh_event_shapes: {name} must be a contiguous {dt} [{rows}, {Cn}] tensor on the engine's "
                                      "device", details=f"got {v.dtype} {tuple(v.shape)} on {v.device}")
        if nbr is None or q is None or (lat_k is None) != (lon_k is None):
            raise ProcessingError("mesh_event_shapes: nbr and q are needed, and lat_k and lon_k come together")
        tmin_h, n_ev, t0, off, n_slots, alloc = self._event_slots("mesh_event_shapes", ev_tmin, ev_tmax, t0)
        if acc is None:
            self._check_fits(152 * n_slots + 12 * (n_ev + 2), "mesh event shapes",
                             f"{n_slots} (timestep, event) slots between each event's first and last timestep, 152 bytes each, "
                             f"and the tables of {n_ev} events")
            box = self._buf(None, "msh_box", (alloc, 6), torch.int32, self.device)
            box[:, 0::2] = 2**31 - 1
            box[:, 1::2] = -2**31
            acc = {"mom": self._zeros("msh_mom", (alloc, 16), torch.int64), "box": box,
                   "status": self._zeros("msh_status", (1,), torch.int64), **self._slot_tables(tmin_h, off)}
        else:
            self._slot_acc_check("mesh_event_shapes", acc, "mom", alloc, off)
        self.call("marex_mesh_event_shapes_i64", ids, t0, Tb, Cn, n_ev, acc["tmin"], acc["off"], alloc, nbr, mask, q, len_q,
                  lat_k, lon_k, acc["mom"], acc["box"], acc["status"])
        out = {"off": off, "acc": acc}
        if not finish:
            return out
        self._slot_status("mesh_event_shapes", acc)
        out.update(mom=acc["mom"][:n_slots].cpu().numpy(), box=acc["box"][:n_slots].cpu().numpy())
        return out

    def event_categories(self, ids: torch.Tensor, anom: torch.Tensor, ev_tmin, ev_tmax, thr: torch.Tensor, doy,
                         weights: Optional[torch.Tensor] = None, t0: int = 0, field: Optional[torch.Tensor] = None,
                         acc: Optional[dict] = None, finish: bool = False) -> Dict[str, object]:
        """Per (timestep, event) severity categories of the rows ``t0 .. t0 + Tb - 1`` of a tracked field
        (``marex_event_categories_f32``): ``ids`` int32 and ``anom`` float32 ``[Tb, C]``, ``ev_tmin`` / ``ev_tmax`` and
        ``weights`` as in :meth:`event_intensity` (the same slots), ``thr`` float32 ``[n_doy, C]`` on the device and ``doy``
        (int ``[T]``, the row of ``thr`` of every global step).  ``field``: the WHOLE uint8 ``[T, C]`` output (the rows of
        this window are written: 0 no event, class + 1 otherwise), or None.  The first block allocates zeroed accumulators
        and uploads the tables; a later block passes the ``"acc"`` entry of the previous result, whatever the block length.
        Returns ``off``, ``acc`` and -- with ``finish``, which costs the one host read -- ``cat_cnt`` int64 ``[n, 7]``
        (cells below, moderate, strong, severe, extreme, undefined, with a non-finite anomaly) and ``cat_area`` float64
        ``[n, 6]`` (None without ``weights``).  A cell of an event outside its declared span, or under a ``doy`` label
        outside ``0 .. n_doy - 1``, raises :class:`ProcessingError` (it was counted, nothing was written out of range)."""
        Tb, Cn = self._ids_check(ids)
        self._anomaly_window_check("event_categories", anom, Tb, Cn)
        self._weights_check("event_categories", weights, Cn)
        self._thresholds_check("event_categories", thr, doy, Cn, f"the thresholds must be a contiguous float32 [n_doy, {Cn}] "
                               "tensor on the engine's device, with the row of every step")
        tmin_h, n_ev, t0, off, n_slots, alloc = self._event_slots("event_categories", ev_tmin, ev_tmax, t0)
        self._whole_output_check("event_categories", "field", field, Cn, t0 + Tb)
        n_doy = int(thr.shape[0])
        weighted = weights is not None
        if acc is None:
            tabs = label_tables("event_categories", (("doy", doy, None),))
            self._check_fits((56 + (48 if weighted else 0)) * n_slots + 12 * (n_ev + 2) + 4 * tabs["doy"].size + 16, "event categories",
                             f"{n_slots} (timestep, event) slots between each event's first and last timestep, "
                             f"{56 + (48 if weighted else 0)} bytes each, the tables of {n_ev} events and the row of every step")
            acc = {"cnt": self._zeros("cat_cnt", (alloc, 7), torch.int64),
                   "area": self._zeros("cat_area", (alloc, 6), torch.float64) if weighted else None,
                   "status": self._zeros("cat_status", (2,), torch.int64), **self._slot_tables(tmin_h, off),
                   "n_doy": n_doy, **self._upload_tables(tabs)}
        else:
            self._slot_acc_check("event_categories", acc, "cnt", alloc, off, n_doy, weighted)
        if acc["len"]["doy"] < t0 + Tb:
            raise ProcessingError(f"event_categories: doy has {acc['len']['doy']} labels, the window ends at step {t0 + Tb}")
        self.call("marex_event_categories_f32", ids, anom, t0, Tb, Cn, n_ev, acc["tmin"], acc["off"], alloc, thr,
                  acc["tabs"]["doy"], n_doy, weights, acc["cnt"], acc["area"], field, acc["status"])
        out: Dict[str, object] = {"off": off, "acc": acc}
        if not finish:
            return out
        self._slot_status("event_categories", acc, n_doy)
        out.update(cat_cnt=acc["cnt"][:n_slots].cpu().numpy(),
                   cat_area=acc["area"][:n_slots].cpu().numpy() if weighted else None)
        return out

    def occurrence(self, x: torch.Tensor, t0: int = 0, grp=None, G: int = 1, sgrp=None, G2: int = 0, cls=None, R: int = 0,
                   runs: bool = True, event_ids=(), acc: Optional[dict] = None, finish: bool = True) -> Dict[str, object]:
        """Occurrence statistics of the rows ``t0 .. t0 + Tb - 1`` of a mask or an ID field (``marex_occurrence_u8`` /
        ``marex_occurrence_i32``): ``x`` uint8, bool (read as uint8) or int32 ``[Tb, C]``; a cell is present where
        ``x > 0``.  ``grp`` (int ``[T]``, global steps, or None with ``G == 1``) labels the steps for the per-cell counts,
        ``sgrp`` (int ``[T]``) and ``cls`` (int ``[C]``; outside ``0 .. R - 1``: counted nowhere) the steps and the cells for
        the section counts, given together or not at all.  ``event_ids``: positive IDs, each counted on its own
        (``x == id``, one launch per ID on the same window).  The first window allocates zeroed accumulators and uploads the
        tables; a later window passes the ``"acc"`` entry of the previous result -- the window lengths do not matter, the
        run statistics are carried.  Returns ``acc`` and -- unless ``finish`` is False, which defers them and the one host
        read -- ``cell_cnt`` uint32 ``[G, C]``, ``runs`` uint32 ``[3, C]`` (open run, runs begun, longest run; None without
        ``runs``), ``sec_cnt`` uint64 ``[G2, R]`` (None without sections) and ``dur`` uint32 ``[K, C]``.  A negative ID
        raises the trackers' "Object IDs must be non-negative" error, a step label outside its range a
        :class:`ProcessingError`; both were counted, nothing was written out of range."""
        x, Tb, Cn = self._presence_window("occurrence", x)
        t0, G, G2, R = int(t0), int(G), int(G2), int(R)
        ids = [int(k) for k in event_ids]
        if t0 < 0 or G <= 0 or (grp is None and G != 1) or any(k <= 0 or k > 2**31 - 1 for k in ids):
            raise ProcessingError("occurrence: t0 must not be negative, G and the event IDs must be positive, and G > 1 needs labels",
                                  details=f"t0 = {t0}, G = {G}, labels {'given' if grp is not None else 'missing'}, event_ids {ids[:8]}")
        sect = self._sections_check("occurrence", sgrp, cls, G2, R)
        plan = (G, Cn, G2 if sect else 0, R if sect else 0, bool(runs), tuple(ids))
        if acc is None:
            tabs = label_tables("occurrence", (("grp", grp, None), ("sgrp", sgrp if sect else None, None),
                                               ("cls", cls if sect else None, Cn)))
            K = len(ids)
            need = 4 * G * Cn + (12 * Cn if runs else 0) + (8 * G2 * R if sect else 0) + 4 * K * Cn + 16 + self._table_bytes(tabs)
            self._check_fits(need, "occurrence",
                             f"{G} x {Cn} uint32 counts, {'3 x ' + str(Cn) + ' uint32 run statistics, ' if runs else ''}"
                             f"{G2 if sect else 0} x {R if sect else 0} uint64 section counts, {K} x {Cn} uint32 counts of "
                             f"selected events, and the label tables")
            acc = {"cell_cnt": self._zeros("occ_cnt", (G, Cn), torch.int32),
                   "runs": self._zeros("occ_runs", (3, Cn), torch.int32) if runs else None,
                   "sec_cnt": self._zeros("occ_sec", (G2, R), torch.int64) if sect else None,
                   "dur": self._zeros("occ_dur", (K, Cn), torch.int32) if K else None,
                   "status": self._zeros("occ_status", (2,), torch.int64), "plan": plan, **self._upload_tables(tabs)}
        self._window_check("occurrence", acc, plan, ("grp", "sgrp"), t0, Tb, Cn)
        fn = "marex_occurrence_i32" if x.dtype == torch.int32 else "marex_occurrence_u8"
        tb = acc["tabs"]
        self.call(fn, x, t0, Tb, Cn, 0, tb["grp"], G, tb["sgrp"], G2 if sect else 0, tb["cls"], R if sect else 0, acc["runs"],
                  acc["cell_cnt"], acc["sec_cnt"], acc["status"])
        for k, ev in enumerate(ids):  # the window is resident: one more pass over it per selected event
            self.call(fn, x, t0, Tb, Cn, ev, None, 1, None, 0, None, 0, None, acc["dur"][k], None, acc["status"])
        out: Dict[str, object] = {"acc": acc}
        if not finish:
            return out
        self._stream_status("occurrence", acc, 1 + len(ids), f"grp must hold 0 .. {G - 1}, sgrp 0 .. {G2 - 1}")
        host = self._host
        out.update(cell_cnt=host(acc["cell_cnt"], np.uint32), runs=host(acc["runs"], np.uint32),
                   sec_cnt=host(acc["sec_cnt"], np.uint64),
                   dur=host(acc["dur"], np.uint32) if ids else np.zeros((0, Cn), np.uint32))
        return out

    #: rows of the state a cell carries between the windows of :meth:`compound` (include/marex_hip.h)
    COMPOUND_STATE_ROWS = 13
    #: the largest ``max_lag`` / ``tolerance`` of :meth:`compound`: what the history words of a field hold
    COMPOUND_MAX_LAG = 30

    def compound(self, a: torch.Tensor, b: torch.Tensor, t0: int = 0, max_lag: int = 0, tolerance: int = 0, grp=None, G: int = 1,
                 sgrp=None, G2: int = 0, cls=None, R: int = 0, mask: Optional[torch.Tensor] = None, acc: Optional[dict] = None,
                 finish: bool = True) -> Dict[str, object]:
        """Compound events of the rows ``t0 .. t0 + Tb - 1`` of two presence fields (``marex_compound_u8``): ``a`` and ``b``
        uint8 or bool (read as uint8) ``[Tb, C]``, present where nonzero.  ``max_lag`` and ``tolerance``: ``0 .. 30``.
        ``grp``, ``G``, ``sgrp``, ``G2``, ``cls`` and ``R`` as in :meth:`occurrence`.  ``mask``: the WHOLE contiguous uint8
        ``[T, C]`` joint mask on the engine's device, ``T >= t0 + Tb`` (the rows of this window are written, zeros
        included), or None.  The first window allocates zeroed accumulators and uploads the tables; a later window passes
        the ``"acc"`` entry of the previous result -- the window lengths do not matter, histories, open and waiting runs
        are carried.  Returns ``acc`` and -- unless ``finish`` is False, which defers them and the one host read --
        ``days`` uint32 ``[3, G, C]`` (steps with A, with B, with both), ``runs`` uint32 ``[3, C]`` (the joint mask's open
        run, runs begun, longest run), ``co`` uint32 ``[4, C]`` (runs of A, coincident runs of A, runs of B, coincident runs
        of B), ``lag_days`` uint32 ``[2 max_lag + 1, C]`` (None with ``max_lag == 0``) and ``sec_cnt`` uint64
        ``[3, G2, R]`` (None without sections).  A step label outside its range raises :class:`ProcessingError`; its
        cells were counted, nothing was written out of range."""
        a, Tb, Cn = self._presence_window("compound", a)
        b, Tb_b, Cn_b = self._presence_window("compound", b)
        if a.dtype != torch.uint8 or b.dtype != torch.uint8 or (Tb_b, Cn_b) != (Tb, Cn):
            raise ProcessingError("compound: both fields must be uint8 or bool windows of one shape",
                                  details=f"got {a.dtype} {tuple(a.shape)} and {b.dtype} {tuple(b.shape)}")
        ints = (t0, max_lag, tolerance, G, G2, R)
        if any(isinstance(v, bool) or not isinstance(v, (int, np.integer)) for v in ints):
            raise ProcessingError("compound: t0, max_lag, tolerance, G, G2 and R must be integers", details=f"got {ints}")
        t0, L, K, G, G2, R = (int(v) for v in ints)
        if t0 < 0 or G <= 0 or (grp is None and G != 1) or not 0 <= L <= self.COMPOUND_MAX_LAG or not 0 <= K <= self.COMPOUND_MAX_LAG:
            raise ProcessingError(f"compound: t0 must not be negative, G must be positive, G > 1 needs labels, and max_lag and "
                                  f"tolerance must lie in 0 .. {self.COMPOUND_MAX_LAG}",
                                  details=f"t0 = {t0}, G = {G}, labels {'given' if grp is not None else 'missing'}, max_lag = {L}, "
                                          f"tolerance = {K}")
        sect = self._sections_check("compound", sgrp, cls, G2, R)
        self._whole_output_check("compound", "mask", mask, Cn, t0 + Tb)
        S = self.COMPOUND_STATE_ROWS
        plan = (G, Cn, G2 if sect else 0, R if sect else 0, L, K)
        if acc is None:
            tabs = label_tables("compound", (("grp", grp, None), ("sgrp", sgrp if sect else None, None),
                                             ("cls", cls if sect else None, Cn)))
            rows = 3 * G + S + (2 * L + 1 if L else 0)
            need = 4 * rows * Cn + (24 * G2 * R if sect else 0) + 16 + self._table_bytes(tabs)
            self._check_fits(need, "compound",
                             f"3 x {G} x {Cn} uint32 counts, {S} x {Cn} uint32 of carried state, {2 * L + 1 if L else 0} x {Cn} "
                             f"uint32 lag counts, 3 x {G2 if sect else 0} x {R if sect else 0} uint64 section counts, and the "
                             f"label tables")
            acc = {"cell_cnt": self._zeros("cmp_cnt", (3, G, Cn), torch.int32), "state": self._zeros("cmp_state", (S, Cn), torch.int32),
                   "lag": self._zeros("cmp_lag", (2 * L + 1, Cn), torch.int32) if L else None,
                   "sec_cnt": self._zeros("cmp_sec", (3, G2, R), torch.int64) if sect else None,
                   "status": self._zeros("cmp_status", (2,), torch.int64), "plan": plan, **self._upload_tables(tabs)}
        self._window_check("compound", acc, plan, ("grp", "sgrp"), t0, Tb, Cn)
        tb = acc["tabs"]
        self.call("marex_compound_u8", a, b, t0, Tb, Cn, L, K, tb["grp"], G, tb["sgrp"], G2 if sect else 0, tb["cls"],
                  R if sect else 0, acc["state"], acc["cell_cnt"], acc["lag"], acc["sec_cnt"], mask, acc["status"])
        out: Dict[str, object] = {"acc": acc}
        if not finish:
            return out
        self._stream_status("compound", acc, 1, f"grp must hold 0 .. {G - 1}, sgrp 0 .. {G2 - 1}")
        host = self._host
        state = host(acc["state"], np.uint32)
        out.update(days=host(acc["cell_cnt"], np.uint32), runs=state[0:3], co=state[7:11], lag_days=host(acc["lag"], np.uint32),
                   sec_cnt=host(acc["sec_cnt"], np.uint64))
        return out

    #: the largest ``max_lag`` of :meth:`event_composites`: the ``2 L + 1`` lags of an anchor are the lanes of one wave
    COMPOSITES_MAX_LAG = 30
    #: ``anchor`` of :meth:`event_composites` as the library takes it
    COMPOSITES_ANCHORS = {"onset": 0, "end": 1}

    @staticmethod
    def composites_rows(a: int, b: int, T: int, max_lag: int) -> Tuple[int, int]:
        """``(first, end)`` of the rows that the anchors at the steps ``a .. b - 1`` need: ``H = max(max_lag, 1)`` steps of
        halo on both sides, inside the record."""
        H = max(int(max_lag), 1)
        return max(0, a - H), min(T, b + H)

    def event_composites(self, x: torch.Tensor, v: torch.Tensor, r0: int, a: int, b: int, T: int, max_lag: int = 10,
                         anchor: str = "onset", grp=None, G: int = 1, acc: Optional[dict] = None,
                         finish: bool = True) -> Dict[str, object]:
        """Lagged composites of ``v`` around the anchors at the steps ``a .. b - 1`` (``marex_event_composites_u8``): ``x``
        uint8 or bool (read as uint8) and ``v`` float32, both ``[Tr, C]``, are the rows ``r0 .. r0 + Tr - 1`` of a record of
        ``T`` steps and must cover :meth:`composites_rows` -- the halo is read but owns no anchors, nothing else is carried
        between windows.  ``anchor``: ``"onset"`` (a step ``s > 0`` with ``x[s]`` and not ``x[s - 1]``) or ``"end"`` (a step
        ``e < T - 1`` with ``x[e]`` and not ``x[e + 1]``); ``max_lag``: ``0 .. 30``; ``grp`` (int ``[T]``, global steps, or
        None with ``G == 1``) labels the anchors by their own step.  The first window allocates zeroed accumulators and
        uploads the labels; a later window passes the ``"acc"`` entry of the previous result -- the windows do not matter,
        not even to the last bit of the sums.  Returns ``acc`` and -- unless ``finish`` is False, which defers them and the
        one host read -- ``anchors`` uint32 ``[G, C]``, ``count`` uint32, ``sum`` and ``sumsq`` float64 ``[G, 2 L + 1, C]``
        (the device holds them cell-major, ``[G, C, 2 L + 1]``).  An anchor under a label outside ``0 .. G - 1`` raises
        :class:`ProcessingError`; it was counted, nothing was written out of range."""
        what = "event_composites"
        x, Tr, Cn = self._presence_window(what, x)
        if x.dtype != torch.uint8:
            raise ProcessingError(f"{what}: the field must be a uint8 or bool window", details=f"got {x.dtype} {tuple(x.shape)}")
        self._anomaly_window_check(what, v, Tr, Cn)
        ints = (r0, a, b, T, max_lag, G)
        if any(isinstance(k, bool) or not isinstance(k, (int, np.integer)) for k in ints):
            raise ProcessingError(f"{what}: r0, a, b, T, max_lag and G must be integers", details=f"got {ints}")
        r0, a, b, T, L, G = (int(k) for k in ints)
        if not isinstance(anchor, str) or anchor not in self.COMPOSITES_ANCHORS or not 0 <= L <= self.COMPOSITES_MAX_LAG or G <= 0 or (grp is None and G != 1):
            raise ProcessingError(f"{what}: anchor must be 'onset' or 'end', max_lag must lie in 0 .. {self.COMPOSITES_MAX_LAG}, "
                                  "G must be positive, and G > 1 needs labels",
                                  details=f"anchor = {anchor!r}, max_lag = {L}, G = {G}, labels {'given' if grp is not None else 'missing'}")
        if not (0 <= r0 and r0 + Tr <= T and 0 <= a < b <= T):
            raise ProcessingError(f"{what}: needs 0 <= r0, r0 + Tr <= T and 0 <= a < b <= T",
                                  details=f"r0 = {r0}, Tr = {Tr}, a = {a}, b = {b}, T = {T}")
        lo, hi = self.composites_rows(a, b, T, L)
        if r0 > lo or r0 + Tr < hi:
            raise ProcessingError(f"{what}: the rows {r0} .. {r0 + Tr - 1} do not cover the halo of the steps {a} .. {b - 1}",
                                  details=f"with max_lag = {L} they must cover {lo} .. {hi - 1}")
        W = 2 * L + 1
        plan = (G, Cn, L, anchor, T)
        if acc is None:
            tabs = label_tables(what, (("grp", grp, None),))
            need = G * Cn * (4 + 20 * W) + 8 + self._table_bytes(tabs)
            self._check_fits(need, what, f"{G} x {Cn} cells of 4 + 20 x {W} bytes (anchors; count, sum and sum of squares of "
                                         f"{W} lags), and the label table")
            acc = {"anchors": self._zeros("cps_anchors", (G, Cn), torch.int32), "cnt": self._zeros("cps_cnt", (G, Cn, W), torch.int32),
                   "sum": self._zeros("cps_sum", (G, Cn, W), torch.float64), "sumsq": self._zeros("cps_sumsq", (G, Cn, W), torch.float64),
                   "status": self._zeros("cps_status", (1,), torch.int64), "plan": plan, **self._upload_tables(tabs)}
        self._window_check(what, acc, plan, ("grp",), 0, T, Cn)
        self.call("marex_event_composites_u8", x, v, r0, Tr, a, b, T, Cn, L, self.COMPOSITES_ANCHORS[anchor], acc["tabs"]["grp"],
                  G, acc["anchors"], acc["sum"], acc["sumsq"], acc["cnt"], acc["status"])
        out: Dict[str, object] = {"acc": acc}
        if not finish:
            return out
        lost = int(acc["status"].cpu().numpy()[0])
        if lost:
            raise ProcessingError(f"{what}: {lost} anchors lie under a step label outside its range",
                                  details=f"grp must hold 0 .. {G - 1}; the anchors were counted, nothing was written out of range")
        lags_first = lambda t, dt: np.ascontiguousarray(self._host(t, dt).transpose(0, 2, 1))  # noqa: E731
        out.update(anchors=self._host(acc["anchors"], np.uint32), count=lags_first(acc["cnt"], np.uint32),
                   sum=lags_first(acc["sum"], np.float64), sumsq=lags_first(acc["sumsq"], np.float64))
        return out

    #: the longest series :meth:`trend_stats` and :meth:`trend_select` take (include/marex_hip.h)
    TREND_MAX_STEPS = 256

    def _trend_check(self, what: str, y: torch.Tensor, x: torch.Tensor) -> tuple:
        """``(G, C)`` of the maps ``y`` float64 ``[G, C]`` over ``x`` float64 ``[G]``, both contiguous on the engine's device."""
        for name, t, nd in (("y", y, 2), ("x", x, 1)):
            if not isinstance(t, torch.Tensor) or t.dtype != torch.float64 or t.dim() != nd or not t.is_contiguous() or \
                    t.device != self.device:
                raise ProcessingError(f"{what}: {name} must be a contiguous float64 {'[G, C]' if nd == 2 else '[G]'} tensor on "
                                      "the engine's device",
                                      details=f"got {getattr(t, 'dtype', type(t).__name__)} {tuple(getattr(t, 'shape', ()))} on "
                                              f"{getattr(t, 'device', 'the host')}")
        G, Cn = int(y.shape[0]), int(y.shape[1])
        if int(x.shape[0]) != G or not 2 <= G <= self.TREND_MAX_STEPS or not 0 < Cn < 2**31 - 1:
            raise ProcessingError(f"{what}: y must be [G, C] and x [G] with 2 <= G <= {self.TREND_MAX_STEPS} and 0 < C < 2^31 - 1",
                                  details=f"got y {tuple(y.shape)} and x {tuple(x.shape)}")
        return G, Cn

    def trend_stats(self, y: torch.Tensor, x: torch.Tensor) -> Dict[str, torch.Tensor]:
        """Per cell of the maps ``y`` float64 ``[G, C]`` over the abscissae ``x`` float64 ``[G]`` (finite and strictly
        increasing: the caller checks; a non-finite sample of ``y`` is missing), in one launch (``marex_trend_stats_f64``):
        ``n`` int32 ``[C]`` valid samples, ``s`` int32 ``[C]`` the Mann-Kendall S, ``ties`` int32 ``[C]`` the sum over the
        tie groups of ``t (t - 1)(2 t + 5)``, ``med`` float64 ``[2, C]`` the medians of the valid y and of their x, ``sums``
        float64 ``[5, C]``: x mean, y mean, Sxx, Sxy, Syy.  Device tensors; nothing is read back."""
        G, Cn = self._trend_check("trend_stats", y, x)
        self._check_fits(4 * 3 * Cn + 8 * 7 * Cn + 16, "trend_stats", f"3 x {Cn} int32 and 7 x {Cn} float64 of results")
        buf = lambda name, shape, dt: self._buf(None, name, shape, dt, self.device)  # noqa: E731
        out = {"n": buf("trend_n", (Cn,), torch.int32), "s": buf("trend_s", (Cn,), torch.int32),
               "ties": buf("trend_ties", (Cn,), torch.int32), "med": buf("trend_med", (2, Cn), torch.float64),
               "sums": buf("trend_sums", (5, Cn), torch.float64)}
        status = torch.zeros((2,), dtype=torch.int64, device=self.device)
        self.call("marex_trend_stats_f64", y, x, G, Cn, out["n"], out["s"], out["ties"], out["med"], out["sums"], status)
        return out

    def trend_select(self, y: torch.Tensor, x: torch.Tensor, ranks) -> torch.Tensor:
        """Order statistics of the pairwise slopes ``((y[j] - y[i]) / (x[j] - x[i])) + 0.0``, ``i < j`` both valid, of every
        cell (``marex_trend_select_f64``): ``ranks`` int32 ``[K, C]`` (an array or a tensor), returns float64 ``[K, C]`` on
        the device, the ``ranks[k, c]``-th smallest slope of cell ``c`` (0-based), NaN for a rank outside ``0 .. P - 1``.
        Synchronises for the status word: a selection that did not close in 64 bisection steps raises
        :class:`ProcessingError` (its output is NaN, nothing else was written)."""
        G, Cn = self._trend_check("trend_select", y, x)
        r = ranks if isinstance(ranks, torch.Tensor) else torch.from_numpy(np.ascontiguousarray(ranks))
        if r.dtype != torch.int32 or r.dim() != 2 or int(r.shape[1]) != Cn or int(r.shape[0]) < 1:
            raise ProcessingError(f"trend_select: ranks must be int32 [K, {Cn}] with K >= 1",
                                  details=f"got {r.dtype} {tuple(r.shape)}")
        K = int(r.shape[0])
        self._check_fits(12 * K * Cn + 16, "trend_select", f"{K} x {Cn} int32 ranks and as many float64 results")
        r = r.to(self.device).contiguous()
        out = self._buf(None, "trend_sel", (K, Cn), torch.float64, self.device)
        status = torch.zeros((2,), dtype=torch.int64, device=self.device)
        self.call("marex_trend_select_f64", y, x, G, Cn, r, K, out, status)
        open_ = int(status[1].item())
        if open_:
            raise ProcessingError(f"trend_select: {open_} selections did not close within 64 bisection steps",
                                  details="their results are NaN; this is a defect of the kernel, not of the data")
        return out

    def local_intensity(self, x: torch.Tensor, anom: torch.Tensor, t0: int = 0, grp=None, G: int = 1,
                        thr: Optional[torch.Tensor] = None, doy=None, sgrp=None, G2: int = 0, cls=None, R: int = 0,
                        acc: Optional[dict] = None, finish: bool = True, match: int = 0) -> Dict[str, object]:
        """Per-cell intensity of the rows ``t0 .. t0 + Tb - 1`` (``marex_local_intensity_u8`` /
        ``marex_local_intensity_i32``): ``x`` uint8, bool (read as uint8) or int32 ``[Tb, C]`` (present where ``x > 0``, or
        where ``x == match``) and ``anom`` float32 ``[Tb, C]``.  ``grp`` (int ``[T]``, global steps, or None with
        ``G == 1``) labels the steps.  ``thr`` (float32 ``[n_doy, C]`` on the device) with ``doy`` (int ``[T]``, the row of
        ``thr`` of every global step) adds the category counts; ``sgrp`` (int ``[T]``) and ``cls`` (int ``[C]``; outside
        ``0 .. R - 1``: counted nowhere) the section counts, which need ``thr``.  The first window allocates zeroed
        accumulators and uploads the tables; a later window passes the ``"acc"`` entry of the previous result -- the window
        lengths do not matter, not even to the last bit of ``sum``.  Returns ``acc`` and -- unless ``finish`` is False,
        which defers them and the one host read -- ``days`` and ``invalid`` uint32 ``[G, C]``, ``sum`` float64 ``[G, C]``,
        ``vmax`` float32 ``[G, C]`` (NaN: none), ``tmax`` int32 ``[G, C]`` (-1: none), ``cat_days`` uint32 ``[G, 6, C]``
        and ``sec_cnt`` uint64 ``[G2, R, 6]`` (None without thresholds / sections).  A negative ID raises the trackers'
        "Object IDs must be non-negative" error, a step label outside its range a :class:`ProcessingError`; both were
        counted, nothing was written out of range."""
        x, Tb, Cn = self._presence_window("local_intensity", x)
        self._anomaly_window_check("local_intensity", anom, Tb, Cn)
        t0, G, G2, R, match = int(t0), int(G), int(G2), int(R), int(match)
        cats = thr is not None or doy is not None
        if t0 < 0 or G <= 0 or (grp is None and G != 1) or match < 0 or match > 2**31 - 1:
            raise ProcessingError("local_intensity: t0 and match must not be negative, G must be positive, and G > 1 needs labels",
                                  details=f"t0 = {t0}, G = {G}, labels {'given' if grp is not None else 'missing'}, match = {match}")
        if cats:
            self._thresholds_check("local_intensity", thr, doy, Cn, f"the categories need thresholds, a contiguous float32 "
                                   f"[n_doy, {Cn}] tensor on the engine's device, and the row of every step")
        sect = self._sections_check("local_intensity", sgrp, cls, G2, R, cats)
        n_doy = int(thr.shape[0]) if cats else 0
        plan = (G, Cn, n_doy, G2 if sect else 0, R if sect else 0, match)
        if acc is None:
            tabs = label_tables("local_intensity", (("grp", grp, None), ("doy", doy if cats else None, None),
                                                    ("sgrp", sgrp if sect else None, None), ("cls", cls if sect else None, Cn)))
            need = G * Cn * (24 + (24 if cats else 0)) + (48 * G2 * R if sect else 0) + 16 + self._table_bytes(tabs)
            self._check_fits(need, "local intensity",
                             f"{G} x {Cn} cells of {24 + (24 if cats else 0)} bytes (days, invalid, sum, maximum, its step"
                             f"{', six category counts' if cats else ''}), {G2 if sect else 0} x {R if sect else 0} x 6 uint64 "
                             f"section counts, and the label tables")
            acc = {"days": self._zeros("li_days", (G, Cn), torch.int32), "invalid": self._zeros("li_invalid", (G, Cn), torch.int32),
                   "sum": self._zeros("li_sum", (G, Cn), torch.float64), "vmax": self._zeros("li_vmax", (G, Cn), torch.int32),
                   "tmax": self._zeros("li_tmax", (G, Cn), torch.int32),
                   "cat_days": self._zeros("li_cat", (G, 6, Cn), torch.int32) if cats else None,
                   "sec_cnt": self._zeros("li_sec", (G2, R, 6), torch.int64) if sect else None,
                   "status": self._zeros("li_status", (2,), torch.int64), "plan": plan, **self._upload_tables(tabs)}
        self._window_check("local_intensity", acc, plan, ("grp", "doy", "sgrp"), t0, Tb, Cn)
        fn = "marex_local_intensity_i32" if x.dtype == torch.int32 else "marex_local_intensity_u8"
        tb = acc["tabs"]
        self.call(fn, x, anom, t0, Tb, Cn, match, tb["grp"], G, thr if cats else None, tb["doy"], n_doy, tb["sgrp"],
                  G2 if sect else 0, tb["cls"], R if sect else 0, acc["days"], acc["invalid"], acc["sum"], acc["vmax"],
                  acc["tmax"], acc["cat_days"], acc["sec_cnt"], acc["status"])
        out: Dict[str, object] = {"acc": acc}
        if not finish:
            return out
        self._stream_status("local_intensity", acc, 1, f"grp must hold 0 .. {G - 1}, doy 0 .. {n_doy - 1}, sgrp 0 .. {G2 - 1}")
        host = self._host
        key = host(acc["vmax"], np.uint32)
        out.update(days=host(acc["days"], np.uint32), invalid=host(acc["invalid"], np.uint32), sum=host(acc["sum"], np.float64),
                   vmax=self._key_max(key), tmax=self._key_step(key, host(acc["tmax"], np.int32)),
                   cat_days=host(acc["cat_days"], np.uint32), sec_cnt=host(acc["sec_cnt"], np.uint64))
        return out

    def _float_window(self, what: str, x: torch.Tensor) -> tuple:
        """``(rows, Cn)`` of a window of a float32 field."""
        if not isinstance(x, torch.Tensor) or x.dim() != 2 or x.dtype != torch.float32 or not x.is_contiguous() or x.device != self.device:
            raise ProcessingError(f"{what}: the field must be a contiguous float32 [T, C] tensor on the engine's device",
                                  details=f"got {getattr(x, 'dtype', type(x))} {tuple(getattr(x, 'shape', ()))} on "
                                          f"{getattr(x, 'device', 'the host')}")
        return int(x.shape[0]), int(x.shape[1])

    def group_mean(self, x: torch.Tensor, lab, G: int, t0: int = 0, acc: Optional[dict] = None, finish: bool = True) -> Dict[str, object]:
        """Per (label, cell) the count and the sequential float64 sum of the finite samples of the rows ``t0 .. t0 + Tb - 1``
        (``marex_group_mean_f32``): ``x`` float32 ``[Tb, C]``, ``lab`` int ``[T]`` by the global step, -1 (the step is
        skipped) or ``0 .. G - 1``.  The first window allocates zeroed accumulators and uploads the labels; a later window
        passes the ``"acc"`` entry of the previous result -- the window lengths do not matter, not even to the last bit of
        ``sum``.  Returns ``acc`` and, with ``finish``, ``sum`` float64 and ``cnt`` uint32 ``[G, C]``.  A label outside
        ``-1 .. G - 1`` raises :class:`ProcessingError`; its cells were counted, nothing was written out of range."""
        Tb, Cn = self._float_window("group_mean", x)
        t0, G = int(t0), int(G)
        if t0 < 0 or G <= 0 or lab is None:
            raise ProcessingError("group_mean: t0 must not be negative, G must be positive, and the steps need labels",
                                  details=f"t0 = {t0}, G = {G}, labels {'given' if lab is not None else 'missing'}")
        plan = (G, Cn)
        if acc is None:
            tabs = label_tables("group_mean", (("lab", lab, None),))
            self._check_fits(12 * G * Cn + 8 + self._table_bytes(tabs), "group mean",
                             f"{G} x {Cn} cells of 12 bytes (sum, count) and the label table")
            acc = {"sum": self._zeros("gm_sum", (G, Cn), torch.float64), "cnt": self._zeros("gm_cnt", (G, Cn), torch.int32),
                   "status": self._zeros("gm_status", (1,), torch.int64), "plan": plan, **self._upload_tables(tabs)}
        self._window_check("group_mean", acc, plan, ("lab",), t0, Tb, Cn)
        self.call("marex_group_mean_f32", x, t0, Tb, Cn, acc["tabs"]["lab"], G, acc["sum"], acc["cnt"], acc["status"])
        out: Dict[str, object] = {"acc": acc}
        if not finish:
            return out
        lost = int(acc["status"].cpu().numpy()[0])
        if lost:
            raise ProcessingError(f"group_mean: {lost} cells lie under a step label outside its range",
                                  details=f"lab must hold -1 .. {G - 1}; the cells were counted, nothing was written out of range")
        out.update(sum=self._host(acc["sum"], np.float64), cnt=self._host(acc["cnt"], np.uint32))
        return out

    #: the most alert levels and the longest window of :meth:`heat_stress`
    HEAT_STRESS_MAX_LEVELS, HEAT_STRESS_MAX_WINDOW = 6, 366

    def heat_stress(self, x: torch.Tensor, mmm, t0: int = 0, lead: int = 0, window: int = 84, hotspot_min: float = 1.0,
                    steps_per_week: float = 7.0, levels=(4.0, 8.0), grp=None, G: int = 1, dhw: Optional[torch.Tensor] = None,
                    alert: Optional[torch.Tensor] = None, summary: bool = True, acc: Optional[dict] = None,
                    finish: bool = True) -> Dict[str, object]:
        """Accumulated heat stress of the rows ``t0 .. t0 + Tb - 1`` (``marex_heat_stress_f32``): ``x`` float32
        ``[lead + Tb, C]`` begins ``lead = min(window, t0)`` rows before the window -- the history that leaves the running
        sum -- and ``mmm`` is the float32 ``[C]`` threshold (a host array is uploaded).  ``grp`` (int ``[T]``, global steps,
        or None with ``G == 1``) labels the steps.  ``dhw`` / ``alert``: the WHOLE float32 / uint8 ``[T, C]`` outputs, or
        None.  The first window allocates the zeroed carried sum and accumulators and uploads the tables; a later window
        passes the ``"acc"`` entry of the previous result and must begin where that ended -- the window lengths do not
        matter to any bit.  Returns ``acc`` and, with ``finish`` and ``summary``, ``dhw_max`` and ``hotspot_max`` float32
        (NaN: none), ``tmax`` int32 (-1: none), ``invalid`` uint32 ``[G, C]``, ``alert_steps`` uint32 ``[G, 3 + L, C]`` and
        ``onset`` int32 ``[G, L, C]`` (-1: none).  A step label outside ``0 .. G - 1`` raises :class:`ProcessingError`; its
        cells were counted, nothing was written out of range."""
        rows, Cn = self._float_window("heat_stress", x)
        t0, lead, G = int(t0), int(lead), int(G)
        lev = np.asarray(levels, dtype=np.float32).reshape(-1)
        L = int(lev.size)
        hmin, spw = float(np.float32(hotspot_min)), float(steps_per_week)
        if isinstance(window, bool) or not isinstance(window, (int, np.integer)) or not 1 <= window <= self.HEAT_STRESS_MAX_WINDOW or \
                not 2.0 ** -10 <= hmin < 1024.0 or not (spw > 0 and np.isfinite(spw)) or L > self.HEAT_STRESS_MAX_LEVELS or \
                not np.isfinite(lev).all() or not (np.diff(lev) > 0).all():
            raise ProcessingError(f"heat_stress: window must be an integer in 1 .. {self.HEAT_STRESS_MAX_WINDOW}, hotspot_min in "
                                  f"[2^-10, 1024), steps_per_week positive and finite, levels at most "
                                  f"{self.HEAT_STRESS_MAX_LEVELS} finite, strictly increasing values",
                                  details=f"window = {window!r}, hotspot_min = {hotspot_min!r}, steps_per_week = "
                                          f"{steps_per_week!r}, levels = {lev.tolist()}")
        window = int(window)
        if t0 < 0 or lead != min(window, t0) or G <= 0 or (grp is None and G != 1):
            raise ProcessingError("heat_stress: t0 must not be negative, lead must be min(window, t0), G must be positive, and "
                                  "G > 1 needs labels",
                                  details=f"t0 = {t0}, lead = {lead}, window = {window}, G = {G}, labels "
                                          f"{'given' if grp is not None else 'missing'}")
        Tb = rows - lead
        end = t0 + max(Tb, 0)
        self._whole_output_check("heat_stress", "dhw output", dhw, Cn, end, dtype=torch.float32)
        self._whole_output_check("heat_stress", "alert output", alert, Cn, end)
        plan = (G, Cn, window, hmin, spw, tuple(lev.tolist()), bool(summary))
        if acc is None:
            tabs = label_tables("heat_stress", (("grp", grp, None),))
            per = 16 + 4 * (3 + L) + 4 * max(L, 1) if summary else 0
            self._check_fits(8 * Cn + G * Cn * per + 8 + self._table_bytes(tabs), "heat stress",
                             f"{Cn} cells of 8 bytes of carried sum, {G} x {Cn} cells of accumulators, {per} bytes each, and the "
                             "label table")
            acc = {"state": self._zeros("hs_state", (Cn,), torch.float64), "status": self._zeros("hs_status", (1,), torch.int64),
                   "mmm": self._cell_vector("heat_stress", "mmm", mmm, torch.float32, Cn, upload=True, typ="float32"),
                   "levels": self._dev(lev if L else np.zeros(1, np.float32)), "plan": plan, "next": t0,
                   **{k: None for k in ("dhw_max", "tmax", "hotspot_max", "alert_steps", "invalid", "onset")},
                   **self._upload_tables(tabs)}
            if summary:
                for k in ("dhw_max", "tmax", "hotspot_max", "invalid"):
                    acc[k] = self._zeros("hs_" + k, (G, Cn), torch.int32)
                acc["alert_steps"] = self._zeros("hs_alert_steps", (G, 3 + L, Cn), torch.int32)
                acc["onset"] = self._zeros("hs_onset", (G, max(L, 1), Cn), torch.int32)
        self._window_check("heat_stress", acc, plan, ("grp",), t0, Tb, Cn)
        if Tb < 0 or t0 != acc["next"]:
            raise ProcessingError("heat_stress: the windows must follow each other, each with its history rows in front",
                                  details=f"the window begins at step {t0} with {rows} rows and lead {lead}; step {acc['next']} is next")
        self.call("marex_heat_stress_f32", x, acc["mmm"], t0, lead, Tb, Cn, window, hmin, spw, acc["levels"], L, acc["tabs"]["grp"], G,
                  acc["state"], acc["dhw_max"], acc["tmax"], acc["hotspot_max"], acc["alert_steps"], acc["invalid"], acc["onset"],
                  dhw, alert, acc["status"])
        acc["next"] = t0 + Tb
        out: Dict[str, object] = {"acc": acc}
        if not finish:
            return out
        lost = int(acc["status"].cpu().numpy()[0])
        if lost:
            raise ProcessingError(f"heat_stress: {lost} cells lie under a step label outside its range",
                                  details=f"grp must hold 0 .. {G - 1}; the cells were counted, nothing was written out of range")
        if summary:
            host = self._host
            key, on = host(acc["dhw_max"], np.uint32), host(acc["onset"], np.int32)[:, :L]
            out.update(dhw_max=self._key_max(key), tmax=self._key_step(key, host(acc["tmax"], np.int32)),
                       hotspot_max=self._key_max(host(acc["hotspot_max"], np.uint32)), invalid=host(acc["invalid"], np.uint32),
                       alert_steps=host(acc["alert_steps"], np.uint32), onset=(on - 1).astype(np.int32))
        return out

    #: the largest voxel grid of :meth:`voxel_table` (the stopping margin of marex_nearest.hip is derived for it)
    NEAREST_MAX_VOXELS = 1024

    def _unit_vectors(self, what: str, name: str, v) -> torch.Tensor:
        """``v`` as the contiguous float64 ``[3, N]`` table on the engine's device (a host array is uploaded)."""
        if not isinstance(v, torch.Tensor):
            h = np.ascontiguousarray(v)
            if h.dtype != np.float64 or h.ndim != 2 or h.shape[0] != 3:
                raise ProcessingError(f"{what}: {name} must be float64 [3, N] unit vectors", details=f"got {h.dtype} {h.shape}")
            v = self._dev(h)
        if v.dtype != torch.float64 or v.dim() != 2 or int(v.shape[0]) != 3 or int(v.shape[1]) < 1 or not v.is_contiguous() or \
                v.device != self.device:
            raise ProcessingError(f"{what}: {name} must be a contiguous, non-empty float64 [3, N] tensor on the engine's device",
                                  details=f"got {v.dtype} {tuple(v.shape)} on {v.device}")
        return v

    def nearest_brute(self, src, ids, dst, sel=None, index: Optional[torch.Tensor] = None, q: Optional[torch.Tensor] = None):
        """The exact nearest source of every target (``marex_nearest_brute_f64``): ``src`` float64 ``[3, N]`` unit vectors with
        their cell numbers ``ids`` int32 ``[N]`` (None: ``0 .. N - 1``), ``dst`` float64 ``[3, M]``.  ``sel`` (int32 ``[K]``
        device tensor) restricts the search to the targets it lists and needs ``index`` and ``q``, which keep every other
        entry.  Returns the device tensors ``(index int32 [M], q float64 [M])``: the smallest ``(q, cell number)``, -1 and
        +inf for a target with a NaN coordinate."""
        what = "nearest_brute"
        src, dst = self._unit_vectors(what, "the sources", src), self._unit_vectors(what, "the targets", dst)
        N, M = int(src.shape[1]), int(dst.shape[1])
        ids = self._cell_vector(what, "the cell numbers", ids, torch.int32, N, upload=True, typ="int32")
        if sel is None:
            index, q, K = self._buf(None, "nn_index", (M,), torch.int32, self.device), self._buf(None, "nn_q", (M,), torch.float64, self.device), M
        else:
            self._cell_vector(what, "the index", index, torch.int32, M, typ="int32")
            self._cell_vector(what, "q", q, torch.float64, M, typ="float64")
            K = int(sel.numel())
            if index is None or q is None or sel.dtype != torch.int32 or sel.dim() != 1 or not 1 <= K <= M:
                raise ProcessingError(f"{what}: a target list needs 1 .. M int32 entries and the index and q it continues",
                                      details=f"got {sel.dtype} {tuple(sel.shape)} for {M} targets")
        self.call("marex_nearest_brute_f64", src, ids, N, dst, M, sel, K, index, q)
        return index, q

    def voxel_table(self, src, ids, n: int) -> Dict[str, object]:
        """The sources binned into ``n^3`` voxels over ``[-1, 1]^3`` (``marex_voxel_count_f64``, a prefix sum,
        ``marex_voxel_scatter_f64``): ``sorted`` float64 ``[3, N]`` and ``ids`` int32 ``[N]`` in voxel order, ``off`` int32
        ``[n^3 + 1]``, ``n``.  The table is dense: ``16 n^3`` bytes while it is built (counts, their int64 prefix sum, offsets),
        ``4 n^3`` afterwards."""
        what = "voxel_table"
        src = self._unit_vectors(what, "the sources", src)
        N = int(src.shape[1])
        if isinstance(n, bool) or not isinstance(n, (int, np.integer)) or not 1 <= n <= self.NEAREST_MAX_VOXELS:
            raise ProcessingError(f"{what}: the voxel grid must have 1 .. {self.NEAREST_MAX_VOXELS} voxels per axis", details=f"n = {n!r}")
        n = int(n)
        ids = self._cell_vector(what, "the cell numbers", ids, torch.int32, N, upload=True, typ="int32")
        self._check_fits(16 * n ** 3 + 28 * N, "voxel table",
                         f"{n}^3 voxels of 16 bytes while the table is built (counts, their 64-bit prefix sum, offsets) and {N} sources of 28 bytes")
        count = self._zeros("nn_count", (n ** 3,), torch.int32)
        self.call("marex_voxel_count_f64", src, N, n, count)
        off = torch.zeros((n ** 3 + 1,), dtype=torch.int32, device=self.device)
        off[1:] = torch.cumsum(count, 0)  # plumbing: N < 2^31, so the int64 sums fit int32
        count.zero_()
        srt, sid = self._buf(None, "nn_sorted", (3, N), torch.float64, self.device), self._buf(None, "nn_sorted_ids", (N,), torch.int32, self.device)
        self.call("marex_voxel_scatter_f64", src, ids, N, n, off, count, srt, sid)
        return {"sorted": srt, "ids": sid, "off": off, "n": n}

    def nearest_voxel(self, table: dict, dst, max_rings: int, qmax: float = float("inf")):
        """The ring search of ``marex_nearest_voxel_f64`` over a :meth:`voxel_table`: the device tensors ``(index int32 [M],
        q float64 [M], flag uint8 [M])``; ``flag`` 1 marks a target still open after ``max_rings`` rings."""
        what = "nearest_voxel"
        dst = self._unit_vectors(what, "the targets", dst)
        M, N, n = int(dst.shape[1]), int(table["sorted"].shape[1]), int(table["n"])
        max_rings, qmax = int(max_rings), float(qmax)
        if max_rings < 0 or not qmax >= 0 or tuple(table["off"].shape) != (n ** 3 + 1,) or tuple(table["ids"].shape) != (N,):
            raise ProcessingError(f"{what}: max_rings and qmax must not be negative, and the table must be that of voxel_table",
                                  details=f"max_rings = {max_rings}, qmax = {qmax}, offsets {tuple(table['off'].shape)} for n = {n}")
        index, q = self._buf(None, "nn_index", (M,), torch.int32, self.device), self._buf(None, "nn_q", (M,), torch.float64, self.device)
        flag = self._buf(None, "nn_flag", (M,), torch.uint8, self.device)
        self.call("marex_nearest_voxel_f64", table["sorted"], table["ids"], N, table["off"], n, dst, M, max_rings, qmax, index, q, flag)
        return index, q, flag

    def nearest_index(self, src, ids, dst, method: str = "brute", voxels: Optional[int] = None, max_rings: Optional[int] = None,
                      qmax: float = float("inf")) -> Dict[str, object]:
        """The nearest eligible source cell of every target, on the host: ``index`` int32 ``[M]`` (a cell number of ``ids``,
        -1: none) and ``q`` float64 ``[M]`` (its squared chord, +inf: none), ``fallback`` (the targets the ring search left
        to the brute kernel) and ``voxels``.  ``method``: ``"brute"``, or ``"voxel"`` with ``voxels`` per axis and
        ``max_rings`` (None: ``voxels``, the rings that always cover the grid).  ``qmax``: the ring search may give up on a
        target whose nearest source has ``q > qmax``; what it then reports for that target is not defined beyond that."""
        if method not in ("brute", "voxel"):
            raise ProcessingError("nearest_index: the method is 'brute' or 'voxel'", details=f"method = {method!r}")
        src, dst = self._unit_vectors("nearest_index", "the sources", src), self._unit_vectors("nearest_index", "the targets", dst)
        fallback = 0
        if method == "brute":
            index, q = self.nearest_brute(src, ids, dst)
            voxels = 0
        else:
            table = self.voxel_table(src, ids, voxels)
            index, q, flag = self.nearest_voxel(table, dst, table["n"] if max_rings is None else max_rings, qmax)
            sel = torch.nonzero(flag).reshape(-1).to(torch.int32)  # a synchronising compaction: plumbing
            fallback = int(sel.numel())
            if fallback:
                self.nearest_brute(table["sorted"], table["ids"], dst, sel=sel, index=index, q=q)
        return {"index": self._host(index, np.int32), "q": self._host(q, np.float64), "fallback": fallback, "voxels": int(voxels)}

    def resample_nearest(self, x: torch.Tensor, index: torch.Tensor, out: torch.Tensor, fill) -> None:
        """``out [Tb, M] = x [Tb, C]`` gathered through ``index`` int32 ``[M]``, ``fill`` where the index is negative
        (``marex_resample_nearest_u8`` / ``_i32`` / ``_f32`` by the dtype of ``x``: uint8, int32 or float32).  ``out`` is a
        contiguous tensor of that dtype, for instance the rows of a window in the whole output."""
        what = "resample_nearest"
        names = {torch.uint8: "marex_resample_nearest_u8", torch.int32: "marex_resample_nearest_i32", torch.float32: "marex_resample_nearest_f32"}
        if not isinstance(x, torch.Tensor) or x.dim() != 2 or x.dtype not in names or not x.is_contiguous() or x.device != self.device:
            raise ProcessingError(f"{what}: the field must be a contiguous uint8, int32 or float32 [T, C] tensor on the engine's device",
                                  details=f"got {getattr(x, 'dtype', type(x))} {tuple(getattr(x, 'shape', ()))} on "
                                          f"{getattr(x, 'device', 'the host')}")
        Tb, Cn = int(x.shape[0]), int(x.shape[1])
        if not isinstance(index, torch.Tensor) or index.dtype != torch.int32 or index.dim() != 1 or index.device != self.device:
            raise ProcessingError(f"{what}: the index must be an int32 [M] tensor on the engine's device",
                                  details=f"got {getattr(index, 'dtype', type(index))} {tuple(getattr(index, 'shape', ()))}")
        M = int(index.shape[0])
        if not isinstance(out, torch.Tensor) or out.dtype != x.dtype or tuple(out.shape) != (Tb, M) or not out.is_contiguous() or \
                out.device != self.device:
            raise ProcessingError(f"{what}: the output must be a contiguous {x.dtype} [{Tb}, {M}] tensor on the engine's device",
                                  details=f"got {getattr(out, 'dtype', type(out))} {tuple(getattr(out, 'shape', ()))}")
        if x.dtype == torch.float32:
            fill = float(fill)
        else:
            lo, hi = (0, 255) if x.dtype == torch.uint8 else (-2 ** 31, 2 ** 31 - 1)
            if isinstance(fill, float) and not fill.is_integer() or not lo <= int(fill) <= hi:
                raise ProcessingError(f"{what}: the fill of a {x.dtype} field must be an integer in {lo} .. {hi}", details=f"fill = {fill!r}")
            fill = int(fill)
        if Tb == 0 or M == 0:
            return
        if Cn == 0:
            out.fill_(fill)
            return
        self.call(names[x.dtype], x, Tb, Cn, index, M, fill, out)

    #: the most regions of :meth:`regional_series`
    REGIONAL_MAX_REGIONS = 32767

    @staticmethod
    def regional_layout(cells_per_lane: int) -> Tuple[int, int, int]:
        """``(cells of a wave per row, cells of a workgroup per row, rows between two of a workgroup's)`` of the kernels of
        ``marex_regional_series_*``, as the library was compiled (``marex_regional_layout``): at four cells per lane (a
        uint8 field without thresholds, ``C % 4 == 0``, aligned arrays) and at one.  Needs no device."""
        out = (C.c_int32 * 3)()
        if _lib.load().marex_regional_layout(int(cells_per_lane), out) != 0:
            raise ProcessingError(f"regional_layout: cells_per_lane must be 1 or 4, got {cells_per_lane}")
        return int(out[0]), int(out[1]), int(out[2])

    @staticmethod
    def regional_slot_bytes(T: int, R: int, anomalies: bool, categories: bool, areas: bool) -> int:
        """The bytes of the ``T x R`` slots of :meth:`regional_series` and of their spare row: area and two counts (24 per
        slot), with anomalies two sums and the maximum's key (24, the key padded to 8), with thresholds six counts (48)
        and, with areas, six areas (48)."""
        per = 24 + (24 if anomalies else 0) + (48 if categories else 0) + (48 if categories and areas else 0)
        return (int(T) + 1) * int(R) * per

    def regional_series(self, x: torch.Tensor, reg, R: int, T: int, t0: int = 0, q=None, wf=None,
                        anom: Optional[torch.Tensor] = None, thr: Optional[torch.Tensor] = None, doy=None, match: int = 0,
                        acc: Optional[dict] = None, finish: bool = True) -> Dict[str, object]:
        """Per (timestep, region) series of the rows ``t0 .. t0 + Tb - 1`` of a ``[T, C]`` mask or ID field
        (``marex_regional_series_u8`` / ``marex_regional_series_i32``): ``x`` uint8, bool (read as uint8) or int32
        ``[Tb, C]`` (present where ``x > 0``, or where ``x == match``).  ``reg`` (int ``[C]``): the region of every cell,
        outside ``0 .. R - 1``: none.  ``q`` (int64 ``[C]``, the fixed-point areas of ``track_mesh.mesh_weight_tables`` row
        0; None: 1 per cell) and ``wf`` (float32 ``[C]``, the weights of the anomaly sums, needs ``anom``; None: 1) are host
        arrays.  ``anom`` float32 ``[Tb, C]`` adds the sums and the maximum; ``thr`` (float32 ``[n_doy, C]`` on the device)
        with ``doy`` (int ``[T]``, the row of ``thr`` of every global step) the categories, which need ``anom``.  The first
        window allocates the ``T x R`` slots (and one spare row of them that nothing addresses), zeroes them and uploads
        the tables; a later window passes the ``"acc"`` entry of the previous result -- the window lengths do not matter.
        Returns ``acc`` and -- unless ``finish`` is False, which defers them and the one host read -- ``area`` int64
        ``[T, R]`` (the sum of ``q``, or the cells), ``cnt`` int64 ``[T, R, 2]`` (cells counted in ``area``; present cells
        with a non-finite anomaly, which count for nothing else), ``sums`` float64 ``[T, R, 2]`` (sum of ``wf``, sum of
        ``wf`` x anomaly), ``vmax`` float32 ``[T, R]`` (NaN: none), ``cat_cnt`` int64 ``[T, R, 6]`` and ``cat_area`` int64
        ``[T, R, 6]`` (None without anomalies / thresholds / ``q``).  A negative ID raises the trackers' "Object IDs must be
        non-negative" error, a ``doy`` label outside its range a :class:`ProcessingError`; both were counted, nothing was
        written out of range."""
        x, Tb, Cn = self._presence_window("regional_series", x)
        t0, R, T, match = int(t0), int(R), int(T), int(match)
        cats = thr is not None or doy is not None
        if t0 < 0 or T < t0 + Tb or R <= 0 or R > self.REGIONAL_MAX_REGIONS or match < 0 or match > 2**31 - 1:
            raise ProcessingError(f"regional_series: t0 and match must not be negative, the window must end inside the {T} steps "
                                  f"of the slots, and R must lie in 1 .. {self.REGIONAL_MAX_REGIONS}",
                                  details=f"t0 = {t0}, Tb = {Tb}, R = {R}, match = {match}")
        if anom is None and (wf is not None or cats):
            raise ProcessingError("regional_series: weights and thresholds need the anomalies")
        if anom is not None:
            self._anomaly_window_check("regional_series", anom, Tb, Cn)
        if cats:
            self._thresholds_check("regional_series", thr, doy, Cn, f"the categories need thresholds, a contiguous float32 "
                                   f"[n_doy, {Cn}] tensor on the engine's device, and the row of every step")
        n_doy = int(thr.shape[0]) if cats else 0
        plan = (T, R, Cn, n_doy, match, q is not None, wf is not None, anom is not None)
        if acc is None:
            tabs = label_tables("regional_series", (("reg", reg, Cn), ("doy", doy if cats else None, None)))
            qh = None if q is None else self._area_q_check("regional_series", q, Cn)  # checked here, uploaded once it fits
            wh = self._cell_vector("regional_series", "wf", wf, torch.float32, Cn, upload="later", noun="weights")
            slots_b = self.regional_slot_bytes(T, R, anom is not None, cats, q is not None)
            self._check_fits(slots_b + 16 + self._table_bytes(tabs) + (8 * Cn if q is not None else 0) +
                             (4 * Cn if wf is not None else 0), "regional series",
                             f"{T} x {R} (timestep, region) slots of {slots_b // ((T + 1) * R)} bytes, the region of every cell"
                             f"{', its area' if q is not None else ''}{', its weight' if wf is not None else ''} and the label tables")

            def slots(name, tail, dtype):  # T rows that the kernel adds into, one more that it must leave alone
                b = self._buf(None, name, (T + 1, R) + tail, dtype, self.device)
                b[:T].zero_()
                return b

            acc = {"area": slots("reg_area", (), torch.int64), "cnt": slots("reg_cnt", (2,), torch.int64),
                   "sums": slots("reg_sums", (2,), torch.float64) if anom is not None else None,
                   "vmax": slots("reg_vmax", (), torch.int32) if anom is not None else None,
                   "cat_cnt": slots("reg_cat_cnt", (6,), torch.int64) if cats else None,
                   "cat_area": slots("reg_cat_area", (6,), torch.int64) if cats and q is not None else None,
                   "status": self._zeros("reg_status", (2,), torch.int64), "plan": plan,
                   "q": None if qh is None else self._dev(qh), "wf": None if wh is None else self._dev(wh),
                   **self._upload_tables(tabs)}
        self._window_check("regional_series", acc, plan, ("doy",), t0, Tb, Cn)
        fn = "marex_regional_series_i32" if x.dtype == torch.int32 else "marex_regional_series_u8"
        tb = acc["tabs"]
        self.call(fn, x, t0, Tb, Cn, T, match, tb["reg"], R, acc["q"], acc["wf"], anom, thr if cats else None, tb["doy"], n_doy,
                  acc["area"], acc["cnt"], acc["sums"], acc["vmax"], acc["cat_cnt"], acc["cat_area"], acc["status"])
        out: Dict[str, object] = {"acc": acc}
        if not finish:
            return out
        self._stream_status("regional_series", acc, 1, f"doy must hold 0 .. {n_doy - 1}")

        def host(name, dt):
            return None if acc[name] is None else acc[name][:T].cpu().numpy().view(dt)

        key = host("vmax", np.uint32)
        out.update(area=host("area", np.int64), cnt=host("cnt", np.int64), sums=host("sums", np.float64),
                   vmax=None if key is None else self._key_max(key), cat_cnt=host("cat_cnt", np.int64),
                   cat_area=host("cat_area", np.int64))
        return out

    @staticmethod
    def exposure_layout() -> Dict[str, int]:
        """What the kernels of ``marex_event_exposure_*`` were compiled with (``marex_event_exposure_layout``): the cells of
        a ``piece``, a ``wave`` and a workgroup (``wg``) per row, the rows between two of a workgroup's (``row_stride``) and
        the ``id_bits``, ``rank_bits`` and ``step_bits`` of the key.  Needs no device."""
        out = (C.c_int32 * 7)()
        if _lib.load().marex_event_exposure_layout(out) != 0:
            raise ProcessingError("exposure_layout: the library refused the call")
        return dict(zip(("piece", "wave", "wg", "row_stride", "id_bits", "rank_bits", "step_bits"), (int(v) for v in out)))

    @staticmethod
    def exposure_key(step, rank, ident) -> np.ndarray:
        """The uint64 keys of ``(step within the window, region rank, ID)``: ``id << 33 | rank << 17 | step``."""
        L = HotPath.exposure_layout()
        s, r, i = (np.asarray(v).astype(np.uint64) for v in (step, rank, ident))
        return (i << np.uint64(L["rank_bits"] + L["step_bits"])) | (r << np.uint64(L["step_bits"])) | s

    @staticmethod
    def exposure_home(key, cap: int) -> np.ndarray:
        """The entry at which the probes of ``key`` begin in a table of ``cap`` entries: the splitmix64 finaliser of the
        kernels (marex_common.hip.h), for tests that place keys in the table."""
        with np.errstate(over="ignore"):
            k = np.asarray(key, dtype=np.uint64).copy()
            k ^= k >> np.uint64(30)
            k *= np.uint64(0xbf58476d1ce4e5b9)
            k ^= k >> np.uint64(27)
            k *= np.uint64(0x94d049bb133111eb)
            k ^= k >> np.uint64(31)
        return (k & np.uint64(int(cap) - 1)).astype(np.int64)

    @staticmethod
    def exposure_entry_bytes(areas: bool, anomalies: bool) -> int:
        """The bytes of one table entry of :meth:`event_exposure`: key and counts (16), the area (8), two sums and the
        maximum's key (20)."""
        return 16 + (8 if areas else 0) + (20 if anomalies else 0)

    @staticmethod
    def exposure_cap(runs: int) -> int:
        """The table of :meth:`event_exposure` for ``runs`` runs: a power of two, at least 64, load factor <= 1/2 even if
        every run were a key of its own."""
        return max(64, 1 << max(2 * int(runs) - 1, 1).bit_length())

    def event_exposure(self, ids: torch.Tensor, rank, R: int, t0: int = 0, q=None, wf=None, anom: Optional[torch.Tensor] = None,
                       cap: Optional[int] = None) -> Dict[str, object]:
        """The (timestep, region, event) records of one window of a tracked field (``marex_event_exposure_count_i32`` /
        ``marex_event_exposure_i32``): ``ids`` int32 ``[Tb, C]`` (a cell belongs to event ``ids > 0``), the rows
        ``t0 .. t0 + Tb - 1``; ``rank`` int32 ``[C]``, the region rank of every cell, outside ``0 .. R - 1``: no region, which
        is kept under rank ``R``.  ``q`` (int64 ``[C]``, the fixed-point areas of ``regional.area_weight_table``; None: 1 per
        cell), ``wf`` (float32 ``[C]``, the weights of the anomaly sums, needs ``anom``; None: 1) and ``rank`` are host arrays
        or tensors on the engine's device (a caller with many windows uploads them once).  ``anom`` float32 ``[Tb, C]`` adds
        the sums and the maximum.  ``cap`` overrides the planned table size (tests).

        Returns host arrays sorted by ``(id, rank, t)``: ``t`` int64 (global steps), ``rank`` and ``id`` int32, ``cells`` and
        ``finite`` int64 (all cells; those with a finite anomaly -- all of them without ``anom``), ``area`` int64 (the sum of
        ``q`` over all cells, or the cells), ``sums`` float64 ``[n, 2]`` (sum of ``wf``, sum of ``wf`` x anomaly over the
        finite cells) and ``vmax`` float32 (NaN: none), both None without ``anom``; and ``runs``, ``cap`` and
        ``table_bytes``, what the count pass found and the table took.  A negative ID raises the trackers' "Object IDs must
        be non-negative" error; a table that the keys do not fit raises :class:`ProcessingError` and leaves the engine as
        it was."""
        Tb, Cn = self._ids_check(ids)
        L = self.exposure_layout()
        t0, R = int(t0), int(R)
        if t0 < 0 or R <= 0 or R > self.REGIONAL_MAX_REGIONS or Tb > 1 << L["step_bits"] or Tb == 0 or Cn == 0:
            raise ProcessingError(f"event_exposure: t0 must not be negative, R must lie in 1 .. {self.REGIONAL_MAX_REGIONS} and a "
                                  f"window must hold 1 .. {1 << L['step_bits']} steps of at least one cell",
                                  details=f"t0 = {t0}, Tb = {Tb}, C = {Cn}, R = {R}")
        if anom is None and wf is not None:
            raise ProcessingError("event_exposure: weights need the anomalies")
        if anom is not None:
            self._anomaly_window_check("event_exposure", anom, Tb, Cn)
        from .exposure import _no_records  # the front end of this method: it imports the engine only when it runs
        if q is not None and not isinstance(q, torch.Tensor):  # a host vector is checked and uploaded, a tensor is checked
            self._area_q_check("event_exposure", q, Cn)
        reg_d, q_d, w_d = (self._cell_vector("event_exposure", name, v, dt, Cn, upload=True)
                           for name, v, dt in (("rank", rank, torch.int32), ("q", q, torch.int64), ("wf", wf, torch.float32)))
        an, ar = anom is not None, q_d is not None
        empty = dict(_no_records(an), runs=0, cap=0, table_bytes=0)
        status = self._buf(None, "exp_status", (8,), torch.int64, self.device)
        self.call("marex_event_exposure_count_i32", ids, Tb, Cn, reg_d, R, status)
        s = status.cpu().numpy()
        neg, runs = int(s[0]), int(s[2])
        if neg:
            raise create_data_validation_error("Object IDs must be non-negative", details=f"{neg} negative cells; 0 is background",
                                               data_info={"negative_cells": neg})
        if runs == 0:
            return empty
        planned = self.exposure_cap(runs)
        cap = planned if cap is None else int(cap)
        if cap < 64 or cap & (cap - 1):
            raise ProcessingError(f"event_exposure: cap={cap} is not a power of two >= 64")
        per = self.exposure_entry_bytes(ar, an)
        n_out = min(runs, cap)
        nbytes = per * (cap + n_out)
        self._check_fits(nbytes, "event exposure", f"a hash table of {cap} entries of {per} bytes for {runs} runs of equal "
                         f"(timestep, region, event) keys, and {n_out} compacted entries")
        dev = self.device

        def pair(name, tail, dtype, on=True):
            if not on:
                return None, None
            return self._buf(None, "exp_" + name, (cap,) + tail, dtype, dev), self._buf(None, "exp_out_" + name, (n_out,) + tail, dtype, dev)

        keys, out_k = pair("keys", (), torch.int64)
        cnt, out_c = pair("cnt", (), torch.int64)
        area, out_a = pair("area", (), torch.int64, ar)
        sums, out_s = pair("sums", (2,), torch.float64, an)
        vmax, out_v = pair("vmax", (), torch.int32, an)
        self.call("marex_event_exposure_i32", ids, Tb, Cn, reg_d, R, q_d, w_d, anom, cap, keys, cnt, area, sums, vmax, status,
                  n_out, out_k, out_c, out_a, out_s, out_v)
        s = status.cpu().numpy()
        n = int(s[3])
        if s[1] != 0 or not 0 < n <= n_out:
            raise ProcessingError(f"event_exposure: the table of {cap} entries does not hold the keys of {runs} runs",
                                  details=f"{n} entries were taken; a table planned by the engine holds {planned}")
        k = out_k[:n].cpu().numpy().view(np.uint64)
        order = np.argsort(k, kind="stable")
        k = k[order]
        c = out_c[:n].cpu().numpy().view(np.uint64)[order]
        sb, rb = np.uint64(L["step_bits"]), np.uint64(L["rank_bits"])
        cells = (c & np.uint64(0xFFFFFFFF)).astype(np.int64)
        out = dict(empty, runs=runs, cap=cap, table_bytes=nbytes,
                   t=(k & np.uint64((1 << L["step_bits"]) - 1)).astype(np.int64) + t0,
                   rank=((k >> sb) & np.uint64((1 << L["rank_bits"]) - 1)).astype(np.int32), id=(k >> (sb + rb)).astype(np.int32),
                   cells=cells, finite=(c >> np.uint64(32)).astype(np.int64),
                   area=out_a[:n].cpu().numpy()[order] if ar else cells.copy())
        if an:
            out.update(sums=out_s[:n].cpu().numpy()[order], vmax=self._key_max(out_v[:n].cpu().numpy().view(np.uint32)[order]))
        return out

    @staticmethod
    def matching_layout() -> Dict[str, int]:
        """What the kernels of ``marex_event_matching_*`` were compiled with (``marex_event_matching_layout``): the cells of
        a ``piece``, a ``wave`` and a workgroup (``wg``) per row, the rows between two of a workgroup's (``row_stride``),
        the most bits an ID takes (``id_bits``) and the fewest that remain for the step (``min_step_bits``).  Needs no device."""
        out = (C.c_int32 * 6)()
        if _lib.load().marex_event_matching_layout(out) != 0:
            raise ProcessingError("matching_layout: the library refused the call")
        return dict(zip(("piece", "wave", "wg", "row_stride", "id_bits", "min_step_bits"), (int(v) for v in out)))

    @staticmethod
    def matching_widths(max_a: int, max_b: int, Tb: int) -> tuple:
        """``(bits_a, bits_b, bits_step)`` of the key of :meth:`event_matching` for a window of ``Tb`` steps whose largest
        IDs are ``max_a`` and ``max_b``: the bit lengths of the two (at least 1 each) and, for the step, what the window
        needs (at least 1) or what is left of 64 bits -- at least 2.  A window of more than ``2^bits_step`` steps is run in
        pieces of that many."""
        max_a, max_b, Tb = int(max_a), int(max_b), int(Tb)
        if not (0 <= max_a < 2**31 and 0 <= max_b < 2**31 and Tb >= 1):
            raise ProcessingError("matching_widths: IDs lie in 0 .. 2^31 - 1 and a window holds at least one step",
                                  details=f"max_a = {max_a}, max_b = {max_b}, Tb = {Tb}")
        ba, bb = max(1, max_a.bit_length()), max(1, max_b.bit_length())
        return ba, bb, min(64 - ba - bb, max(1, (Tb - 1).bit_length()))

    @staticmethod
    def matching_key(step, a, b, widths) -> np.ndarray:
        """The uint64 keys of ``(step within the launch, ID of A, ID of B)`` under ``widths``:
        ``a << (bits_b + bits_step) | b << bits_step | step``."""
        _, bb, bs = (int(w) for w in widths)
        s, x, y = (np.asarray(v).astype(np.uint64) for v in (step, a, b))
        return (x << np.uint64(bb + bs)) | (y << np.uint64(bs)) | s

    @staticmethod
    def matching_entry_bytes(areas: bool) -> int:
        """The bytes of one table entry of :meth:`event_matching`: key and cells (16), the area (8)."""
        return 16 + (8 if areas else 0)

    def event_matching(self, ids_a: torch.Tensor, ids_b: torch.Tensor, t0: int = 0, q=None, cap: Optional[int] = None) -> Dict[str, object]:
        """The (timestep, event of A, event of B) records of one window of two tracked fields
        (``marex_event_matching_count_i32`` / ``marex_event_matching_i32``): ``ids_a`` and ``ids_b`` int32 ``[Tb, C]`` (a
        cell belongs to event ``ids > 0`` of its field), the rows ``t0 .. t0 + Tb - 1``.  A cell is present where either
        field holds an event; the cells of an event that the other field leaves uncovered are kept under the partner 0.
        ``q`` (int64 ``[C]``, the fixed-point areas of ``regional.area_weight_table``; None: 1 per cell) is a host array or
        a tensor on the engine's device.  ``cap`` overrides the planned table size (tests).

        The key is one 64-bit word whose widths (:meth:`matching_widths`) come from the largest IDs the count pass found;
        a window of more steps than the key's step takes is run as sub-windows of ``2^bits_step`` rows.

        Returns host arrays sorted by ``(a, b, t)``: ``t`` int64 (global steps), ``a`` and ``b`` int32, ``cells`` int64,
        ``area`` int64 (the sum of ``q``, or the cells); and ``runs``, ``cap``, ``table_bytes`` and ``widths``, what the count
        pass found, the table took and the key was laid out with.  A negative ID raises the trackers' "Object IDs must be
        non-negative" error naming the field; a table that the keys do not fit raises :class:`ProcessingError` and leaves the
        engine as it was."""
        Tb, Cn = self._ids_check(ids_a)
        if self._ids_check(ids_b) != (Tb, Cn):
            raise ProcessingError("event_matching: the two ID fields differ in shape",
                                  details=f"ids_a {tuple(ids_a.shape)}, ids_b {tuple(ids_b.shape)}")
        t0 = int(t0)
        if t0 < 0 or Tb == 0 or Cn == 0:
            raise ProcessingError("event_matching: t0 must not be negative and a window must hold at least one step of at least one cell",
                                  details=f"t0 = {t0}, Tb = {Tb}, C = {Cn}")
        from .matching import _no_records  # the front end of this method: it imports the engine only when it runs
        if q is not None and not isinstance(q, torch.Tensor):  # a host vector is checked and uploaded, a tensor is checked
            self._area_q_check("event_matching", q, Cn)
        q_d = self._cell_vector("event_matching", "q", q, torch.int64, Cn, upload=True)
        ar = q_d is not None
        empty = dict(_no_records(), runs=0, cap=0, table_bytes=0, widths=None)
        status = self._buf(None, "mat_status", (8,), torch.int64, self.device)
        self.call("marex_event_matching_count_i32", ids_a, ids_b, Tb, Cn, status)
        s = status.cpu().numpy()
        runs = int(s[2])
        for neg, name in ((int(s[0]), "ID_field_a"), (int(s[1]), "ID_field_b")):
            if neg:
                raise create_data_validation_error("Object IDs must be non-negative",
                                                   details=f"{name}: {neg} negative cells; 0 is background",
                                                   data_info={"field": name, "negative_cells": neg})
        if runs == 0:
            return empty
        widths = self.matching_widths(int(s[3]), int(s[4]), Tb)
        sub = 1 << widths[2]
        planned = self.exposure_cap(runs)
        cap = planned if cap is None else int(cap)
        if cap < 64 or cap & (cap - 1):
            raise ProcessingError(f"event_matching: cap={cap} is not a power of two >= 64")
        per = self.matching_entry_bytes(ar)
        n_out = min(runs, cap)
        nbytes = per * (cap + n_out)
        self._check_fits(nbytes, "event matching", f"a hash table of {cap} entries of {per} bytes for {runs} runs of equal "
                         f"(timestep, event of A, event of B) keys of {widths[0]} + {widths[1]} + {widths[2]} bits, and {n_out} "
                         "compacted entries")
        dev = self.device
        keys, out_k = (self._buf(None, "mat_" + n, (m,), torch.int64, dev) for n, m in (("keys", cap), ("out_keys", n_out)))
        cnt, out_c = (self._buf(None, "mat_" + n, (m,), torch.int64, dev) for n, m in (("cnt", cap), ("out_cnt", n_out)))
        area, out_a = ((self._buf(None, "mat_" + n, (m,), torch.int64, dev) for n, m in (("area", cap), ("out_area", n_out)))
                       if ar else (None, None))
        ba, bb, bs = widths
        parts = []
        for r0 in range(0, Tb, sub):
            r1 = min(Tb, r0 + sub)
            self.call("marex_event_matching_i32", ids_a[r0:r1], ids_b[r0:r1], r1 - r0, Cn, q_d, ba, bb, bs, cap, keys, cnt, area,
                      status, n_out, out_k, out_c, out_a)
            s = status.cpu().numpy()
            n = int(s[7])
            if s[6] != 0:
                raise ProcessingError(f"event_matching: {int(s[6])} cells hold an ID beyond the {ba} and {bb} bits of the key",
                                      details="the widths come from the count pass of the same window: an internal error")
            if s[5] != 0 or not 0 <= n <= n_out:
                raise ProcessingError(f"event_matching: the table of {cap} entries does not hold the keys of {runs} runs",
                                      details=f"{n} entries were taken; a table planned by the engine holds {planned}")
            k = out_k[:n].cpu().numpy().view(np.uint64)
            parts.append((k >> np.uint64(bs), (k & np.uint64((1 << bs) - 1)).astype(np.int64) + (t0 + r0),
                          out_c[:n].cpu().numpy(), out_a[:n].cpu().numpy() if ar else None))
        pair, t, cells, areas = (np.concatenate([p[j] for p in parts]) if parts[0][j] is not None else None for j in range(4))
        if pair.size == 0:
            raise ProcessingError(f"event_matching: no entry for {runs} runs (internal sizing error)")
        order = np.lexsort((t, pair))  # (a, b) is one integer; the sub-windows are in ascending time
        pair, t, cells = pair[order], t[order], cells[order].astype(np.int64)
        return dict(empty, runs=runs, cap=cap, table_bytes=nbytes, widths=widths, t=t,
                    a=(pair >> np.uint64(bb)).astype(np.int32), b=(pair & np.uint64((1 << bb) - 1)).astype(np.int32),
                    cells=cells, area=areas[order] if ar else cells.copy())

    def cell_event_records(self, acc: dict) -> Dict[str, object]:
        """The record buffers of a second pass of :meth:`cell_events`, from the accumulators of a finished summary pass:
        ``off`` int64 ``[C + 1]`` (the exclusive scan of the events per cell, summed over the groups, on the device), ``n``
        and one array per record field, ``[n]`` on the device.  :class:`ProcessingError` with the figures when they do not
        fit."""
        G, Cn, anomalies = acc["plan"][0], acc["plan"][1], acc["plan"][2]
        off = torch.zeros(Cn + 1, dtype=torch.int64, device=self.device)
        torch.cumsum(acc["events"].sum(dim=0, dtype=torch.int64), 0, out=off[1:])
        n = int(off[-1].item())
        per = 8 + (20 if anomalies else 0)
        self._check_fits(per * n, "cell events", f"{n} event records of {per} bytes (start, end"
                         f"{', maximum, its step, float64 sum, invalid steps' if anomalies else ''}) for the second pass")
        alloc = max(n, 1)
        rec = {"off": off, "n": n, "start": self._buf(None, "ce_rstart", (alloc,), torch.int32, self.device),
               "end": self._buf(None, "ce_rend", (alloc,), torch.int32, self.device)}
        if anomalies:
            rec.update(vmax=self._buf(None, "ce_rvmax", (alloc,), torch.int32, self.device),
                       tmax=self._buf(None, "ce_rtmax", (alloc,), torch.int32, self.device),
                       sum=self._buf(None, "ce_rsum", (alloc,), torch.float64, self.device),
                       invalid=self._buf(None, "ce_rinv", (alloc,), torch.int32, self.device))
        return rec

    def cell_events(self, x: torch.Tensor, anom: Optional[torch.Tensor] = None, t0: int = 0, min_duration: int = 5,
                    max_gap: int = 2, grp=None, G: int = 1, mask: Optional[torch.Tensor] = None, records: Optional[dict] = None,
                    acc: Optional[dict] = None, finish: bool = True) -> Dict[str, object]:
        """Per-cell events under the duration and gap rule of the rows ``t0 .. t0 + Tb - 1`` (``marex_cell_events_u8``):
        ``x`` uint8 or bool ``[Tb, C]`` and, optionally, ``anom`` float32 ``[Tb, C]``.  ``grp`` (int ``[T]``, global steps, or
        None with ``G == 1``) labels the steps; an event belongs to the group of its start.  ``mask``: the WHOLE uint8
        ``[T, C]`` output (rows of earlier windows are completed when a run qualifies), or None.  The first window allocates
        the zeroed state and accumulators and uploads the labels; a later window passes the ``"acc"`` entry of the previous
        result -- the window lengths do not matter, not even to the last bit of ``sum``; ``finish`` on the last window
        closes the open events.  Returns ``acc`` and, with ``finish``, ``events``, ``event_days`` and ``duration_max`` uint32
        ``[G, C]`` and with ``anom`` ``sum`` float64, ``vmax`` float32 (NaN: none) and ``invalid`` uint32 ``[G, C]``.
        ``records``: the buffers of :meth:`cell_event_records` make the call the SECOND pass (a fresh ``acc``, no
        accumulators, no mask): the events are written at ``off[c] + k`` and ``finish`` returns ``rec``, the host arrays
        ``off``, ``start``, ``end`` (and ``vmax``, ``tmax``, ``sum``, ``invalid``), beside ``records``, the device buffers.
        An event whose start label lies outside ``0 .. G - 1`` raises :class:`ProcessingError`; it was counted, nothing was
        written out of range."""
        x, Tb, Cn = self._presence_window("cell_events", x)
        if x.dtype != torch.uint8:
            raise ProcessingError("cell_events: the field must be a uint8 or bool mask", details=f"got {x.dtype}")
        if anom is not None:
            self._anomaly_window_check("cell_events", anom, Tb, Cn)
        t0, G, D, gap = int(t0), int(G), int(min_duration), int(max_gap)
        if t0 < 0 or G <= 0 or (grp is None and G != 1) or not 1 <= D <= 2**31 - 1 or not 0 <= gap <= 2**31 - 1:
            raise ProcessingError("cell_events: t0 and max_gap must not be negative, G and min_duration must be positive, and "
                                  "G > 1 needs labels", details=f"t0 = {t0}, G = {G}, labels {'given' if grp is not None else 'missing'}, "
                                                                f"min_duration = {D}, max_gap = {gap}")
        anomalies, second = anom is not None, records is not None
        self._whole_output_check("cell_events", "mask", mask, Cn, t0 + Tb, second)
        plan = (G, Cn, anomalies, D, gap, second)
        if acc is None:
            tabs = label_tables("cell_events", (("grp", grp, None),))
            planes = 10 if anomalies else 4
            per_acc = 0 if second else 12 + (16 if anomalies else 0)
            need = Cn * (4 * planes + (16 if anomalies else 0)) + G * Cn * per_acc + 16 + self._table_bytes(tabs)
            self._check_fits(need, "cell events",
                             f"{Cn} cells of carried state, {4 * planes + (16 if anomalies else 0)} bytes each, {G} x {Cn} cells "
                             f"of accumulators, {per_acc} bytes each, and the label table")
            acc = {"state_i32": self._zeros("ce_sti", (planes, Cn), torch.int32),
                   "state_f64": self._zeros("ce_stf", (2, Cn), torch.float64) if anomalies else None,
                   "status": self._zeros("ce_status", (2,), torch.int64), "plan": plan,
                   **{k: None for k in ("events", "event_days", "duration_max", "sum", "vmax", "invalid")},
                   **self._upload_tables(tabs)}
            if not second:
                for k in ("events", "event_days", "duration_max") + (("vmax", "invalid") if anomalies else ()):
                    acc[k] = self._zeros("ce_" + k, (G, Cn), torch.int32)
                if anomalies:
                    acc["sum"] = self._zeros("ce_sum", (G, Cn), torch.float64)
        self._window_check("cell_events", acc, plan, ("grp",), t0, Tb, Cn)
        if second and (int(records["off"].numel()) != Cn + 1 or ("sum" in records) != anomalies):
            raise ProcessingError("cell_events: the record buffers were planned for another call",
                                  details=f"{int(records['off'].numel()) - 1} cells there, {Cn} here")
        rec = records or {}
        self.call("marex_cell_events_u8", x, anom, t0, Tb, Cn, D, gap, int(bool(finish)), acc["tabs"]["grp"], G,
                  acc["state_i32"], acc["state_f64"], acc["events"], acc["event_days"], acc["duration_max"], acc["sum"],
                  acc["vmax"], acc["invalid"], mask, rec.get("off"), rec.get("start"), rec.get("end"), rec.get("vmax"),
                  rec.get("tmax"), rec.get("sum"), rec.get("invalid"), acc["status"])
        out: Dict[str, object] = {"acc": acc}
        if not finish:
            return out
        bad, over = (int(v) for v in acc["status"].cpu().numpy())
        if bad:
            raise ProcessingError(f"cell_events: {bad} events start under a step label outside its range",
                                  details=f"grp must hold 0 .. {G - 1}; the events were counted, nothing was written out of range")
        if over:
            raise ProcessingError(f"cell_events: {over} events found no room in the records of their cell",
                                  details="the record offsets do not belong to this field; nothing was written out of range")
        host = self._host
        if second:
            n = records["n"]
            r = {"off": records["off"].cpu().numpy(), "start": host(records["start"][:n], np.int32),
                 "end": host(records["end"][:n], np.int32)}
            if anomalies:
                key = host(records["vmax"][:n], np.uint32)
                r.update(vmax=self._key_max(key), tmax=self._key_step(key, host(records["tmax"][:n], np.int32)),
                         sum=host(records["sum"][:n], np.float64), invalid=host(records["invalid"][:n], np.uint32))
            out.update(rec=r, records=records)
            return out
        out.update(events=host(acc["events"], np.uint32), event_days=host(acc["event_days"], np.uint32),
                   duration_max=host(acc["duration_max"], np.uint32))
        if anomalies:
            key = host(acc["vmax"], np.uint32)
            out.update(sum=host(acc["sum"], np.float64), vmax=self._key_max(key),
                       invalid=host(acc["invalid"], np.uint32))
        return out

    def event_rename(self, ids: torch.Tensor, ny: int, nx: int, lut, ev_tmin, ev_tmax,
                     weights: Optional[torch.Tensor] = None) -> Dict[str, np.ndarray]:
        """The device pass of cluster_rename_objects_and_props on a grid (track.py:2897-2976, 3140-3247), in one kernel and
        in place, with compact slots: ``ids`` int32 ``[T, ny * nx]`` -> ``lut[id]`` for ``0 < id < len(lut)``, else 0
        (``lut``: int32 event numbers 0..n_ev).  ``ev_tmin`` / ``ev_tmax`` (int, ``[n_ev + 1]``, entry 0 unused) declare the
        first and last timestep of every event (``tmax < tmin``: absent); event ``e`` owns one slot per step of that span,
        ``off[e] + t - ev_tmin[e]``, with ``off`` (int64 ``[n_ev + 2]``) the exclusive scan of the span lengths.  Returns
        ``off`` and, over the ``off[-1]`` slots, ``mom`` int64 ``[n, 5]`` and ``gid`` int32 ``[n]`` as
        :meth:`event_moments` defines them and, with float32 ``weights`` of a slice, ``wmom`` float64 ``[n, 4]``.  A cell of an
        event outside its declared span is renamed but raises :class:`ProcessingError` (nothing is written out of range)."""
        T, Cn = self._ids_check(ids)
        if Cn != ny * nx:
            raise ProcessingError(f"event_rename: {Cn} cells per slice, ny * nx = {ny * nx}")
        lut_h = np.asarray(lut)
        tmin_h, tmax_h = np.asarray(ev_tmin, dtype=np.int64), np.asarray(ev_tmax, dtype=np.int64)
        n_ev = int(tmin_h.size) - 1
        if lut_h.dtype != np.int32 or lut_h.ndim != 1 or lut_h.size == 0:
            raise ProcessingError("event_rename: the table must be a non-empty int32 vector", details=f"got {lut_h.dtype} {lut_h.shape}")
        if n_ev <= 0 or tmin_h.ndim != 1 or tmax_h.shape != tmin_h.shape or int(lut_h.max()) > n_ev:
            raise ProcessingError("event_rename: ev_tmin and ev_tmax must have one entry per event 0..n_ev, n_ev > 0, and the "
                                  "table must map to those events",
                                  details=f"largest entry {int(lut_h.max())}, spans {tmin_h.shape} / {tmax_h.shape}")
        off = self.event_slot_plan(tmin_h, tmax_h, T)
        n_slots = int(off[-1])
        per = 44 + (32 if weights is not None else 0)
        self._check_fits(per * n_slots + 4 * lut_h.size + 12 * (n_ev + 2), "event properties",
                         f"{n_slots} (timestep, event) slots between each event's first and last timestep, {per} bytes each, "
                         f"and the tables of {lut_h.size} IDs and {n_ev} events")
        alloc = max(n_slots, 1)  # no event has a step: one slot that nothing addresses
        acc = torch.empty((alloc, 5), dtype=torch.int64, device=self.device)
        gid = torch.empty(alloc, dtype=torch.int32, device=self.device)
        wacc = torch.empty((alloc, 4), dtype=torch.float64, device=self.device) if weights is not None else None
        status = torch.empty(1, dtype=torch.int64, device=self.device)
        self.call("marex_event_rename_i32", ids, T, int(ny), int(nx), self._dev(lut_h), lut_h.size, n_ev,
                  self._dev(np.clip(tmin_h, 0, 2**31 - 1).astype(np.int32)), self._dev(off), alloc, weights, acc, wacc, gid, status)
        bad = int(status.item())
        if bad:
            raise ProcessingError(f"event_rename: {bad} cells belong to an event outside its declared span of timesteps",
                                  details="ev_tmin / ev_tmax do not cover the field; the cells were renamed, not accumulated")
        out = {"off": off, "mom": acc[:n_slots].cpu().numpy(), "gid": gid[:n_slots].cpu().numpy()}
        if wacc is not None:
            out["wmom"] = wacc[:n_slots].cpu().numpy()
        return out

    def filter_small_objects(self, data_bin: torch.Tensor, ny: int, nx: int, area_filter_quartile: float = 0.5,
                             area_filter_absolute: Optional[float] = None, regional_mode: bool = False,
                             wsp: Optional[dict] = None) -> Dict[str, object]:
        """Remove the objects smaller than a percentile (or an absolute number) of cells (track.py:1755-1911, gridded).
        Series with more than 2^31 - 2 cells are labelled in time blocks (objects never span timesteps here)."""
        T, Cn = data_bin.shape
        tb = max(1, min(T, (2**31 - 2) // Cn))
        blocks = []
        for i, t0 in enumerate(range(0, T, tb)):
            sub = None if wsp is None else wsp.setdefault(f"ccl{i}", {})
            lab = self.label_objects_2d(data_bin[t0:t0 + tb], ny, nx, wrap_x=not regional_mode, wsp=sub)
            blocks.append((t0, lab["labels"], lab["areas"]))
        per_block = [a.reshape(-1)[a.reshape(-1) > 0] for _, _, a in blocks]  # ordered by (time, first cell)
        obj_areas = torch.cat(per_block)
        n_before = int(obj_areas.numel())
        if n_before == 0:
            raise ProcessingError("No objects found for area-based filtering")
        if area_filter_absolute is not None:
            thr = float(area_filter_absolute)
        else:
            thr = _linear_percentile(obj_areas, area_filter_quartile)
        out = self._buf(wsp, "filtered", tuple(data_bin.shape), torch.uint8, self.device)
        dropped = False  # the reference's `object_ids_keep[0] = -1`: the first object of the whole list is never kept
        n_after = int((obj_areas.to(torch.float64) >= thr).sum().item())
        for (t0, labels, areas), pa in zip(blocks, per_block):
            first = 0
            if not dropped and pa.numel() > 0:
                flat = areas.reshape(-1)
                root = int(torch.nonzero(flat > 0)[0].item())
                first = root + 1
                if float(flat[root].item()) >= thr:
                    n_after -= 1
                dropped = True
            self.call("marex_filter_by_area_u8", labels, areas, labels.numel(), thr, first, out[t0:t0 + labels.shape[0]])
        return {"filtered": out, "area_threshold": thr, "object_areas": obj_areas, "n_before": n_before, "n_after": n_after,
                "labels": blocks[0][1] if len(blocks) == 1 else [b[1] for b in blocks]}

    # ------------------------------------------------------------------ pre-processing in time blocks
    def compact_positive(self, areas: torch.Tensor, out: Optional[torch.Tensor] = None, used: int = 0):
        """The positive entries of an int32 tensor in index order (``marex_compact_positive_i32``): the per-object areas
        that the per-timestep labellings leave at the root cells.  Returns ``(list, count, first_index)``: ``list`` int32
        with the entries at ``[used, used + count)`` -- ``out`` when its room sufficed, else a larger tensor that carries
        ``out[:used]`` over --, ``count`` a host int (the call's one host read) and ``first_index`` an int64 ``[1]`` device
        tensor, the index of the first positive entry or -1."""
        flat = areas.reshape(-1)
        n = int(flat.numel())
        if flat.dtype != torch.int32 or n <= 0 or n > LABEL_BLOCK_CELLS:
            raise ProcessingError("compact_positive: needs a non-empty int32 tensor of at most 2^31 - 2 entries",
                                  details=f"got {flat.dtype} with {n} entries")
        used = int(used)
        if out is None:
            out = torch.empty((max(1024, n // 64),), dtype=torch.int32, device=self.device)
        res = torch.empty((2,), dtype=torch.int64, device=self.device)  # n_out, first_index
        for _ in range(2):
            self._bind_stream()
            tail = out[used:]
            rc = self.lib.marex_compact_positive_i32(self.ctx.handle, flat.data_ptr(), n, tail.data_ptr() if tail.numel() else
                                                     res.data_ptr(), int(tail.numel()), res.data_ptr(), res.data_ptr() + 8)
            if rc != -7:
                break
            count = int(res[0].item())  # the list was too short: grow it (at least doubling) and compact again
            grown = torch.empty((max(2 * int(out.numel()), used + count),), dtype=torch.int32, device=self.device)
            grown[:used] = out[:used]
            out = grown
        self.ctx.check(rc, "marex_compact_positive_i32")
        return out, int(res[0].item()), res[1:2]

    def preprocess_blocked(self, data: Optional[torch.Tensor], mask: torch.Tensor, R_fill: int, T_fill: int, block_steps: int,
                           area_filter_quartile: float = 0.5, area_filter_absolute: Optional[float] = None, *,
                           ny: Optional[int] = None, nx: Optional[int] = None, regional_mode: bool = False,
                           nbr: Optional[torch.Tensor] = None, q: Optional[torch.Tensor] = None, e: int = 0,
                           fetch=None, shape: Optional[Tuple[int, int]] = None, wsp: Optional[dict] = None) -> Dict[str, object]:
        """``fill_holes`` -> ``fill_time_gaps`` -> ``filter_small_objects`` over a ``[T, C]`` uint8 field in blocks of
        ``block_steps`` timesteps: bit for bit the three whole-field calls, at one full-size uint8
        output plus a window of ``block_steps + 2 T_fill`` steps.  Grid form: ``ny``, ``nx`` (and ``regional_mode``); mesh
        form: ``nbr`` int32 ``[3, C]``, the weight table ``q`` and its exponent ``e`` (sizes in cells, the percentile over
        the clusters larger than 50 (5) cells, keep strictly above the threshold, no first-object rule).

        ``data`` is the field on the device; or ``data=None`` with ``shape=(T, C)`` and ``fetch(t0, t1, buf)``, which fills
        the uint8 ``[t1 - t0, C]`` device tensor ``buf`` with the rows ``[t0, t1)`` of a field that lives on the host: only
        one window of it is on the device at a time.

        Returns the dict of :meth:`filter_small_objects` without ``labels``, plus ``raw_area`` and ``processed_area``: the
        cells set in the input and in ``filtered`` (grid), the float64 area-weighted sums over the timesteps (mesh)."""
        mesh = nbr is not None
        T, Cn = (int(k) for k in (data.shape if data is not None else shape))
        if T <= 0 or Cn <= 0:
            raise ProcessingError("preprocess_blocked: empty field", details=f"{T} steps of {Cn} cells")
        if Cn > LABEL_BLOCK_CELLS:
            raise TrackingError(f"one timestep of {Cn} cells exceeds the labelling block of {LABEL_BLOCK_CELLS} cells")
        if not mesh:
            assert Cn == int(ny) * int(nx)
        R, Tf = int(R_fill), int(T_fill)
        B = max(1, min(int(block_steps), T, LABEL_BLOCK_CELLS // Cn))
        W = min(T, B + 2 * Tf)
        wsp = {} if wsp is None else wsp
        dev, u8 = self.device, torch.uint8
        out = self._buf(None, "filtered", (T, Cn), u8, dev)
        # the window buffers at their largest, once: no block allocates
        if data is None:
            self._buf(wsp, "window_in", (W, Cn), u8, dev)
        if Tf > 0:
            self._buf(wsp, "window_filled", (W, Cn), u8, dev)
            self._buf(wsp, "window_closed", (W, Cn), u8, dev)
        self._buf(wsp, "block_labels", (B, Cn), torch.int32, dev)
        self._buf(wsp, "block_areas", (B, Cn), torch.int32, dev)
        wrap = 0 if regional_mode else 1
        absolute = area_filter_absolute is not None

        def holes(src, rows, radius, dst):
            if mesh:
                self.call("marex_fill_holes_mesh_u8", src, mask, nbr, rows, Cn, radius, dst)
            else:
                self.call("marex_fill_holes_u8", src, mask, rows, int(ny), int(nx), radius, int(bool(regional_mode)), dst)

        def label(t0, t1):
            labels = self._buf(wsp, "block_labels", (t1 - t0, Cn), torch.int32, dev)
            areas = self._buf(wsp, "block_areas", (t1 - t0, Cn), torch.int32, dev)
            if mesh:
                self.call("marex_label_mesh_i32", out[t0:t1], mask, nbr, t1 - t0, Cn, labels, areas)
            else:
                self.call("marex_label2d_i32", out[t0:t1], t1 - t0, int(ny), int(nx), wrap, labels, areas)
            return labels, areas

        # areas per timestep, raw and processed: integer sums of the mesh's weights, of unit weights on a grid (the cell
        # count; torch's own sum of a uint8 block would widen it to 8 bytes per cell first)
        if mesh:
            self._mesh_weights_check(q, Cn, "preprocess_blocked")
            weights = q[0]
        else:
            weights = torch.ones((Cn,), dtype=torch.int64, device=dev)
        area_t = torch.zeros((2, T), dtype=torch.int64, device=dev)

        def count_area(which, rows, t0, t1):
            self.call("marex_mesh_area_i64", rows, t1 - t0, Cn, weights, area_t[which, t0:t1])

        def keep(labels, areas, thr, first, t0, t1):  # in place: the kernel reads labels and areas, not the mask
            level = float(np.floor(thr) + 1.0) if mesh else thr  # strict ">" on integer sizes
            self.call("marex_filter_by_area_u8", labels, areas, labels.numel(), level, first, out[t0:t1])
            count_area(1, out[t0:t1], t0, t1)

        blocks = [(t0, min(T, t0 + B)) for t0 in range(0, T, B)]
        lst = torch.empty((1024,), dtype=torch.int32, device=dev)
        n_list = 0
        first = None  # (t0 of the first block with an object, its root's index in the block: int64 [1] on the device)
        thr = float(area_filter_absolute) if absolute else None
        # ---- pass 1: morphology into `out`, per-timestep labelling, the per-object list
        for t0, t1 in blocks:
            w0, w1 = max(0, t0 - Tf), min(T, t1 + Tf)
            if data is not None:
                win = data[w0:w1]
            else:
                win = self._buf(wsp, "window_in", (w1 - w0, Cn), u8, dev)
                fetch(w0, w1, win)
            count_area(0, win[t0 - w0:t1 - w0], t0, t1)
            if Tf > 0:
                a = self._buf(wsp, "window_filled", (w1 - w0, Cn), u8, dev)
                holes(win, w1 - w0, R, a)
                c = self._buf(wsp, "window_closed", (w1 - w0, Cn), u8, dev)
                self.call("marex_time_closing_u8", a, w1 - w0, Cn, Tf, c)
                holes(c[t0 - w0:t1 - w0], t1 - t0, R // 2, out[t0:t1])
            else:
                holes(win, t1 - t0, R, out[t0:t1])
            labels, areas = label(t0, t1)
            lst, cnt, fidx = self.compact_positive(areas, lst, n_list)
            drop = 0
            if cnt and first is None and not mesh:
                first = (t0, fidx.clone())
                if absolute:
                    drop = int(fidx.item()) + 1  # the first object is known when it is met
            n_list += cnt
            if absolute:  # one pass is enough
                keep(labels, areas, thr, drop, t0, t1)
        obj = lst[:n_list]
        if mesh:
            obj = obj[obj > (5 if absolute else 50)]
        n_before = int(obj.numel())
        if n_before == 0:
            raise ProcessingError("No objects found for area-based filtering")
        if not absolute:
            thr = _linear_percentile(obj, area_filter_quartile)
        if mesh:
            n_after = int((obj.to(torch.float64) > thr).sum().item())
        else:
            n_after = int((obj.to(torch.float64) >= thr).sum().item())
            if float(obj[0].item()) >= thr:  # the reference's `object_ids_keep[0] = -1`
                n_after -= 1
        # ---- pass 2 (percentile filter): label the owned rows again and filter them in place
        if not absolute:
            first_t0, first_root = (first[0], int(first[1].item())) if first is not None else (-1, -1)
            for t0, t1 in blocks:
                labels, areas = label(t0, t1)
                keep(labels, areas, thr, first_root + 1 if t0 == first_t0 else 0, t0, t1)
        sums = area_t.cpu().numpy()
        if mesh:  # as mesh_area forms them: S / 2^e per timestep, then the float64 sum over the timesteps
            raw, processed = (float(np.ldexp(v.astype(np.float64), -int(e)).sum()) for v in sums)
        else:
            raw, processed = (float(int(v.sum())) for v in sums)
        return {"filtered": out, "area_threshold": thr, "object_areas": obj, "n_before": n_before, "n_after": n_after,
                "raw_area": raw, "processed_area": processed}

    def fill_holes_mesh(self, data_bin: torch.Tensor, mask: torch.Tensor, nbr: torch.Tensor, R_fill: int,
                        wsp: Optional[dict] = None) -> torch.Tensor:
        """``fill_holes`` on an unstructured mesh (track.py:1543-1606): ``nbr`` int32 ``[3, C]``, 0-based, -1 = none."""
        T, Cn = data_bin.shape
        out = self._buf(wsp, "filled_mesh", (T, Cn), torch.uint8, self.device)
        self.call("marex_fill_holes_mesh_u8", data_bin, mask, nbr, T, Cn, int(R_fill), out)
        return out

    def filter_small_objects_mesh(self, data_bin: torch.Tensor, mask: torch.Tensor, nbr: torch.Tensor,
                                  area_filter_quartile: float = 0.5, area_filter_absolute: Optional[float] = None,
                                  wsp: Optional[dict] = None) -> Dict[str, object]:
        """``filter_small_objects`` on an unstructured mesh (track.py:1776-1857): sizes in cells, percentile over the
        clusters larger than 50 (5) cells, keep STRICTLY larger than the threshold."""
        T, Cn = data_bin.shape
        labels = self._buf(wsp, "labels_mesh", (T, Cn), torch.int32, self.device)
        areas = self._buf(wsp, "areas_mesh", (T, Cn), torch.int32, self.device)
        self.call("marex_label_mesh_i32", data_bin, mask, nbr, T, Cn, labels, areas)
        flat = areas.reshape(-1)
        big = flat[flat > (5 if area_filter_absolute is not None else 50)]
        n_before = int(big.numel())
        if n_before == 0:
            raise ProcessingError("No objects found for area-based filtering")
        if area_filter_absolute is not None:
            thr = float(area_filter_absolute)
        else:
            thr = _linear_percentile(big, area_filter_quartile)
        out = self._buf(wsp, "filtered_mesh", (T, Cn), torch.uint8, self.device)
        # strict ">" : areas are integers, so "> thr" == ">= floor(thr) + 1"
        self.call("marex_filter_by_area_u8", labels, areas, labels.numel(), float(np.floor(thr) + 1.0), 0, out)
        return {"filtered": out, "area_threshold": thr, "object_areas": big, "n_before": n_before,
                "n_after": int((big.to(torch.float64) > thr).sum().item()), "labels": labels}

    def hobday_thresholds_exact(self, anom: torch.Tensor, dcal: DeviceCalendar, percentile: float, wd: int,
                                wsp: Optional[dict] = None) -> torch.Tensor:
        """``np.nanpercentile`` per (dayofyear window, cell), float32, layout ``[366, C]`` (detect.py:1921-1956)."""
        T_out, Cn = anom.shape
        nd = np.diff(dcal.plan.doy_start).astype(np.int64)
        half = int(wd) // 2
        ext = np.concatenate([nd[-half:], nd, nd[:half]]) if half else nd
        max_rows = int(np.convolve(ext, np.ones(wd, dtype=np.int64), mode="valid").max())
        q32 = np.float32(percentile) / np.float32(100)  # NumPy's own float32 quantile
        thr = self._buf(wsp, "thr_doy_major", (N_DOY, Cn), torch.float32, self.device)
        overflow = torch.zeros((1,), dtype=torch.int32, device=self.device)
        self.call("marex_hobday_exact_f32", anom, T_out, Cn, dcal.doy_start, dcal.doy_rows, max(max_rows, 1), float(q32),
                  float(q32), int(wd), thr, overflow)
        if int(overflow.item()) != 0:
            raise ProcessingError("exact Hobday percentile: selection buffer overflow (internal sizing error)")
        return thr

    # ------------------------------------------------------------------ stage a14 global thresholds
    def global_threshold(self, anom: torch.Tensor, percentile: float, method_percentile: str, bins: Optional[BinTable]):
        """Per-cell constant threshold, float64 ``[C]`` (detect.py:2873-2912) + warning statistics."""
        from .binning import global_bins

        T_out, Cn = anom.shape
        thr = torch.empty((Cn,), dtype=torch.float64, device=self.device)
        q = float(percentile) / 100.0
        if method_percentile == "exact":
            self.call("marex_global_threshold_f32", anom, T_out, Cn, q, 1, None, None, 0, 0.0, 0.0, thr, None, None)
            return {"thr_f64": thr, "stats": {"n_too_low": 0, "n_too_high": 0, "min": float("nan"), "max": float("nan")}}
        gb = global_bins(bins.precision, bins.max_anomaly)
        edges = self._dev(gb.edges.astype(np.float64))
        centres = self._dev(gb.centres.astype(np.float64))
        stats = torch.zeros((8,), dtype=torch.int32, device=self.device)
        minmax = torch.tensor([float("inf"), float("-inf")], dtype=torch.float64, device=self.device)
        self.call("marex_global_threshold_f32", anom, T_out, Cn, q, 0, edges, centres, gb.nb, float(gb.lower_bound),
                  float(gb.upper_bound), thr, stats, minmax)
        self.sync()
        s = stats.cpu().numpy().view(np.uint32)
        mm = minmax.cpu().numpy()
        return {
            "thr_f64": thr,
            "stats": {
                "n_too_low": int(s[2]), "n_too_high": int(s[3]),
                "min": float(mm[0]) if np.isfinite(mm[0]) else float("nan"),
                "max": float(mm[1]) if np.isfinite(mm[1]) else float("nan"),
            },
        }

    def mask_ge_const(self, anom: torch.Tensor, thr_f64: torch.Tensor, wsp: Optional[dict] = None) -> Dict[str, torch.Tensor]:
        T_out, Cn = anom.shape
        ext, n_true = self._extreme_buffers(wsp, T_out, Cn)
        self.call("marex_mask_ge_const_f32", anom, thr_f64, T_out, Cn, ext, n_true)
        return {"extreme": ext, "n_true": n_true}

    # ------------------------------------------------------------------ Blosc / LZ4 chunk compression (zarr_io.write_array)
    def blosc_work_bytes(self, nbytes: int, typesize: int, n_chunks: int, blocksize: int = 0, shuffle: int = 1) -> int:
        """Device scratch ``blosc_compress`` needs for ``n_chunks`` chunks of ``nbytes`` bytes (byte planes, encoded
        streams and per-stream integers)."""
        out = C.c_int64(0)
        rc = self.lib.marex_blosc_compress_work_bytes(int(nbytes), int(typesize), int(shuffle), int(blocksize), int(n_chunks),
                                                      C.byref(out))
        if rc != 0:
            raise ProcessingError("marex_blosc_compress_work_bytes failed", details=f"nbytes {nbytes}, typesize {typesize}")
        return int(out.value)

    def blosc_compress(self, chunks: torch.Tensor, typesize: int, blocksize: int = 0, shuffle: int = 1, variant: int = 0,
                       wsp: Optional[dict] = None):
        """Compress every row of ``chunks`` (contiguous uint8 ``[B, nbytes]`` on this device) into a Blosc-1 / LZ4 frame
        byte-identical to ``marex_blosc_compress_h`` with ``dstcap = nbytes + 16``.  Returns ``(frames, lengths)``:
        frames uint8 ``[B, nbytes + 16]`` on the device (row i holds frame i in its first ``lengths[i]`` bytes) and
        lengths int64 NumPy ``[B]`` (synchronises).  ``variant`` 0: one wave per LZ4 stream, 1: one lane per stream."""
        if chunks.dtype != torch.uint8 or chunks.dim() != 2 or not chunks.is_contiguous() or chunks.device != self.device:
            raise ProcessingError("blosc_compress: chunks must be a contiguous uint8 [B, nbytes] tensor on the engine's device",
                                  details=f"got {chunks.dtype} {tuple(chunks.shape)} on {chunks.device}")
        B, nb = (int(k) for k in chunks.shape)
        lengths = np.zeros(B, np.int64)
        if B == 0:
            return torch.empty((0, nb + 16), dtype=torch.uint8, device=self.device), lengths
        wb = self.blosc_work_bytes(nb, typesize, B, blocksize, shuffle)
        work = self._buf(wsp, "blosc_work", (max(wb, 1),), torch.uint8, self.device)
        frames = self._buf(wsp, "blosc_frames", (B, nb + 16), torch.uint8, self.device)
        lens = self._buf(wsp, "blosc_lens", (B,), torch.int64, self.device)
        self.call("marex_blosc_compress_d", chunks, nb, B, int(typesize), int(shuffle), int(blocksize), int(variant), work, wb,
                  frames, lens)
        lengths[:] = lens.cpu().numpy()
        if (lengths < 16).any() or (lengths > nb + 16).any():
            raise ProcessingError("blosc_compress: frame length out of range (internal error)", details=str(lengths[:8]))
        return frames, lengths
