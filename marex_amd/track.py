"""Event tracking on the device: ``marEx.tracker(...).run()`` for gridded data, without merging (marEx/track.py:1162-1232,
1370-1497) and with merging and splitting (track.py:2554-3802; see ``tracker.track_objects``).

The pipeline stays in HBM from the extreme mask to the ID field: ``fill_holes`` -> ``fill_time_gaps`` ->
``filter_small_objects`` -> 26-connected labelling in (time, y, x), periodic in x unless ``regional_mode``
(track.py:2006-2048), then one device-to-host copy of ``ID_field``.  IDs run from 1 to ``N_events_final`` in the order of
each event's first cell in C order.  That is the reference's numbering as read from its code path (dask_image labels
every time block with ``scipy.ndimage.label``, offsets the labels block by block and relabels through
``connected_components``); it has not been run against dask_image itself.
"""
from __future__ import annotations

import logging
from typing import Dict, List, Literal, Optional, Tuple, Union

import numpy as np

from .exceptions import ConfigurationError, ProcessingError, TrackingError, create_data_validation_error
from .track_mesh import _MeshStages, _not_built, mesh_weight_tables  # noqa: F401 -- mesh_weight_tables is public here

logger = logging.getLogger("marex_amd")

#: cells of one labelling call (int32 parents; the limit of the 2-D labeller too) and of a field under merge tracking
MAX_CELLS = 2**31 - 1

#: regionprops names calculate_object_properties computes on the device
SUPPORTED_PROPERTIES = ("label", "area", "centroid")

_I32_MAX = 2**31 - 1

#: ID fields of at least this many bytes come to the host through pinned staging buffers
PINNED_ID_FIELD_BYTES = 256 << 20

#: cells of one labelling block (engine.LABEL_BLOCK_CELLS; repeated here so that this module imports without torch)
_BLOCK_CELLS = 2**31 - 2


def labelling_memory_need(T: int, C: int, max_block_cells: Optional[int] = None, resident: bool = False) -> Dict[str, int]:
    """Bytes of the device buffers ``HotPath.label_objects_3d`` holds for a ``[T, C]`` field, by name: the uint8 mask
    (unless it is ``resident`` already), the int32 ID field, the int32 areas of one call (of the largest block on the
    blocked path) and the library's rank scratch of the same size.  The object-level tables of the blocked path
    (12 bytes per provisional object) are not known before labelling and are left out."""
    n = int(T) * int(C)
    blocked = max_block_cells is not None or n > _BLOCK_CELLS
    limit = _BLOCK_CELLS if max_block_cells is None else min(int(max_block_cells), _BLOCK_CELLS)
    blk = min(n, max(1, limit // int(C)) * int(C)) if blocked else n
    need = {} if resident else {"mask uint8": n}
    need.update({"ID field int32": 4 * n, "areas int32 (one block)": 4 * blk, "rank scratch int32 (one block)": 4 * blk})
    return need


def tracking_memory_need(T: int, ny: int, nx: int, R_fill: int, T_fill: int, resident: bool = False) -> Dict[str, int]:
    """Bytes of the ``[T, C]`` device buffers alive at the peak of ``tracker(allow_merging=False).run()``, by name.  The
    peak is inside ``filter_small_objects`` at the end of ``run_preprocess``: the input mask, the hole-filled mask, the
    gap-filled mask (``T_fill > 0``), the int32 labels and areas of the per-timestep labelling (8 bytes per cell) and the
    filtered mask, torch's temporaries while it selects the non-zero areas of one labelling block (4 bytes per cell of the
    block, as measured: DESIGN.md section 4), plus the library's scratch at its largest -- the bit-packed padded images of
    ``fill_holes`` or the int32 copy of one labelling block.  The labelling that follows holds less (:func:`labelling_memory_need`, with the
    ID field reusing what the pre-processing released: mask + 4 n + 8 bytes per cell of a block against at least 11 n + 4 per
    cell of a block here), so a run that passes this check fits."""
    n = int(T) * int(ny) * int(nx)
    R = int(R_fill)
    packed = 16 * int(T) * (ny + 4 * R) * ((nx + 4 * R + 63) // 64) if R > 0 else 0
    need = {} if resident else {"mask uint8": n}
    need["hole-filled mask uint8"] = n
    if int(T_fill) > 0:
        need["gap-filled mask uint8"] = n
    need.update({"2-D labels int32": 4 * n, "2-D areas int32": 4 * n, "filtered mask uint8": n,
                 "area selection temporaries": 4 * min(n, _BLOCK_CELLS),
                 "library scratch": max(packed, 4 * min(n, _BLOCK_CELLS))})
    return need


#: the name of the input's entry in :func:`preprocess_memory_need` when it is allocated already (not taken from free memory)
_RESIDENT_INPUT = "input mask uint8 (resident, allocated already)"


def preprocess_memory_need(T: int, ny: Optional[int], C: int, R_fill: int, T_fill: int, block_steps: int,
                           resident: bool = False, host_input: bool = False) -> Dict[str, int]:
    """Bytes of the device buffers of the time-blocked pre-processing (``HotPath.preprocess_blocked``)
    of a ``[T, C]`` field in blocks of ``block_steps`` steps, by name; ``ny`` is the grid's row count, None on a mesh.
    The input (one byte per cell; no entry with ``host_input``: only a window of a host array is ever uploaded), the
    full-size uint8 output, three uint8 windows of ``B + 2 T_fill`` steps (the uploaded input, the hole-filled and the
    time-closed rows), the int32 labels and areas of ``B`` steps, the int64 raw and processed areas per timestep (with
    the unit weights that count cells on a grid), and the library's scratch at its largest: the bit-packed
    padded images of ``fill_holes`` over the window (two byte copies of it on a mesh) or the int32 copy of the labelled
    block with the compaction's tile counts.  The per-object list (4 bytes per object) is not known before and left out.
    :func:`preprocess_alloc_bytes` is what of this has yet to be allocated."""
    T, C, R, Tf = int(T), int(C), int(R_fill), int(T_fill)
    B = max(1, min(int(block_steps), T))
    W = min(T, B + 2 * Tf)
    n = T * C
    if ny is None:
        morph = 2 * W * C
    else:
        nx = C // int(ny)
        morph = 16 * W * (int(ny) + 4 * R) * ((nx + 4 * R + 63) // 64) + 256 if R > 0 else 0
    tiles = (B * C + 4095) // 4096
    need = {}
    if not host_input:
        need[_RESIDENT_INPUT if resident else "input mask uint8"] = n
    need["pre-processed mask uint8"] = n
    need["window buffers 3 x uint8"] = 3 * W * C
    need["block labels int32"] = 4 * B * C
    need["block areas int32"] = 4 * B * C
    need["areas per timestep and unit weights int64"] = 16 * T + (8 * C if ny is not None else 0)
    need["library scratch"] = max(morph, 4 * B * C, 4 * (2 * tiles + 1))
    return need


def preprocess_alloc_bytes(need: Dict[str, int]) -> int:
    """The bytes of a :func:`preprocess_memory_need` that come out of the free device memory: all but a resident input."""
    return sum(v for k, v in need.items() if k != _RESIDENT_INPUT)


def plan_preprocess_blocks(T: int, C: int, T_fill: int, free_bytes: int, ny: Optional[int] = None, R_fill: int = 0,
                           resident: bool = False, host_input: bool = False) -> int:
    """The largest number of owned steps ``B`` (at most ``T``, and at most what one labelling call takes: 2^31 - 2 cells)
    whose :func:`preprocess_memory_need`, less a resident input, fits ``free_bytes``.  :class:`TrackingError` with both
    numbers when even one step does not fit.  Needs no GPU."""
    T, C = int(T), int(C)
    if T <= 0 or C <= 0:
        raise TrackingError(f"cannot plan pre-processing blocks for an empty field ({T} steps of {C} cells)")
    if C > _BLOCK_CELLS:
        raise TrackingError(f"one timestep of {C} cells exceeds the labelling block of {_BLOCK_CELLS} cells")
    need = lambda b: preprocess_memory_need(T, ny, C, R_fill, T_fill, b, resident, host_input)  # noqa: E731
    fits = lambda b: preprocess_alloc_bytes(need(b)) <= int(free_bytes)  # noqa: E731
    if not fits(1):
        n1 = need(1)
        raise TrackingError(f"pre-processing in time blocks: one step per block needs {preprocess_alloc_bytes(n1) / 1e9:.3f} GB "
                            f"of device memory, {int(free_bytes) / 1e9:.3f} GB are free",
                            details="; ".join(f"{k} {v / 1e9:.3f} GB" for k, v in n1.items()),
                            suggestions=["Keep the input on the host", "Free device memory held by other arrays"])
    lo, hi = 1, max(1, min(T, _BLOCK_CELLS // C))  # the need grows with B: bisect
    while lo < hi:
        mid = (lo + hi + 1) // 2
        if fits(mid):
            lo = mid
        else:
            hi = mid - 1
    return lo


def merge_memory_need(T: int, ny: int, nx: int, block_steps: int, resident: bool = False, weights: bool = False) -> Dict[str, int]:
    """Bytes of the ``[T, C]`` device buffers alive at the peak of merge tracking with ``merge_block_steps=block_steps``
    (``tracker.track_objects``), by name.  The peak is inside the per-timestep labelling: the
    pre-processed uint8 mask (unless it is ``resident`` already), the int32 ID field, the labelling's scratch of one block
    -- its int32 areas and the library's int32 rank array, 8 bytes per cell of ``min(block_steps, T)`` steps, of at most
    2^31 - 2 cells -- and, with ``weights``, the float32 cell areas of one slice.  Everything after it runs on the ID field
    alone: the merge loop works on two slices, the cluster renaming is in place.

    Not knowable before the run, and therefore not in here: the hash table of the final overlap pass (32 bytes per run of
    equal pairs of one block), the compact (timestep, event) slots of the renaming (44 bytes each, 76 with weights) and
    the per-object tables (about 100 bytes per (timestep, object) slot of the properties, 16 per ID).  Each of them is
    checked against the free device memory where it is allocated."""
    T, C = int(T), int(ny) * int(nx)
    n = T * C
    steps = max(1, min(int(block_steps), T, max(1, _BLOCK_CELLS // C)))
    need = {} if resident else {"pre-processed mask uint8": n}
    need["ID field int32"] = 4 * n
    need["labelling scratch int32 (areas and ranks of one block)"] = 8 * steps * C
    if weights:
        need["cell areas float32 (one slice)"] = 4 * C
    return need


def plan_merge_blocks(T: int, ny: int, nx: int, free_bytes: int, resident: bool = False, weights: bool = False) -> int:
    """The largest ``merge_block_steps`` (at most ``T``, and at most 2^31 - 2 cells a block) whose :func:`merge_memory_need`
    fits ``free_bytes``.  :class:`TrackingError` with both numbers when even one step does not fit.  Needs no GPU."""
    T, C = int(T), int(ny) * int(nx)
    if T <= 0 or C <= 0:
        raise TrackingError(f"cannot plan merge-tracking blocks for an empty field ({T} steps of {C} cells)")
    if C > _BLOCK_CELLS:
        raise TrackingError(f"one timestep of {C} cells exceeds the labelling block of {_BLOCK_CELLS} cells")
    need = lambda b: merge_memory_need(T, ny, nx, b, resident, weights)  # noqa: E731
    fits = lambda b: sum(need(b).values()) <= int(free_bytes)  # noqa: E731
    if not fits(1):
        n1 = need(1)
        raise TrackingError(f"merge tracking in time blocks: one step per block needs {sum(n1.values()) / 1e9:.3f} GB "
                            f"of device memory, {int(free_bytes) / 1e9:.3f} GB are free",
                            details="; ".join(f"{k} {v / 1e9:.3f} GB" for k, v in n1.items()),
                            suggestions=["Track a shorter record", "Free device memory held by other arrays"])
    lo, hi = 1, max(1, min(T, _BLOCK_CELLS // C))  # the need grows with B: bisect
    while lo < hi:
        mid = (lo + hi + 1) // 2
        if fits(mid):
            lo = mid
        else:
            hi = mid - 1
    return lo


def merge_block_pairs(lists) -> np.ndarray:
    """One overlap list out of the lists of consecutive time blocks (each ``(n, 3)`` ``[id at t, id at t + 1, cells]``, the
    blocks sharing one step across every seam, so that every pair of steps is counted in exactly one of them): equal pairs
    are merged and their counts summed -- after merging an ID lives through many steps and meets the same neighbour in
    several blocks -- and the rows come out sorted lexicographically, ``(n, 3)`` int32, as ``HotPath.overlap_pairs`` over the
    whole field gives them.  :class:`ProcessingError` when a sum does not fit int32."""
    rows = [np.asarray(r, dtype=np.int64).reshape(-1, 3) for r in lists if len(r)]
    if not rows:
        return np.zeros((0, 3), np.int32)
    a = np.concatenate(rows)
    k, inv = np.unique((a[:, 0] << 32) | a[:, 1], return_inverse=True)
    c = np.zeros(k.size, np.int64)
    np.add.at(c, inv.reshape(-1), a[:, 2])
    if c.max() > _I32_MAX:
        raise ProcessingError("overlap pairs: a pair overlaps in 2^31 or more cells, which int32 cannot hold",
                              details=f"largest overlap {int(c.max())} cells")
    return np.stack([k >> 32, k & 0xFFFFFFFF, c], axis=1).astype(np.int32)


def _tensor_of(da):
    """The torch tensor behind a device-resident DataArray, else None (never copies)."""
    t = getattr(da, "device_tensor", None)
    if t is not None:
        return t
    d = getattr(da, "data", None)
    if d is not None and type(d).__module__.startswith("torch"):
        return d
    return None


def _host(a) -> np.ndarray:
    t = _tensor_of(a)
    if t is not None:
        return t.cpu().numpy()
    return np.asarray(a.values if hasattr(a, "values") else a)


def _coord_dims(c, default):
    d = getattr(c, "dims", None)
    return tuple(d) if d else default


def _time_chunk_layout(data_bin, dimensions, timechunks) -> Optional[List[int]]:
    """Lengths of the time chunks the merge loop walks (track.py:3379-3382): the time chunk tuple of ``data_bin``
    (``.chunks`` of a Dask-backed DataArray, else the store's regular chunk in ``encoding["chunks"]``), else regular chunks of
    ``timechunks`` counted from t = 0 with the remainder last; None when none of them is known.  A ``timechunks`` that
    disagrees with data_bin's own chunks is ignored with a warning: the merge results follow the chunks the loop walks."""
    timedim = (dimensions or {}).get("time", "time")
    dims = tuple(getattr(data_bin, "dims", ()) or ())
    shape = tuple(getattr(data_bin, "shape", ()) or ())
    if timedim not in dims or len(shape) != len(dims):
        return None
    k = dims.index(timedim)
    T = int(shape[k])
    regular = lambda step: [min(step, T - s) for s in range(0, T, step)]  # noqa: E731
    if timechunks is not None and int(timechunks) <= 0:
        raise ConfigurationError("timechunks must be a positive number of timesteps", details=f"timechunks={timechunks}")
    own = None
    ch = getattr(data_bin, "chunks", None)
    if isinstance(ch, (tuple, list)) and len(ch) == len(dims) and isinstance(ch[k], (tuple, list)):
        c = [int(v) for v in ch[k]]
        if sum(c) == T and all(v > 0 for v in c):
            own = c
    enc = (getattr(data_bin, "encoding", None) or {}).get("chunks")
    if own is None and isinstance(enc, (tuple, list)) and len(enc) == len(dims) and int(enc[k]) > 0:
        own = regular(int(enc[k]))
    if own is not None:
        if timechunks is not None and own != regular(int(timechunks)):
            logger.warning(f"timechunks={int(timechunks)} is ignored: data_bin's own time chunks {tuple(own)} decide the "
                           "merge loop (and its results); rechunk data_bin to change them")
        return own
    return regular(int(timechunks)) if timechunks is not None else None


def _components(n: int, a: np.ndarray, b: np.ndarray) -> np.ndarray:
    """Connected components of nodes 0..n-1 under the edges (a, b): labels 0..N-1 numbered by each component's smallest
    node (scipy's connected_components order): hooking the larger root under the smaller, then pointer jumping."""
    lab = np.arange(n, dtype=np.int64)
    while True:
        ra, rb = lab[a], lab[b]
        hi, lo = np.maximum(ra, rb), np.minimum(ra, rb)
        ch = hi != lo
        if not ch.any():
            break
        np.minimum.at(lab, hi[ch], lo[ch])
        while True:
            nxt = lab[lab]
            if np.array_equal(nxt, lab):
                break
            lab = nxt
    roots = np.unique(lab)
    return np.searchsorted(roots, lab)


class _Props:
    """Area and centroid of the live object IDs, indexed densely by ID (the reference's object_props Dataset)."""

    def __init__(self, ids, area, cy, cx):
        n = int(ids.max()) + 1 if len(ids) else 1
        self.area = np.zeros(n)
        self.cy = np.zeros(n)
        self.cx = np.zeros(n)
        self.alive = np.zeros(n, dtype=bool)
        self.set(ids, area, cy, cx)

    def _grow(self, hi: int) -> None:
        if hi < self.alive.size:
            return
        n = max(hi + 1, 2 * self.alive.size)
        for k in ("area", "cy", "cx", "alive"):
            a = getattr(self, k)
            b = np.zeros(n, dtype=a.dtype)
            b[:a.size] = a
            setattr(self, k, b)

    def set(self, ids, area, cy, cx) -> None:
        ids = np.asarray(ids, dtype=np.int64)
        if ids.size:
            self._grow(int(ids.max()))
            self.area[ids], self.cy[ids], self.cx[ids] = area, cy, cx
            self.alive[ids] = True

    def has(self, i) -> np.ndarray:
        i = np.asarray(i, dtype=np.int64)
        ok = (i >= 0) & (i < self.alive.size)
        return ok & self.alive[np.where(ok, i, 0)]

    def ids(self) -> np.ndarray:
        return np.nonzero(self.alive)[0]

    def max_id(self) -> int:
        i = self.ids()
        return int(i[-1]) if i.size else 0

    def dataset(self):
        from .xr_compat import DataArray, Dataset

        i = self.ids()
        coord = {"ID": ("ID", i.astype(np.int64))}
        return Dataset({"area": DataArray(self.area[i], dims=("ID",), coords=coord),
                        "centroid": DataArray(np.stack([self.cy[i], self.cx[i]]), dims=("component", "ID"), coords=coord)},
                       coords=coord)

    @classmethod
    def of(cls, object_props) -> "_Props":
        if isinstance(object_props, _Props):
            return object_props
        ids = np.asarray(object_props["ID"].values, dtype=np.int64)
        c = np.asarray(object_props["centroid"].values, dtype=np.float64)
        return cls(ids, np.asarray(object_props["area"].values, dtype=np.float64), c[0], c[1])


class tracker(_MeshStages):  # noqa: N801 -- the reference's public name (marEx.tracker)
    """Identify extreme events as connected regions in (time, y, x) of a binary field on a grid; on an unstructured mesh,
    the merge tracker from the pre-processing to the events.

    The constructor takes the reference's arguments (track.py:323-348).  Supported here: gridded data, with
    ``allow_merging=False`` (the reference's "basic" tracker) and with ``allow_merging=True`` (the default: merging and
    splitting, centroid or ``nn_partitioning``).  Merge results depend on the time chunks the per-timestep loop walks: they
    are taken from ``data_bin.chunks`` (Dask), from ``data_bin.encoding["chunks"]`` (a store's chunks) or from the
    ``timechunks`` keyword (regular chunks from t = 0); with none of them ``allow_merging=True`` raises
    :class:`ConfigurationError`.  ``checkpoint="save"`` / ``"load"`` raise too.

    Unstructured meshes (``unstructured_grid=True``, marex_amd/track_mesh.py).  ``data_bin`` is ``(time, x)`` (transposed if
    given the other way), ``mask`` ``(x,)``, lat / lon coordinates over ``x``, ``neighbours`` ``("nv", x)`` with 3 rows of
    1-based cell numbers (0: none) and ``cell_areas`` over ``x``; without the last two the constructor raises
    :class:`ConfigurationError`, ``regional_mode=True`` raises ``NotImplementedError`` and ``grid_resolution`` is refused, as
    in the reference.  Built on a mesh, on the device: :meth:`run_preprocess`, :meth:`compute_area`,
    :meth:`identify_objects` (IDs restart at 1 in every timestep, in scipy's ``connected_components`` order),
    :meth:`unique_ids_in_time`, :meth:`calculate_object_properties` (float32 area in the units of ``cell_areas``, float32
    centroid (lat, lon) in degrees on the sphere), :meth:`check_overlap_slice` / :meth:`find_overlapping_objects`
    (``(n, 3)`` float32 ``[id, id, overlap area]``), :meth:`enforce_overlap_threshold` and
    :meth:`split_and_merge_objects_parallel` (the reference's merge algorithm for meshes: it walks the time chunks of
    ``data_bin`` or of ``timechunks=``, no chunk of one step, and raises :class:`TrackingError` after ``max_iteration``
    iterations), :meth:`cluster_rename_objects_and_props` (events with float32 area and centroid on the sphere per
    timestep) and, over them, :meth:`track_objects`, :meth:`run_tracking` (always through :meth:`track_objects`, as in the
    reference) and :meth:`run`.  Areas are integer sums of the fixed-point weights of :func:`mesh_weight_tables`: bitwise
    reproducible, and within the rounding bound of the reference's float32 sums.  The constructor needs no time chunking
    on a mesh, but every stage from split-and-merge on does: without one, :meth:`run`, :meth:`run_tracking`,
    :meth:`track_objects` and :meth:`cluster_rename_objects_and_props` raise :class:`ConfigurationError` before any device
    work.  :meth:`split_and_merge_objects` and :meth:`consolidate_object_ids` are the gridded algorithm and raise
    :class:`ConfigurationError` on a mesh.  ``temp_dir`` is not required (nothing is written to disk).

    ``grid_resolution`` and ``cell_areas`` weight the final area and centroid of merge tracking (object properties count
    cells, as the reference's do, track.py:1499-1518, 2337).  Accepted and ignored: ``temp_dir``,
    ``max_iteration`` on grids (the gridded algorithm walks the timesteps once), ``debug``, ``verbose`` and ``quiet``
    (logging).  ``coordinate_units`` is resolved as the reference does (track.py:919-976) when merging; the basic tracker
    carries the input's lat / lon unchanged.

    The stages of the reference's merge tracker are public methods here too (track.py:1499-1518, 2050-3802):
    :meth:`compute_area`, :meth:`calculate_centroid`, :meth:`calculate_object_properties`, :meth:`check_overlap_slice`,
    :meth:`find_overlapping_objects`, :meth:`enforce_overlap_threshold`, :meth:`consolidate_object_ids`,
    :meth:`split_and_merge_objects`, :meth:`cluster_rename_objects_and_props` and :meth:`track_objects`, on the device.

    Size limits.  One labelling call takes fewer than 2^31 - 1 cells; a longer record is labelled in blocks of timesteps
    of at most 2^31 - 2 cells each, and the objects are joined across the seams on the device, so that ``ID_field`` is what
    one labelling of the whole field would give.  ``label_block_steps`` forces the block length in timesteps (for tests,
    and for less scratch memory: the labelling's work buffers have the size of one block).  This holds for
    ``allow_merging=False`` and :meth:`identify_objects`.  :class:`TrackingError` is raised for a single timestep of
    2^31 - 1 cells or more, for more than 2^31 - 2 objects before the seams are joined, when the buffers of the run
    (:func:`tracking_memory_need`, about 12 bytes per cell) exceed the free device memory -- before anything is allocated,
    with both numbers -- and by merge tracking (``allow_merging=True``) for fields of 2^31 - 1 cells and more unless
    ``merge_block_steps`` is given.

    ``preprocess_block_steps`` (None: the whole-field path above) runs :meth:`run_preprocess` in time blocks of that many
    steps, or with ``"auto"`` of as many as the free device memory takes: the same mask and statistics, at the input, the
    output and a window of ``B + 2 T_fill`` steps (:func:`preprocess_memory_need`, about 2 bytes per cell); a host
    ``data_bin`` is then uploaded one window at a time.  :meth:`run` checks the larger of that and
    :func:`labelling_memory_need` instead.  On grids and on meshes.

    ``merge_block_steps`` (None: merge tracking refuses fields of 2^31 - 1 cells and more, as above) lifts that limit for
    ``allow_merging=True`` on grids: with a number of timesteps ``B``, or with ``"auto"`` the largest ``B`` that the free
    device memory takes, :meth:`run` and :meth:`track_objects` label the objects and collect the final overlap pairs in
    time blocks of at most ``B`` steps and 2^31 - 2 cells; every other pass addresses the field with 64-bit offsets and
    stays whole.  The results do not depend on ``B``.  :meth:`run` then checks the larger of the pre-processing's need and
    :func:`merge_memory_need` (the mask, the int32 ID field and 8 bytes per cell of one block) against the free device
    memory; a single timestep of 2^31 - 1 cells or more stays refused.  Composes with ``preprocess_block_steps``.

    ``data_bin`` may be device resident -- a DataArray whose data is a torch tensor (bool or uint8) on the GPU, e.g. from
    ``zarr_io.open_dataarray_device`` -- and is then consumed without a host round trip.  ``device`` picks the GPU.
    """

    def __init__(
        self,
        data_bin,
        mask,
        R_fill: Union[int, float],
        area_filter_quartile: Optional[float] = None,
        area_filter_absolute: Optional[int] = None,
        temp_dir: Optional[str] = None,
        T_fill: int = 2,
        allow_merging: bool = True,
        nn_partitioning: bool = False,
        overlap_threshold: float = 0.5,
        unstructured_grid: bool = False,
        dimensions: Optional[Dict[str, str]] = None,
        coordinates: Optional[Dict[str, str]] = None,
        neighbours=None,
        cell_areas=None,
        grid_resolution: Optional[float] = None,
        max_iteration: int = 40,
        checkpoint: Optional[Literal["save", "load", "None"]] = None,
        debug: int = 0,
        verbose: Optional[bool] = None,
        quiet: Optional[bool] = None,
        regional_mode: bool = False,
        coordinate_units: Optional[Literal["degrees", "radians"]] = None,
        device: int = 0,
        timechunks: Optional[int] = None,
        label_block_steps: Optional[int] = None,
        preprocess_block_steps: Union[int, str, None] = None,
        merge_block_steps: Union[int, str, None] = None,
    ) -> None:
        supported = "gridded data without checkpointing"
        pbs = preprocess_block_steps
        if pbs is not None and pbs != "auto" and (isinstance(pbs, (bool, str)) or not isinstance(pbs, (int, np.integer)) or pbs <= 0):
            raise ConfigurationError("preprocess_block_steps must be a positive number of timesteps, 'auto' or None",
                                     details=f"preprocess_block_steps={pbs!r}")
        self.preprocess_block_steps = pbs if pbs is None or isinstance(pbs, str) else int(pbs)
        if label_block_steps is not None and (isinstance(label_block_steps, bool) or not isinstance(label_block_steps, (int, np.integer))
                                              or label_block_steps <= 0):
            raise ConfigurationError("label_block_steps must be a positive number of timesteps",
                                     details=f"label_block_steps={label_block_steps!r}")
        self.label_block_steps = None if label_block_steps is None else int(label_block_steps)
        mbs = merge_block_steps
        if mbs is not None and mbs != "auto" and (isinstance(mbs, (bool, str)) or not isinstance(mbs, (int, np.integer)) or mbs <= 0):
            raise ConfigurationError("merge_block_steps must be a positive number of timesteps, 'auto' or None",
                                     details=f"merge_block_steps={mbs!r}")
        if mbs is not None and (unstructured_grid or not allow_merging):
            raise ConfigurationError("merge_block_steps is for merge tracking on grids (allow_merging=True, unstructured_grid=False)",
                                     details="the basic tracker and the mesh tracker take fields of any length already",
                                     suggestions=["Pass merge_block_steps=None"])
        self.merge_block_steps = mbs if mbs is None or isinstance(mbs, str) else int(mbs)
        self._time_chunks = None
        if allow_merging and not unstructured_grid:
            # merge results depend on the time chunks the per-timestep loop walks (track.py:3379-3382, 3602-3615)
            self._time_chunks = _time_chunk_layout(data_bin, dimensions, timechunks)
            if self._time_chunks is None:
                raise ConfigurationError("allow_merging=True is not supported without a time chunking of data_bin",
                                         details="the reference refuses unchunked input (track.py:411-418), and merges "
                                                 "depend on the time chunks",
                                         suggestions=["Pass timechunks=<steps per chunk>", "Chunk data_bin in time",
                                                      "Pass allow_merging=False"])
        if unstructured_grid:
            # split_and_merge_objects_parallel walks these chunks; a mesh tracker without a known chunking still constructs
            self._time_chunks = _time_chunk_layout(data_bin, dimensions, timechunks)
            self._init_mesh(data_bin, mask, R_fill, area_filter_quartile, area_filter_absolute, T_fill, allow_merging,
                            nn_partitioning, overlap_threshold, dimensions, coordinates, neighbours, cell_areas, grid_resolution,
                            max_iteration, checkpoint, regional_mode, coordinate_units, device)
            return
        if checkpoint in ("save", "load"):
            raise ConfigurationError(f"checkpoint={checkpoint!r} is not supported by the device tracker",
                                     details=f"supported: {supported}; the pipeline stays in device memory",
                                     suggestions=["Pass checkpoint=None"])

        self.data_bin = data_bin
        self.mask = mask
        self.regional_mode = bool(regional_mode)
        self.device = device
        dimensions = dimensions or {}
        self.timedim = dimensions.get("time", "time")
        self.xdim = dimensions.get("x", "lon")
        self.ydim = dimensions.get("y", "lat")
        coordinates = coordinates or {}
        self.timecoord = coordinates.get("time", self.timedim)
        self.xcoord = coordinates.get("x", self.xdim)
        self.ycoord = coordinates.get("y", self.ydim)
        self.R_fill = int(R_fill)
        self.T_fill = T_fill
        self._resolve_area_filtering_parameters(area_filter_quartile, area_filter_absolute)
        self.allow_merging = allow_merging
        self.nn_partitioning = bool(nn_partitioning)
        self.overlap_threshold = overlap_threshold
        self.unstructured_grid = unstructured_grid
        self.checkpoint = checkpoint
        self.data_attrs = dict(getattr(data_bin, "attrs", None) or {})
        self._validate_inputs(cell_areas, grid_resolution)
        self.lat_init = data_bin.coords[self.ycoord]
        self.lon_init = data_bin.coords[self.xcoord]
        self.time_values = np.asarray(data_bin.coords[self.timecoord].values)
        self.coordinate_units = coordinate_units
        if self.allow_merging:
            self._unify_coordinates()
            self._cell_weights = self._merge_cell_weights(cell_areas, grid_resolution)

    # ------------------------------------------------------------------ validation (track.py:493-749)
    def _resolve_area_filtering_parameters(self, area_filter_quartile, area_filter_absolute) -> None:
        given = sum(v is not None for v in (area_filter_quartile, area_filter_absolute))
        if given == 0:
            self.area_filter_quartile, self.area_filter_absolute, self._use_absolute_filtering = 0.5, 0, False
        elif given == 1:
            if area_filter_quartile is not None:
                self.area_filter_quartile, self.area_filter_absolute, self._use_absolute_filtering = area_filter_quartile, 0, False
            else:
                self.area_filter_quartile, self.area_filter_absolute, self._use_absolute_filtering = 0.0, area_filter_absolute, True
        else:
            raise ConfigurationError(
                "Cannot specify both area filtering parameters",
                details="area_filter_quartile and area_filter_absolute are mutually exclusive",
                suggestions=["Use area_filter_quartile for percentile-based filtering (e.g., 0.25 for smallest 25%)",
                             "Use area_filter_absolute for fixed minimum area (e.g., 10 for minimum 10 cells)",
                             "Omit both parameters to use default quartile filtering (0.5)"],
                context={"area_filter_quartile": area_filter_quartile, "area_filter_absolute": area_filter_absolute},
            )

    def _validate_inputs(self, cell_areas, grid_resolution) -> None:
        d = self.data_bin
        want = (self.timedim, self.ydim, self.xdim)
        dims = tuple(getattr(d, "dims", ()))
        if dims != want and (len(dims) != 3 or set(dims) != set(want)):
            raise create_data_validation_error(
                "Invalid dimensions for gridded data",
                details=f"Expected 3D array with dimensions {want}, got {list(dims)}",
                suggestions=["Ensure data has time, latitude, and longitude dimensions",
                             "Check dimension mapping and coordinate names"],
                data_info={"actual_dims": list(dims), "expected_dims": list(want)},
            )
        self._perm = tuple(dims.index(k) for k in want)  # the reference transposes to (time, y, x) (track.py:525-527)
        coords = getattr(d, "coords", {})
        if self.timecoord not in coords or self.xcoord not in coords or self.ycoord not in coords:
            raise create_data_validation_error(  # the reference's wording, grids included (track.py:551-553)
                "Missing required coordinates in unstructured data",
                details=f"Expected coordinates ({self.timecoord}, {self.xcoord}, {self.ycoord}), but found {list(coords)}",
                suggestions=["Ensure data_bin contains time, x, and y coordinates",
                             "Specify coordinates in the tracker initialisation with `coordinates` parameter."],
            )
        t = _tensor_of(d)
        dt = str(t.dtype).replace("torch.", "") if t is not None else str(np.asarray(d.values).dtype)
        if dt != "bool" and not (t is not None and dt == "uint8"):  # a device mask may also be 0 / 1 bytes
            raise create_data_validation_error(
                "Input DataArray must be binary (boolean type)",
                details=f"Found dtype {dt}, expected bool",
                suggestions=["Convert data using da > threshold for binary events"],
                data_info={"actual_dtype": dt, "expected_dtype": "bool"},
            )
        if cell_areas is not None and set(getattr(cell_areas, "dims", ())) != {self.ydim, self.xdim}:
            raise create_data_validation_error(
                "Invalid cell_areas dimensions for structured grid",
                details=f"Expected spatial dimensions {{{self.ydim!r}, {self.xdim!r}}}, got {set(getattr(cell_areas, 'dims', ()))}",
                suggestions=["Ensure cell_areas matches the spatial dimensions of your data"],
            )
        if grid_resolution is not None and (isinstance(grid_resolution, bool) or not isinstance(grid_resolution, (int, float))
                                            or grid_resolution <= 0):
            raise create_data_validation_error(
                "grid_resolution must be a positive number",
                details=f"Received grid_resolution={grid_resolution}",
                suggestions=["Provide a positive float value representing grid resolution in degrees"],
            )
        m = _host(self.mask)
        if m.dtype != bool:
            raise create_data_validation_error(
                "Mask must be binary (boolean type)",
                details=f"Found mask dtype {m.dtype}, expected bool",
                suggestions=["Convert mask using mask > 0 or mask.astype(bool)"],
                data_info={"mask_dtype": str(m.dtype)},
            )
        if not m.any():
            raise create_data_validation_error(
                "Mask contains only False values",
                details="Mask should indicate valid regions with True values",
                suggestions=["Check mask orientation - it should mark valid (ocean) regions as True"],
            )
        if tuple(getattr(self.mask, "dims", ())) == (self.xdim, self.ydim):
            m = m.T
        ny, nx = d.shape[self._perm[1]], d.shape[self._perm[2]]
        if m.shape != (ny, nx):
            raise create_data_validation_error("Mask shape does not match the spatial shape of data_bin",
                                               details=f"mask {m.shape}, data ({ny}, {nx})")
        self._mask_host = np.ascontiguousarray(m)
        if not self._use_absolute_filtering:
            if self.area_filter_quartile < 0 or self.area_filter_quartile > 1:
                raise ConfigurationError(
                    "Invalid area_filter_quartile value",
                    details=f"Value {self.area_filter_quartile} is outside valid range [0, 1]",
                    suggestions=["Use values between 0.0 and 1.0"],
                    context={"provided_value": self.area_filter_quartile, "valid_range": [0, 1]},
                )
        elif self.area_filter_absolute <= 0:
            raise ConfigurationError(
                "Invalid area_filter_absolute value",
                details=f"area_filter_absolute={self.area_filter_absolute} must be positive",
                suggestions=["Set area_filter_absolute to a positive integer (e.g., 5, 10, 50)"],
                context={"area_filter_absolute": self.area_filter_absolute},
            )
        if self.T_fill % 2 != 0:
            raise ConfigurationError(
                "T_fill must be even for temporal symmetry",
                details=f"Provided T_fill={self.T_fill} is odd",
                suggestions=["Use even values: 2, 4, 6, 8, etc."],
                context={"provided_value": self.T_fill, "requirement": "even number"},
            )
        if self.R_fill < 0 or self.R_fill > 63:
            raise ConfigurationError("R_fill must be between 0 and 63 on the device path", details=f"R_fill={self.R_fill}")

    @staticmethod
    def _check_size(shape) -> None:
        n = int(np.prod([int(k) for k in shape]))
        if n >= MAX_CELLS:
            raise TrackingError("more than 2^31 - 1 cells: merge tracking (allow_merging=True) is not built for such fields",
                                details=f"{n} cells: its dense (timestep, object) tables and slice tables are int32-indexed; "
                                        "allow_merging=False and identify_objects label such a field in time blocks")

    def _perm_of(self, da):
        """Axis order that brings ``da`` to (time, y, x), as :meth:`_device_u8` applies it."""
        dims = tuple(getattr(da, "dims", self._out_dims()))
        return tuple(dims.index(k) for k in self._out_dims()) if set(dims) == set(self._out_dims()) else (0, 1, 2)

    @staticmethod
    def _free_bytes(eng) -> int:
        """What the driver reports free plus what torch's allocator holds cached."""
        import torch

        free, _ = torch.cuda.mem_get_info(eng.device)
        return int(free + torch.cuda.memory_reserved(eng.device) - torch.cuda.memory_allocated(eng.device))

    @staticmethod
    def _check_fits(eng, need: Dict[str, int], what: str, suggestions: Optional[List[str]] = None) -> None:
        """:class:`TrackingError` with both numbers when the ``[T, C]`` buffers of ``need`` (name -> bytes) exceed the free
        device memory -- what the driver reports free plus what torch's allocator holds cached -- instead of a torch
        out-of-memory error half way through."""
        import torch

        free, _ = torch.cuda.mem_get_info(eng.device)
        free += torch.cuda.memory_reserved(eng.device) - torch.cuda.memory_allocated(eng.device)
        total = sum(need.values())
        if total > free:
            raise TrackingError(f"{what}: needs {total / 1e9:.3f} GB of device memory, {free / 1e9:.3f} GB are free",
                                details="; ".join(f"{k} {v / 1e9:.3f} GB" for k, v in need.items()),
                                suggestions=["Track a shorter record", "Free device memory held by other arrays"]
                                + list(suggestions or []))

    def _preprocess_plan(self, eng, T: int, ny: Optional[int], C: int, resident: bool) -> Tuple[int, Dict[str, int]]:
        """``(B, need)`` of the blocked pre-processing: ``preprocess_block_steps`` as given, or with ``"auto"`` the largest
        block that fits fifteen sixteenths of the free device memory (the rest is left to the per-object list, the small
        tables and the allocator's rounding)."""
        if self.preprocess_block_steps == "auto":
            free = self._free_bytes(eng)
            B = plan_preprocess_blocks(T, C, self.T_fill, free - free // 16, ny=ny, R_fill=self.R_fill, resident=resident,
                                       host_input=not resident)
        else:
            B = min(int(self.preprocess_block_steps), T, max(1, _BLOCK_CELLS // C))
        return B, preprocess_memory_need(T, ny, C, self.R_fill, self.T_fill, B, resident=resident, host_input=not resident)

    def _check_memory(self, shape) -> None:
        """The basic tracker's buffers at their peak against the free device memory."""
        T, ny, nx = (int(shape[k]) for k in self._perm)
        resident = _tensor_of(self.data_bin) is not None
        if self.preprocess_block_steps is not None:
            # blocked pre-processing: its own need, or the labelling that follows it (the pre-processed mask + the ID field)
            eng = self._engine()
            _, pre = self._preprocess_plan(eng, T, ny, ny * nx, resident)
            pre = {k: v for k, v in pre.items() if k != _RESIDENT_INPUT}
            block = None if self.label_block_steps is None else self.label_block_steps * ny * nx
            lab = labelling_memory_need(T, ny * nx, block, resident=False)
            self._check_fits(eng, pre if sum(pre.values()) >= sum(lab.values()) else lab, "tracker.run")
            return
        need = tracking_memory_need(T, ny, nx, self.R_fill, self.T_fill, resident=resident)
        self._check_fits(self._engine(), need, "tracker.run", suggestions=["Pass preprocess_block_steps='auto'"])

    def _merge_plan(self, eng, T: int, ny: int, nx: int, resident: bool) -> Tuple[int, Dict[str, int]]:
        """``(B, need)`` of merge tracking in time blocks: ``merge_block_steps`` as given, or with ``"auto"`` the largest
        block that fits fifteen sixteenths of the free device memory (the rule of :meth:`_preprocess_plan`); never more
        than 2^31 - 2 cells a block.  A single slice of 2^31 - 1 cells or more stays refused."""
        C = ny * nx
        if C > _BLOCK_CELLS:
            raise TrackingError(f"one timestep of {C} cells exceeds the labelling block of {_BLOCK_CELLS} cells",
                                details="merge tracking in time blocks needs a single slice below 2^31 - 1 cells")
        weights = self._cell_weights is not None
        if self.merge_block_steps == "auto":
            free = self._free_bytes(eng)
            B = plan_merge_blocks(T, ny, nx, free - free // 16, resident=resident, weights=weights)
        else:
            B = min(int(self.merge_block_steps), T, max(1, _BLOCK_CELLS // C))
        return B, merge_memory_need(T, ny, nx, B, resident=resident, weights=weights)

    def _check_merge_memory(self, shape) -> None:
        """Merge tracking with ``merge_block_steps``: the larger of the pre-processing's buffers and of
        :func:`merge_memory_need` against the free device memory, before any device work."""
        T, ny, nx = (int(shape[k]) for k in self._perm)
        resident = _tensor_of(self.data_bin) is not None
        eng = self._engine()
        if self.preprocess_block_steps is not None:
            _, pre = self._preprocess_plan(eng, T, ny, ny * nx, resident)
            pre = {k: v for k, v in pre.items() if k != _RESIDENT_INPUT}
        else:
            pre = tracking_memory_need(T, ny, nx, self.R_fill, self.T_fill, resident=resident)
        _, mrg = self._merge_plan(eng, T, ny, nx, resident=False)
        self._check_fits(eng, pre if sum(pre.values()) >= sum(mrg.values()) else mrg, "tracker.run",
                         suggestions=[] if self.preprocess_block_steps is not None else ["Pass preprocess_block_steps='auto'"])

    @staticmethod
    def _ids_to_host(eng, ids) -> np.ndarray:
        """The int32 ``[T, C]`` ID field as a NumPy array; a large one goes through the engine's pinned staging buffers
        (marex_amd/transfer.py) instead of one pageable copy."""
        if ids.numel() * 4 < PINNED_ID_FIELD_BYTES:
            return ids.cpu().numpy()
        from .detect import _pipe

        out = np.empty(tuple(ids.shape), dtype=np.int32)
        eng.sync()
        _pipe(eng).download(ids, out)
        return out

    # ------------------------------------------------------------------ device plumbing
    def _engine(self):
        from .detect import get_engine

        return get_engine(self.device)

    def _device_u8(self, da, eng):
        """``da`` as a contiguous uint8 ``[T, ny * nx]`` device tensor in (time, y, x) order; device data is not copied
        to the host, bool tensors are reinterpreted in place."""
        import torch

        t = _tensor_of(da)
        dims = tuple(getattr(da, "dims", self._out_dims()))
        perm = tuple(dims.index(k) for k in self._out_dims()) if set(dims) == set(self._out_dims()) else (0, 1, 2)
        if t is None:
            a = np.asarray(da.values)
            if perm != (0, 1, 2):
                a = np.transpose(a, perm)
            t = torch.from_numpy(np.ascontiguousarray(a).astype(np.uint8)).to(eng.device)
        else:
            if t.device != eng.device:
                t = t.to(eng.device)
            if perm != (0, 1, 2):
                t = t.permute(*perm)
            t = t.contiguous()
            t = t.view(torch.uint8) if t.dtype == torch.bool else t
        T = t.shape[0]
        return t.reshape(T, -1), T, t.shape[1], t.shape[2]

    def _out_dims(self):
        return (self.timedim, self.ydim, self.xdim)

    def _wrap_device(self, t, T, ny, nx, name):
        from .zarr_io import DeviceDataArray

        return DeviceDataArray(t.reshape(T, ny, nx), self._out_dims(), {self.timedim: self.time_values}, name=name)

    # ------------------------------------------------------------------ pipeline (track.py:1162-1497)
    def run(self, return_merges: bool = False, checkpoint: Optional[str] = None):
        """``run_preprocess`` -> ``run_tracking`` -> ``run_stats_attributes``; returns the events Dataset, and with
        ``return_merges`` and merging also the merge events: ``(events_ds, merges_ds)`` (track.py:1162-1232)."""
        if self.unstructured_grid:
            self._mesh_need_chunks("tracker.run")
            self._mesh_merge_chunks()  # a chunk of one step is refused before the pre-processing, not after it
        if self.unstructured_grid or (self.allow_merging and self.merge_block_steps is None):
            self._check_size(self.data_bin.shape)
        elif self.allow_merging:
            self._check_merge_memory(self.data_bin.shape)
        else:
            self._check_memory(self.data_bin.shape)
        data_bin_preprocessed, object_stats = self.run_preprocess(checkpoint=checkpoint)
        events_ds, merges_ds, N_events_final = self.run_tracking(data_bin_preprocessed)
        events_ds = self.run_stats_attributes(events_ds, merges_ds, object_stats, N_events_final)
        if return_merges and self.allow_merging:
            return events_ds, merges_ds
        return events_ds

    def run_preprocess(self, checkpoint: Optional[str] = None) -> Tuple[object, Tuple[float, int, int, float, float, float]]:
        """Fill holes, fill time gaps and remove small objects (track.py:1234-1368), on the device.  Returns the filtered
        mask as a device-resident DataArray and ``(total_area_IDed, N_objects_prefiltered, N_objects_filtered,
        area_threshold, accepted_area_fraction, preprocessed_area_fraction)``, areas in cells.  On a mesh: the mesh forms of
        the same stages, sizes in cells, ``preprocessed_area_fraction`` from the area-weighted :meth:`compute_area`."""
        import torch

        from .track_pre import _preprocess_device

        if checkpoint in ("save", "load"):
            raise ConfigurationError(f"checkpoint={checkpoint!r} is not supported by the device tracker")
        if self.unstructured_grid:
            return self._mesh_run_preprocess()
        eng = self._engine()
        absolute = float(self.area_filter_absolute) if self._use_absolute_filtering else None
        if self.preprocess_block_steps is not None:
            from .track_pre import _preprocess_blocked_device

            T, ny, nx = (int(self.data_bin.shape[k]) for k in self._perm_of(self.data_bin))
            mk = torch.from_numpy(self._mask_host.reshape(-1).astype(np.uint8)).to(eng.device)
            if _tensor_of(self.data_bin) is not None:
                x, host = self._device_u8(self.data_bin, eng)[0], None
            else:  # stays on the host: the blocks upload their windows
                x, host = None, np.asarray(self.data_bin.values)
                if self._perm_of(self.data_bin) != (0, 1, 2):
                    host = np.transpose(host, self._perm_of(self.data_bin))
            B, _ = self._preprocess_plan(eng, T, ny, ny * nx, resident=x is not None)
            filtered, stats = _preprocess_blocked_device(eng, x, host, mk, ny, nx, self.R_fill, self.T_fill,
                                                         self.area_filter_quartile, absolute, self.regional_mode, B)
            return self._wrap_device(filtered, T, ny, nx, "data_bin_preproc"), stats
        x, T, ny, nx = self._device_u8(self.data_bin, eng)
        mk = torch.from_numpy(self._mask_host.reshape(-1).astype(np.uint8)).to(eng.device)
        filtered, stats = _preprocess_device(eng, x, mk, ny, nx, self.R_fill, self.T_fill, self.area_filter_quartile, absolute,
                                             self.regional_mode)
        return self._wrap_device(filtered, T, ny, nx, "data_bin_preproc"), stats

    def identify_objects(self, data_bin, time_connectivity: bool):
        """Connected regions of ``data_bin`` (track.py:1912-2048, structured grid): 26-connected in (time, y, x) with
        ``time_connectivity``, else 8-connected per timestep; periodic in x unless ``regional_mode``.  Returns
        ``(ID_field int32, None, N_objects)``; IDs 1..N by first cell in C order, unique across time either way.  On a mesh
        (track.py:1932-2005): components over the listed edges per timestep, land excluded, ``time_connectivity=True``
        refused; IDs restart at 1 in every timestep, ranked by each component's smallest cell, and the third value is the
        reference's placeholder 1 (see :meth:`unique_ids_in_time`)."""
        from .xr_compat import DataArray

        if self.unstructured_grid:
            return self._mesh_identify_objects(data_bin, time_connectivity)
        eng = self._engine()
        T, ny, nx = (int(data_bin.shape[k]) for k in self._perm_of(data_bin))
        block = None if self.label_block_steps is None else self.label_block_steps * ny * nx
        need = labelling_memory_need(T, ny * nx, block, resident=_tensor_of(data_bin) is not None)
        self._check_fits(eng, need, "identify_objects")
        x, T, ny, nx = self._device_u8(data_bin, eng)
        r = eng.label_objects_3d(x, ny, nx, wrap_x=not self.regional_mode, connect_t=bool(time_connectivity),
                                 max_block_cells=block)
        ids = self._ids_to_host(eng, r["ids"]).reshape(T, ny, nx)
        N = int(r["n"].item())
        da = DataArray(ids, dims=self._out_dims(), coords={self.timedim: (self.timedim, self.time_values)}, name="ID_field")
        return da, None, N

    def run_tracking(self, data_bin_preprocessed):
        """Events without merging (track.py:1370-1412): ``identify_objects(time_connectivity=True)``; the time
        coordinate gets its own name back when it differs from the time dimension."""
        from .xr_compat import DataArray, Dataset

        if self.unstructured_grid:
            self._mesh_need_chunks("tracker.run_tracking")
        if self.allow_merging or self.unstructured_grid:  # track.py:1388-1390
            return self.track_objects(data_bin_preprocessed)
        ids, _, N_events_final = self.identify_objects(data_bin_preprocessed, time_connectivity=True)
        # IDs are >= 0 by construction (the reference's `where(ID_field > 0, other=0)` is a no-op here)
        da = DataArray(ids.values, dims=self._out_dims(), coords={self.timecoord: (self.timedim, self.time_values)},
                       name="ID_field")
        return Dataset({"ID_field": da}), Dataset(), N_events_final

    def run_stats_attributes(self, events_ds, merges_ds, object_stats, N_events_final: int):
        """Attributes and the printed summary of track.py:1414-1493, then the input's attrs and its lat / lon."""
        total_area_IDed, N_objects_prefiltered, N_objects_filtered, area_threshold, accepted_area_fraction, \
            preprocessed_area_fraction = object_stats
        at = events_ds.attrs
        at["allow_merging"] = int(self.allow_merging)
        at["N_objects_prefiltered"] = int(N_objects_prefiltered)
        at["N_objects_filtered"] = int(N_objects_filtered)
        at["N_events_final"] = int(N_events_final)
        at["R_fill"] = self.R_fill
        at["T_fill"] = self.T_fill
        at["area_filter_quartile"] = self.area_filter_quartile
        at["area_threshold (cells)"] = area_threshold
        at["accepted_area_fraction"] = accepted_area_fraction
        at["preprocessed_area_fraction"] = preprocessed_area_fraction
        if self.allow_merging:  # track.py:1477-1484 (the attrs are set before the summary is printed here)
            at["overlap_threshold"] = self.overlap_threshold
            at["nn_partitioning"] = int(self.nn_partitioning)
            at["total_merges"] = int(len(merges_ds["n_parents"].values))
            at["multi_parent_merges"] = int((np.asarray(merges_ds["n_parents"].values) > 2).sum())
        print("Tracking Statistics:")
        print(f"   Binary Hobday to Processed Area Fraction: {preprocessed_area_fraction}")
        print(f"   Total Object Area IDed (cells): {total_area_IDed}")
        print(f"   Number of Initial Pre-Filtered Objects: {N_objects_prefiltered}")
        print(f"   Number of Final Filtered Objects: {N_objects_filtered}")
        print(f"   Area Cutoff Threshold (cells): {int(area_threshold)}")
        print(f"   Accepted Area Fraction: {accepted_area_fraction}")
        print(f"   Total Events Tracked: {N_events_final}")
        if self.allow_merging:
            print(f"   Total Merging Events Recorded: {at['total_merges']}")
        at.update(self.data_attrs)
        return self._remap_coordinates(events_ds)

    def event_intensity(self, events_ds, dat_anomaly, per_timestep: bool = True, block_steps: Union[int, str, None] = None):
        """The events Dataset of :meth:`run` with the intensity of every event added
        (:func:`marex_amd.intensity.event_intensity` has the variables): ``events_ds["ID_field"]`` joined with
        ``dat_anomaly`` (float, same dimensions in the same order; host or device resident) on this tracker's device, under
        its time names and its area weights -- on a grid the float32 cell areas of the merge tracker's area pass (unit
        weights without ``cell_areas`` / ``grid_resolution``), on a mesh the float32 ``cell_areas``.  Returns a new Dataset;
        ``events_ds`` is not changed.  The ``ID`` axis and ``presence`` of a merge tracker's Dataset are checked against
        what the pass found (:class:`ProcessingError`)."""
        from .intensity import _event_intensity
        from .xr_compat import Dataset

        w = np.asarray(self.cell_area, np.float32) if self.unstructured_grid else getattr(self, "_cell_weights", None)
        n = int(np.asarray(events_ds["ID"].values).size) if "ID" in events_ds else None
        out = _event_intensity(events_ds["ID_field"], dat_anomaly, w, per_timestep, block_steps, self.device, n_events=n,
                               time=(self.timedim, self.timecoord, self.time_values))
        if n is not None and not np.array_equal(np.asarray(out["ID"].values), np.asarray(events_ds["ID"].values)):
            raise ProcessingError("event_intensity: the events of the ID field are not those of the events Dataset",
                                  details=f"IDs 1..{int(np.asarray(out['ID'].values).size)} found, the Dataset lists {n}")
        if "presence" in events_ds:
            dur = np.asarray(events_ds["presence"].values).sum(axis=0)
            if not np.array_equal(dur, np.asarray(out["event_duration"].values)):
                k = int(np.argmax(dur != np.asarray(out["event_duration"].values)))
                raise ProcessingError("event_intensity: an event's duration differs from its presence in the events Dataset",
                                      details=f"event {k + 1}: {int(np.asarray(out['event_duration'].values)[k])} steps in the ID "
                                              f"field, present in {int(dur[k])}")
        data = dict(events_ds.data_vars)
        data.update(out.data_vars)
        ds = Dataset(data)
        ds.attrs.update(events_ds.attrs)
        return ds

    def event_categories(self, events_ds, extremes_ds, thresholds=None, per_timestep: bool = False, return_field: bool = False,
                         block_steps: Union[int, str, None] = None):
        """The events Dataset of :meth:`run` with the severity categories of every event added
        (:func:`marex_amd.event_categories.event_categories` has the variables): ``events_ds["ID_field"]`` joined with
        ``extremes_ds["dat_anomaly"]`` and, unless ``thresholds`` is passed, ``extremes_ds["thresholds"]`` (the Dataset of
        ``preprocess_data``), on this tracker's device, under its time names and with the area weights
        :meth:`event_intensity` takes.  Returns a new Dataset; ``events_ds`` is not changed.  The ``ID`` axis of a merge
        tracker's Dataset is checked against what the pass found (:class:`ProcessingError`)."""
        from .event_categories import _event_categories
        from .xr_compat import Dataset

        w = np.asarray(self.cell_area, np.float32) if self.unstructured_grid else getattr(self, "_cell_weights", None)
        n = int(np.asarray(events_ds["ID"].values).size) if "ID" in events_ds else None
        thr = extremes_ds["thresholds"] if thresholds is None else thresholds
        out = _event_categories(events_ds["ID_field"], extremes_ds["dat_anomaly"], thr, w, per_timestep, return_field,
                                block_steps, self.device, n_events=n, time=(self.timedim, self.timecoord, self.time_values))
        if n is not None and not np.array_equal(np.asarray(out["ID"].values), np.asarray(events_ds["ID"].values)):
            raise ProcessingError("event_categories: the events of the ID field are not those of the events Dataset",
                                  details=f"IDs 1..{int(np.asarray(out['ID'].values).size)} found, the Dataset lists {n}")
        data = dict(events_ds.data_vars)
        data.update(out.data_vars)
        ds = Dataset(data)
        ds.attrs.update(events_ds.attrs)
        return ds

    def event_occurrence(self, events_ds, **kw):
        """Occurrence statistics of the events of :meth:`run` (:func:`marex_amd.occurrence.event_occurrence` has the
        arguments and the variables) from ``events_ds["ID_field"]``, on this tracker's device.  On a mesh ``lat`` defaults
        to the tracker's own latitudes (degrees), so that ``zonal=True`` needs ``lat_bins`` only."""
        from .occurrence import event_occurrence

        kw.setdefault("device", self.device)
        if self.unstructured_grid and kw.get("zonal") and kw.get("lat") is None:
            lat = getattr(self, "lat", None)
            kw["lat"] = np.asarray(lat if lat is not None else _host(self.lat_init))
        return event_occurrence(events_ds["ID_field"], **kw)

    def local_intensity(self, events_or_field, extremes_ds, **kw):
        """Per-cell intensity and severity categories (:func:`marex_amd.local_intensity.local_intensity` has the arguments
        and the variables) on this tracker's device: ``events_or_field`` is the events Dataset of :meth:`run` (its
        ``ID_field`` is taken) or a presence field such as ``extremes_ds["extreme_events"]``; ``dat_anomaly`` and, unless
        ``thresholds`` is passed, ``thresholds`` come from ``extremes_ds``, the Dataset of ``preprocess_data``.  On a mesh
        ``lat`` defaults to the tracker's own latitudes (degrees), so that ``zonal=True`` needs ``lat_bins`` only."""
        from .local_intensity import local_intensity

        kw.setdefault("device", self.device)
        if "thresholds" not in kw and "thresholds" in extremes_ds:
            kw["thresholds"] = extremes_ds["thresholds"]
        if self.unstructured_grid and kw.get("zonal") and kw.get("lat") is None:
            lat = getattr(self, "lat", None)
            kw["lat"] = np.asarray(lat if lat is not None else _host(self.lat_init))
        field = events_or_field["ID_field"] if hasattr(events_or_field, "data_vars") else events_or_field
        return local_intensity(field, extremes_ds["dat_anomaly"], **kw)

    def event_composites(self, events_or_field, values, **kw):
        """Lagged composites of ``values`` around event onsets or ends
        (:func:`marex_amd.composites.event_composites` has the arguments and the variables) on this tracker's device:
        ``events_or_field`` is the events Dataset of :meth:`run` (its ``ID_field`` is taken) or a presence field such as
        ``extremes_ds["extreme_events"]``."""
        from .composites import event_composites

        kw.setdefault("device", self.device)
        field = events_or_field["ID_field"] if hasattr(events_or_field, "data_vars") else events_or_field
        return event_composites(field, values, **kw)

    def event_shapes(self, events_ds, **kw):
        """Shape and movement of the events of :meth:`run` (:func:`marex_amd.shapes.event_shapes` has the arguments and the
        variables) from ``events_ds["ID_field"]``, on this tracker's device and under its time names.  Unless passed:
        ``mask`` is the tracker's mask, ``regional_mode`` its own, ``cell_areas`` the float32 cell areas of the merge
        tracker's area pass (cells without them) and ``lat`` / ``lon`` the 1-D coordinates of the tracked field in degrees,
        so that the path of the centroid comes in km.  The ``ID`` axis of a merge tracker's Dataset is checked against what
        the pass found (:class:`ProcessingError`).  On a mesh tracker this is
        :func:`marex_amd.shapes_mesh.mesh_event_shapes` (its variables and definitions) with the tracker's neighbours,
        ``lat`` / ``lon`` in degrees, ``cell_areas`` and mask; ``edge_lengths``, ``radius_km``, ``per_timestep`` and
        ``block_steps`` may be passed."""
        from .shapes import _event_shapes

        field = events_ds["ID_field"] if hasattr(events_ds, "data_vars") else events_ds
        n = int(np.asarray(events_ds["ID"].values).size) if hasattr(events_ds, "data_vars") and "ID" in events_ds else None
        if self.unstructured_grid:
            from .shapes_mesh import _mesh_event_shapes

            args = {k: kw.pop(k, d) for k, d in (("cell_areas", self.cell_area), ("edge_lengths", None), ("mask", self._mask_host),
                                                 ("radius_km", 6371.0), ("per_timestep", True), ("block_steps", None),
                                                 ("device", self.device))}
            if kw:
                raise TypeError(f"event_shapes() got an unexpected keyword argument {next(iter(kw))!r}")
            return _mesh_event_shapes(field, self._nbr_host, np.asarray(self.lat), np.asarray(self.lon), args["cell_areas"],
                                      args["edge_lengths"], args["mask"], args["radius_km"], args["per_timestep"],
                                      args["block_steps"], args["device"], zero_based=True, n_events=n,
                                      time=(self.timedim, self.timecoord, self.time_values))
        if "mask" not in kw:
            m = getattr(self, "_mask_host", None)
            kw["mask"] = m if m is not None else getattr(self, "mask", None)
        kw.setdefault("regional_mode", bool(self.regional_mode))
        if "cell_areas" not in kw:
            kw["cell_areas"] = getattr(self, "_cell_weights", None)
        if "lat" not in kw and "lon" not in kw and len(field.shape) == 3:
            la, lo = np.asarray(_host(self.lat_init)), np.asarray(_host(self.lon_init))
            if la.shape == (int(field.shape[1]),) and lo.shape == (int(field.shape[2]),):
                kw["lat"], kw["lon"] = la, lo
        args = {k: kw.pop(k, d) for k, d in (("mask", None), ("cell_areas", None), ("edge_lengths", None), ("lat", None),
                                             ("lon", None), ("regional_mode", False), ("per_timestep", True),
                                             ("block_steps", None), ("device", self.device))}
        if kw:
            raise TypeError(f"event_shapes() got an unexpected keyword argument {next(iter(kw))!r}")
        return _event_shapes(field, args["mask"], args["cell_areas"], args["edge_lengths"], args["lat"], args["lon"],
                             args["regional_mode"], args["per_timestep"], args["block_steps"], args["device"], n_events=n,
                             time=(self.timedim, self.timecoord, self.time_values))

    def regional_series(self, events_or_field, extremes_ds=None, regions=None, **kw):
        """Area, intensity and severity categories per region and timestep
        (:func:`marex_amd.regional.regional_series` has the arguments and the variables) on this tracker's device:
        ``events_or_field`` is the events Dataset of :meth:`run` (its ``ID_field`` is taken) or a presence field such as
        ``extremes_ds["extreme_events"]``.  With ``extremes_ds``, the Dataset of ``preprocess_data``, ``dat_anomaly`` and,
        unless ``thresholds`` is passed, ``thresholds`` come from it.  The time dimension and coordinate of the result are
        the tracker's.  Unless passed, ``mask`` is the tracker's mask and ``cell_areas`` its areas: on a mesh its
        ``cell_areas``; on a grid the float32 cell areas of the merge tracker's area pass, which exist only with
        ``allow_merging=True`` and ``cell_areas`` or ``grid_resolution`` -- a grid tracker built with
        ``allow_merging=False``, like one built without areas, gives ``area`` in cells (as :meth:`event_intensity`
        weighs by cells then): pass ``cell_areas=`` here for areas."""
        from .regional import _regional_series

        kw.setdefault("device", self.device)
        if extremes_ds is not None:
            kw.setdefault("dat_anomaly", extremes_ds["dat_anomaly"])
            if "thresholds" not in kw and "thresholds" in extremes_ds:
                kw["thresholds"] = extremes_ds["thresholds"]
        if "mask" not in kw:
            m = getattr(self, "_mask_host", None)
            kw["mask"] = m if m is not None else getattr(self, "mask", None)
        if "cell_areas" not in kw:
            kw["cell_areas"] = np.asarray(_host(self.cell_area)) if self.unstructured_grid else getattr(self, "_cell_weights", None)
        field = events_or_field["ID_field"] if hasattr(events_or_field, "data_vars") else events_or_field
        args = {k: kw.pop(k, None) for k in ("cell_areas", "dat_anomaly", "thresholds", "mask", "by", "event_id", "block_steps",
                                             "device")}
        if kw:
            raise TypeError(f"regional_series() got an unexpected keyword argument {next(iter(kw))!r}")
        return _regional_series(field, regions, time=(self.timedim, self.timecoord, self.time_values), **args)

    def event_exposure(self, events_ds, regions, extremes_ds=None, **kw):
        """Which events of :meth:`run` touched which region, when and how
        (:func:`marex_amd.exposure.event_exposure` has the arguments and the variables) from ``events_ds["ID_field"]``, on
        this tracker's device and with its time values.  With ``extremes_ds``, the Dataset of ``preprocess_data``,
        ``dat_anomaly`` comes from it.  Unless passed, ``mask`` is the tracker's mask and ``cell_areas`` its areas, as in
        :meth:`regional_series`.  The ``ID`` axis of a merge tracker's Dataset is checked against what the pass found
        (:class:`ProcessingError`)."""
        from .exposure import _event_exposure

        kw.setdefault("device", self.device)
        if extremes_ds is not None:
            kw.setdefault("dat_anomaly", extremes_ds["dat_anomaly"])
        if "mask" not in kw:
            m = getattr(self, "_mask_host", None)
            kw["mask"] = m if m is not None else getattr(self, "mask", None)
        if "cell_areas" not in kw:
            kw["cell_areas"] = np.asarray(_host(self.cell_area)) if self.unstructured_grid else getattr(self, "_cell_weights", None)
        is_ds = hasattr(events_ds, "data_vars")
        field = events_ds["ID_field"] if is_ds else events_ds
        args = {k: kw.pop(k, d) for k, d in (("cell_areas", None), ("dat_anomaly", None), ("mask", None), ("per_timestep", False),
                                             ("block_steps", None), ("device", None))}
        if kw:
            raise TypeError(f"event_exposure() got an unexpected keyword argument {next(iter(kw))!r}")
        n = int(np.asarray(events_ds["ID"].values).size) if is_ds and "ID" in events_ds else None
        if n is not None and not np.array_equal(np.asarray(events_ds["ID"].values), np.arange(1, n + 1)):
            raise ProcessingError("event_exposure: the ID axis of the events Dataset is not 1 .. N",
                                  details=f"{n} IDs from {np.asarray(events_ds['ID'].values)[:1]}")
        return _event_exposure(field, regions, time=(self.timedim, self.timecoord, self.time_values), n_events=n, **args)

    def event_matching(self, events_ds, other, **kw):
        """Which events of :meth:`run` are which events of a second tracking of the same cells
        (:func:`marex_amd.matching.event_matching` has the arguments and the variables): ``events_ds["ID_field"]`` is field
        A; ``other``, an events Dataset with ``ID_field`` or a bare field, is field B.  On this tracker's device and with
        its time values, on grids and on meshes.  Unless passed, ``cell_areas`` are the tracker's areas, as in
        :meth:`regional_series`.  The ``ID`` axes of the Datasets, where they exist, give ``Na`` and ``Nb`` and are checked
        against what the pass found (:class:`ProcessingError`)."""
        from .matching import _event_matching

        kw.setdefault("device", self.device)
        if "cell_areas" not in kw:
            kw["cell_areas"] = np.asarray(_host(self.cell_area)) if self.unstructured_grid else getattr(self, "_cell_weights", None)
        args = {k: kw.pop(k, d) for k, d in (("cell_areas", None), ("min_share", 0.0), ("per_timestep", False),
                                             ("block_steps", None), ("device", None))}
        if kw:
            raise TypeError(f"event_matching() got an unexpected keyword argument {next(iter(kw))!r}")
        fields, n = [], []
        for ds, name in ((events_ds, "events"), (other, "other")):
            is_ds = hasattr(ds, "data_vars")
            fields.append(ds["ID_field"] if is_ds else ds)
            n.append(int(np.asarray(ds["ID"].values).size) if is_ds and "ID" in ds else None)
            if n[-1] is not None and not np.array_equal(np.asarray(ds["ID"].values), np.arange(1, n[-1] + 1)):
                raise ProcessingError(f"event_matching: the ID axis of the {name} Dataset is not 1 .. N",
                                      details=f"{n[-1]} IDs from {np.asarray(ds['ID'].values)[:1]}")
        return _event_matching(fields[0], fields[1], time=(self.timedim, self.timecoord, self.time_values), n_events_a=n[0],
                               n_events_b=n[1], **args)

    def _latlon_coords(self) -> dict:
        """The input's lat / lon as coordinate entries ``name -> (dims, host values)``."""
        ydim = self.xdim if self.unstructured_grid else self.ydim  # on a mesh lat runs over the cells too
        return {self.ycoord: (_coord_dims(self.lat_init, (ydim,)), _host(self.lat_init)),
                self.xcoord: (_coord_dims(self.lon_init, (self.xdim,)), _host(self.lon_init))}

    def _remap_coordinates(self, events_ds):
        """Re-assign the input's lat / lon coordinates (track.py:978-983)."""
        from .xr_compat import DataArray, Dataset

        if "centroid" in events_ds.data_vars:
            return self._remap_merge_coordinates(events_ds)
        v = events_ds["ID_field"]
        coords = {self.timecoord: (self.timedim, self.time_values), **self._latlon_coords()}
        out = Dataset({"ID_field": DataArray(v.values, dims=tuple(v.dims), coords=coords, name="ID_field")})
        out.attrs.update(events_ds.attrs)
        return out

    # ------------------------------------------------------------------ object properties and overlaps (track.py:1499-1518, 2050-2552)
    def compute_area(self, data_bin):
        """Cells of ``data_bin`` per timestep (track.py:1499-1518, gridded: ``data_bin.sum(dim=[y, x])``), an int64
        DataArray over time.  ``data_bin`` may be device resident.  On a mesh: the area of the cells set per timestep
        (``(data_bin * cell_area).sum(x)``), float64, from integer sums of the fixed-point cell areas on the device."""
        import torch

        from .xr_compat import DataArray

        if self.unstructured_grid:
            return self._mesh_compute_area(data_bin)
        dims = tuple(getattr(data_bin, "dims", ()) or ())
        if not dims:
            dims = self._out_dims() if len(data_bin.shape) == 3 else (self.ydim, self.xdim)
        axes = tuple(i for i, d in enumerate(dims) if d in (self.ydim, self.xdim))
        t = _tensor_of(data_bin)
        if t is not None:
            area = t.to(torch.int64).sum(dim=axes).cpu().numpy()
        else:
            area = np.asarray(data_bin.values if hasattr(data_bin, "values") else data_bin).sum(axis=axes, dtype=np.int64)
        rest = tuple(d for d in dims if d not in (self.ydim, self.xdim))
        coords = {}
        c = getattr(data_bin, "coords", None) or {}
        if self.timedim in rest and self.timecoord in c:
            coords[self.timecoord] = (self.timedim, np.asarray(c[self.timecoord].values))
        return DataArray(area, dims=rest, coords=coords)

    def calculate_centroid(self, binary_mask, original_centroid: Optional[Tuple[float, float]] = None) -> Tuple[float, float]:
        """Centroid ``(y, x)`` of one object's 2-D mask (track.py:2050-2107), in cell indices.  Unless ``regional_mode``, an
        object with a cell in the first 100 columns and one in the last 100 (the two bands overlap when nx < 200) gets the
        mean of its columns with those right of ``nx // 2`` shifted by ``-nx``, plus ``nx`` if that mean is negative.
        Otherwise ``original_centroid`` is returned as given or, when it is None, the plain means are computed (the
        reference returns None in regional mode without an ``original_centroid``)."""
        m = np.asarray(binary_mask).astype(bool)
        if self.regional_mode:
            if original_centroid is not None:
                return original_centroid
            ys, xs = np.nonzero(m)
            return (np.mean(ys), np.mean(xs))
        near_left_BC = np.any(m[:, :100])
        near_right_BC = np.any(m[:, -100:])
        y_centroid = np.mean(np.nonzero(m)[0]) if original_centroid is None else original_centroid[0]
        if near_left_BC and near_right_BC:
            x = np.nonzero(m)[1]
            x_adj = x.copy()
            x_adj[x > m.shape[1] // 2] -= m.shape[1]
            x_centroid = np.mean(x_adj)
            if x_centroid < 0:
                x_centroid += m.shape[1]
        elif original_centroid is None:
            x_centroid = np.mean(np.nonzero(m)[1])
        else:
            x_centroid = original_centroid[1]
        return (y_centroid, x_centroid)

    def _ids_perm(self, field):
        """Axis order that brings an ID field to (time, y, x), or (y, x) for a single slice."""
        nd = len(field.shape)
        dims = getattr(field, "dims", None)
        want = self._out_dims() if nd == 3 else (self.ydim, self.xdim)
        if dims is not None and len(dims) > 0:
            dims = tuple(dims)
            if nd not in (2, 3) or set(dims) != set(want) or len(dims) != nd:
                raise create_data_validation_error(
                    "Invalid dimensions for an object ID field",
                    details=f"Expected dimensions {self._out_dims()} or {(self.ydim, self.xdim)}, got {list(dims)}",
                    data_info={"actual_dims": list(dims)})
            return tuple(dims.index(k) for k in want)
        if nd not in (2, 3):
            raise create_data_validation_error("Invalid dimensions for an object ID field",
                                               details=f"Expected a 3-D (time, y, x) or 2-D (y, x) array, got shape {tuple(field.shape)}")
        return tuple(range(nd))

    @staticmethod
    def _id_range_error(lo, hi):
        if lo < 0:
            return create_data_validation_error("Object IDs must be non-negative", details=f"smallest ID {lo}; 0 is background",
                                                data_info={"min_id": int(lo), "max_id": int(hi)})
        return create_data_validation_error("Object IDs must fit int32", details=f"largest ID {hi} > {_I32_MAX}",
                                            data_info={"min_id": int(lo), "max_id": int(hi)})

    def _device_ids(self, field, eng):
        """An ID field as a contiguous int32 ``[T, ny * nx]`` device tensor in (time, y, x) order (a 2-D field is one
        slice): ``(tensor, T, ny, nx)``.  An int32 device tensor is used in place; other integer types are range-checked
        and converted."""
        import torch

        perm = self._ids_perm(field)
        t = _tensor_of(field)
        if t is None:
            a = np.asarray(field.values if hasattr(field, "values") else field)
            if a.dtype.kind not in "iu":
                raise create_data_validation_error("Object IDs must be integers", details=f"Found dtype {a.dtype}",
                                                   data_info={"actual_dtype": str(a.dtype)})
            if a.dtype != np.int32 and a.size:
                lo, hi = int(a.min()), int(a.max())
                if lo < 0 or hi > _I32_MAX:
                    raise self._id_range_error(lo, hi)
            t = torch.from_numpy(np.ascontiguousarray(np.transpose(a, perm), dtype=np.int32)).to(eng.device)
        else:
            if t.dtype.is_floating_point or t.dtype.is_complex or t.dtype == torch.bool:
                raise create_data_validation_error("Object IDs must be integers", details=f"Found dtype {t.dtype}",
                                                   data_info={"actual_dtype": str(t.dtype)})
            if t.device != eng.device:
                t = t.to(eng.device)
            if t.dtype != torch.int32 and t.numel():
                lo, hi = int(t.min().item()), int(t.max().item())
                if lo < 0 or hi > _I32_MAX:
                    raise self._id_range_error(lo, hi)
                t = t.to(torch.int32)
            t = t.permute(*perm).contiguous()
        if t.dim() == 2:
            t = t.unsqueeze(0)
        T, ny, nx = (int(k) for k in t.shape)
        return t.reshape(T, ny * nx), T, ny, nx

    def calculate_object_properties(self, object_id_field, properties: Optional[List[str]] = None):
        """Properties of the objects of an ID field (track.py:2109-2390, gridded branch), computed on the device.

        ``properties`` defaults to ``["label", "area"]``; ``"label"`` is always added; ``"area"`` and ``"centroid"`` are
        the other supported names.  Returns a Dataset indexed by ``ID`` (int64): per timeslice in time order, the IDs
        present in that slice in ascending order -- an ID of a multi-day event appears once per timestep, as the
        reference's concatenation of per-slice ``regionprops_table`` results does.  ``area`` is float64 cells;
        ``centroid`` is float64 ``(component, ID)``: the mean row index and the mean column index, the latter with the
        seam rule of :meth:`calculate_centroid` unless ``regional_mode``.  Values <= 0 are background; a negative ID or
        one beyond int32 raises :class:`DataValidationError`.  On a mesh (track.py:2135-2323): ``area`` is float32 in the
        units of ``cell_areas`` and ``centroid`` float32 (lat, lon) in degrees, the direction of the area-weighted mean unit
        vector; one row per (timestep, ID) in (t, ID) order."""
        from .xr_compat import DataArray, Dataset

        if self.unstructured_grid:
            return self._mesh_object_properties(object_id_field, properties)
        properties = ["label", "area"] if properties is None else list(properties)
        if "label" not in properties:
            properties = ["label"] + properties
        bad = [p for p in properties if p not in SUPPORTED_PROPERTIES]
        if bad:
            raise ConfigurationError(f"Unsupported object properties: {bad}",
                                     details=f"supported on the device: {list(SUPPORTED_PROPERTIES)}",
                                     suggestions=[f"Pass a subset of {list(SUPPORTED_PROPERTIES)}"])
        eng = self._engine()
        ids, T, ny, nx = self._device_ids(object_id_field, eng)
        if ids.numel() == 0:
            r = {"id": np.zeros(0, np.int64), "area": np.zeros(0), "centroid": np.zeros((2, 0))}
        else:
            r = eng.object_moments(ids, ny, nx, wrap=not self.regional_mode)
        coord = {"ID": ("ID", r["id"])}
        data = {}
        if "area" in properties:
            data["area"] = DataArray(r["area"], dims=("ID",), coords=coord)
        if "centroid" in properties:
            data["centroid"] = DataArray(r["centroid"], dims=("component", "ID"), coords=coord)
        return Dataset(data, coords=coord)

    def check_overlap_slice(self, ids_t0, ids_next) -> np.ndarray:
        """Overlaps of two ID slices (track.py:2396-2452): ``(n, 3)`` int32 ``[id_t0, id_next, cells]`` over the cells
        where both are > 0, sorted lexicographically; ``(0, 3)`` when there are none.  Computed on the device.  On a mesh:
        ``(n, 3)`` float32 ``[id_t0, id_next, overlap area]``; IDs of 2^24 and above, which the float32 columns would round,
        raise :class:`TrackingError`."""
        import torch

        if self.unstructured_grid:
            return self._mesh_check_overlap_slice(ids_t0, ids_next)
        eng = self._engine()
        a, Ta, nya, nxa = self._device_ids(ids_t0, eng)
        b, Tb, nyb, nxb = self._device_ids(ids_next, eng)
        if (Ta, nya, nxa) != (1, nyb, nxb) or Tb != 1:
            raise create_data_validation_error("check_overlap_slice needs two 2-D slices of the same shape",
                                               details=f"got {tuple(ids_t0.shape)} and {tuple(ids_next.shape)}")
        if a.numel() == 0:
            return np.zeros((0, 3), np.int32)
        return eng.overlap_pairs(torch.cat([a, b], dim=0))

    def find_overlapping_objects(self, object_id_field) -> np.ndarray:
        """Overlaps of every slice t with slice t + 1, t < T - 1 (track.py:2454-2504), computed on the device: ``(n, 3)``
        int32 ``[id at t, id at t + 1, cells]``, counts of equal pairs summed over time, sorted lexicographically.  A sum
        that int32 cannot hold raises :class:`ProcessingError` instead of wrapping.  On a mesh: float32 rows with the shared
        area in the third column, as :meth:`check_overlap_slice`."""
        if self.unstructured_grid:
            return self._mesh_find_overlapping_objects(object_id_field)
        eng = self._engine()
        ids, T, ny, nx = self._device_ids(object_id_field, eng)
        if ids.numel() == 0:
            return np.zeros((0, 3), np.int32)
        return eng.overlap_pairs(ids)

    def enforce_overlap_threshold(self, overlap_objects_list, object_props) -> np.ndarray:
        """Keep the pairs that overlap enough (track.py:2506-2552): pairs whose IDs are not both in ``object_props.ID``
        are dropped; ``fraction = overlap / min(area_0, area_1)``; rows with ``fraction >= overlap_threshold`` are
        returned in the input's dtype, ``(0, 3)`` int32 when none remain.  A fraction above 1 is logged as a warning on
        the ``marex_amd`` logger.  Runs on the host.

        Defined for unique IDs only -- object properties of per-timestep objects, e.g. of
        ``identify_objects(..., time_connectivity=False)``: ``object_props`` with repeated IDs (those of multi-day events)
        raises :class:`DataValidationError`."""
        if self.unstructured_grid:
            return self._mesh_enforce_overlap_threshold(overlap_objects_list, object_props)
        ov = np.asarray(overlap_objects_list)
        empty = np.empty((0, 3), dtype=np.int32)
        if len(ov) == 0:
            return empty
        ids = np.asarray(object_props["ID"].values)
        area = np.asarray(object_props["area"].values, dtype=np.float64)
        order = np.argsort(ids, kind="stable")
        sid, sarea = ids[order], area[order]
        if sid.size > 1 and np.any(sid[1:] == sid[:-1]):
            raise create_data_validation_error(
                "object_props has repeated IDs", details="enforce_overlap_threshold needs one area per ID",
                suggestions=["Compute the properties of per-timestep objects (identify_objects(..., time_connectivity=False))"])

        def lookup(col):
            pos = np.clip(np.searchsorted(sid, col), 0, max(sid.size - 1, 0))
            found = (sid[pos] == col) if sid.size else np.zeros(col.shape, dtype=bool)
            return found, (sarea[pos] if sid.size else np.zeros(col.shape))

        return self._keep_overlaps(ov, lookup)

    def _keep_overlaps(self, ov: np.ndarray, lookup) -> np.ndarray:
        """The overlap-threshold rule (track.py:2506-2552) on ``(n, 3)`` pairs; ``lookup(ids) -> (found, area)`` says per
        column which IDs are known and their areas (any value where not found)."""
        empty = np.empty((0, 3), dtype=np.int32)
        if len(ov) == 0:
            return empty
        (f0, a0), (f1, a1) = lookup(ov[:, 0]), lookup(ov[:, 1])
        valid = f0 & f1
        if not np.any(valid):
            return empty
        valid_overlaps = ov[valid]
        overlap_fractions = valid_overlaps[:, 2].astype(float) / np.minimum(a0[valid], a1[valid])
        if np.any(overlap_fractions > 1.0):
            logger.warning(f"Found {np.sum(overlap_fractions > 1.0)} overlap fractions > 1.0")
            logger.warning(f"Max overlap fraction: {overlap_fractions.max()}")
        return valid_overlaps[overlap_fractions >= self.overlap_threshold]

    # ------------------------------------------------------------------ merge tracking on grids (track.py:2554-3802)
    def _unify_coordinates(self) -> None:
        """Coordinate units (track.py:919-976): ``coordinate_units`` is required in regional mode, else detected from the
        longitude range (~360: degrees, ~2 pi: radians).  ``self.lat`` / ``self.lon`` hold the coordinates in degrees."""
        units = self.coordinate_units
        lon = _host(self.lon_init)
        if self.regional_mode and units is None:
            raise create_data_validation_error("coordinate_units must be specified when regional_mode=True",
                                               suggestions=["Set coordinate_units='degrees' for degree-based coordinates",
                                                            "Set coordinate_units='radians' for radian-based coordinates"])
        if units is not None and units not in ("degrees", "radians"):
            raise create_data_validation_error(f"Invalid coordinate_units '{units}'",
                                               details="coordinate_units must be either 'degrees' or 'radians'")
        if units is None:
            rng = float(lon.max()) - float(lon.min())
            if abs(rng - 360.0) <= 1.0:
                units = "degrees"
            elif abs(rng - 2 * np.pi) <= 0.02:
                units = "radians"
            else:
                raise create_data_validation_error(
                    f"Cannot auto-detect coordinate units from range {rng:.3f}",
                    details=f"Expected ranges: ~360 degrees or ~{2 * np.pi:.3f} radians. Found range: {rng:.3f}",
                    suggestions=["Use regional_mode=True with coordinate_units specified for regional data",
                                 "Specify coordinate_units='degrees' or coordinate_units='radians' explicitly"])
        self.coordinate_units = units
        lat = _host(self.lat_init)
        if units == "radians":
            self.lon, self.lat = lon * 180.0 / np.pi, lat * 180.0 / np.pi
        else:
            self.lon, self.lat = lon, lat

    def _merge_cell_weights(self, cell_areas, grid_resolution):
        """float32 ``[ny, nx]`` cell areas of the final area / centroid pass (track.py:433-470), or None for unit areas
        (cell counts, summed as integers)."""
        d = self.data_bin
        ny, nx = d.shape[self._perm[1]], d.shape[self._perm[2]]
        if grid_resolution is not None:
            if cell_areas is not None:
                logger.warning("grid_resolution parameter overrides provided cell_areas for structured grid")
            lat_r = np.radians(self.lat)
            dl = np.radians(grid_resolution)
            g = (6378.0 ** 2 * np.abs(np.sin(lat_r + dl / 2) - np.sin(lat_r - dl / 2)) * dl).astype(np.float32)
            return np.ascontiguousarray(np.broadcast_to(g[:, None], (ny, nx)), dtype=np.float32)
        if cell_areas is None:
            return None
        a = _host(cell_areas).astype(np.float32)
        if a.ndim == 2 and tuple(getattr(cell_areas, "dims", ())) == (self.xdim, self.ydim):
            a = a.T
        return np.ascontiguousarray(np.broadcast_to(a if a.ndim == 2 else a[:, None], (ny, nx)), dtype=np.float32)

    def _enforce(self, ov: np.ndarray, props: _Props) -> np.ndarray:
        """enforce_overlap_threshold (track.py:2506-2552) against the live props."""
        def lookup(col):
            found = props.has(col)
            return found, props.area[np.where(found, col, 0)]

        return self._keep_overlaps(np.asarray(ov), lookup)

    def _slice_props(self, eng, ids, t, nx):
        r = eng.object_moments(ids[t:t + 1], ids.shape[1] // nx, nx, wrap=not self.regional_mode)
        return r["id"], r["area"], r["centroid"]

    def _consolidate(self, eng, ids, t: int, props: _Props, nx: int) -> None:
        """consolidate_object_ids of slice t against t - 1 (track.py:2554-2656), in place.  Every rename of the reference's
        loop is applied to a host table first (an ID renamed to a child that is renamed later follows it); the slice is
        then relabelled once.  The props the reference recomputes after each parent equal those of the final slice for
        the same IDs: after its last recomputation an ID's cells change only when it is renamed away, which drops it."""
        bo = eng.overlap_pairs(ids[t - 1:t + 1])
        if len(bo) == 0:
            return
        bo = self._enforce(bo, props)
        if len(bo) == 0:
            return
        pids, pc = np.unique(bo[:, 0], return_counts=True)
        members: Dict[int, List[int]] = {}
        firsts = []
        for p in pids[pc > 1].tolist():
            if not props.has(p):
                continue
            ch = bo[bo[:, 0] == p, 1].astype(np.int64).tolist()
            first = ch[0]
            if not props.has(first):
                continue
            for c in ch[1:]:
                if not props.has(c):
                    continue
                members.setdefault(first, [first]).extend(members.pop(c, [c]))
                props.alive[c] = False
            firsts.append(first)
        pairs = sorted((o, lab) for lab, grp in members.items() for o in grp if o != lab)
        if not pairs:
            return
        keys = np.array([o for o, _ in pairs], dtype=np.int32)
        vals = np.array([lab for _, lab in pairs], dtype=np.int32)
        eng.relabel(ids[t], vals, keys)
        sid, sa, sc = self._slice_props(eng, ids, t, nx)
        f = np.unique(np.asarray(firsts, dtype=np.int64))
        f = f[props.has(f)]
        pos = np.searchsorted(sid, f)
        props.set(f, sa[pos], sc[0][pos], sc[1][pos])

    def _merge_step(self, eng, ids, t: int, props: _Props, nx: int, state: dict) -> None:
        """The merges at step t (track.py:3438-3600): up to 10 iterations of partitioning every child with several
        parents at t - 1.

        All merging children of one iteration are partitioned in ONE launch, which gives the reference's result because
        (1) the parents' props at t - 1 do not change inside an iteration (only IDs at t are updated), (2) the child masks
        are disjoint, so one child's relabelling never touches another's cells, (3) the new IDs are fresh, so no cell of
        another child carries one, and (4) the props the reference writes after each child are those of the slice for
        that child's IDs, which later children of the same iteration do not touch: they equal the props of the final
        slice for those IDs."""
        ny = ids.shape[1] // nx
        wrap = not self.regional_mode
        tv = self.time_values[t]
        ov = self._enforce(eng.overlap_pairs(ids[t - 1:t + 1]), props)
        it = 0
        while it < 10:
            if len(ov) == 0:
                break
            uc, cc = np.unique(ov[:, 1], return_counts=True)
            merging = uc[cc > 1]
            if merging.size == 0:
                break
            off, par, lab, maxd, news, children = [0], [], [], [], [], []
            for child in merging.tolist():
                rows = ov[:, 1] == child
                parents = ov[rows, 0].astype(np.int64)
                k = parents.size
                nid = state["next_id"]
                if nid + k - 2 > _I32_MAX:
                    raise ProcessingError("new object IDs overflow int32", details=f"next ID {nid}, {k - 1} more needed")
                new = np.arange(nid, nid + k - 1, dtype=np.int64)
                state["next_id"] = nid + k - 1
                cids = np.concatenate([[child], new]).astype(np.int32)
                state["merges"].append((t, tv, parents.astype(np.int32), cids, ov[rows, 2].astype(np.int32)))
                par.extend(parents.tolist())
                lab.extend(cids.tolist())
                off.append(len(par))
                if self.nn_partitioning:
                    md = max(int(np.sqrt(np.max(props.area[parents])) * 3.0), 40)
                    maxd.extend([md] * k)
                news.append(new)
                children.append(child)
            par = np.asarray(par, dtype=np.int64)
            if self.nn_partitioning:
                eng.partition_nn(ids[t], ids[t - 1], ny, nx, merging, off, par, props.cy[par], props.cx[par], lab, maxd, wrap)
            else:
                eng.partition_centroid(ids[t], ny, nx, merging, off, props.cy[par], props.cx[par], lab, wrap)
            sid, sa, sc = self._slice_props(eng, ids, t, nx)
            for child, new in zip(children, news):
                j = np.searchsorted(sid, child)
                if j < sid.size and sid[j] == child:
                    props.set([child], sa[j], sc[0][j], sc[1][j])
                else:
                    props.alive[child] = False
                    logger.info(f"Deleted child_id {child} because parents have split/morphed")
                pos = np.minimum(np.searchsorted(sid, new), max(sid.size - 1, 0))
                got = (sid[pos] == new) if sid.size else np.zeros(new.size, bool)
                props.set(new[got], sa[pos[got]], sc[0][pos[got]], sc[1][pos[got]])
                if not got.all():
                    logger.warning(f"Missing newly created child_ids {set(new[~got].tolist())} "
                                   "because parents have split/morphed in the meantime...")
            ov = self._enforce(eng.overlap_pairs(ids[t - 1:t + 1]), props)
            it += 1
        if it == 10:
            logger.warning(f"Resolving mergers at timestep {t} did not converge after 10 iterations")

    def _split_and_merge(self, eng, ids, props: _Props, nx: int, block_steps: Optional[int] = None):
        """split_and_merge_objects (track.py:3337-3802) on the device field ``ids`` int32 [T, C], in place: returns the
        final overlap pairs (n, 2) and the merge records.  After the merges of step u, step u is consolidated against
        u - 1 (at relative step u + 1 of its chunk, or by the end-of-chunk pass), except when u is alone in its chunk.
        With ``block_steps`` the final overlap pass over the whole field runs in time blocks of that many steps, one step
        shared across each seam (its hash table then has the size of one block's runs), merged by :func:`merge_block_pairs`."""
        T = ids.shape[0]
        chunks = self._time_chunks or [T]
        if sum(chunks) != T:
            raise ConfigurationError("the time chunks do not cover the time axis", details=f"{chunks} for {T} steps")
        state = {"next_id": props.max_id() + 1, "merges": []}
        start = 0
        for L in chunks:
            for r in range(L):
                t = start + r
                if r > 0 and t >= 2:
                    self._consolidate(eng, ids, t - 1, props, nx)
                if t > 0:
                    self._merge_step(eng, ids, t, props, nx, state)
            if L >= 2:
                self._consolidate(eng, ids, start + L - 1, props, nx)
            start += L
        if block_steps is None:
            ov = eng.overlap_pairs(ids)
        else:
            from .engine import plan_time_blocks

            blocks = plan_time_blocks(T, ids.shape[1], int(block_steps) * ids.shape[1])
            ov = merge_block_pairs([eng.overlap_pairs(ids[t0:min(t1 + 1, T)]) for t0, t1 in blocks])
        ov = self._enforce(ov, props)
        if len(ov):
            uc, cc = np.unique(ov[:, 1], return_counts=True)
            if (cc > 1).any():
                logger.warning(f"Tracker Warning: {int((cc > 1).sum())} children have multiple parents after splitting/merging")
        return ov[:, :2], state["merges"]

    def _merges_dataset(self, merges):
        """merge_events of track.py:3758-3794."""
        from .xr_compat import DataArray, Dataset

        mp = max((len(m[2]) for m in merges), default=1)
        mc = max((len(m[3]) for m in merges), default=1)
        P = np.full((len(merges), mp), -1, np.int32)
        Cc = np.full((len(merges), mc), -1, np.int32)
        A = np.full((len(merges), mp), -1, np.int32)
        for i, (_, _, p, c, a) in enumerate(merges):
            P[i, :len(p)], Cc[i, :len(c)], A[i, :len(a)] = p, c, a
        times = np.array([m[1] for m in merges], dtype=self.time_values.dtype) if merges else np.array([], dtype=np.float64)
        ds = Dataset({"parent_IDs": DataArray(P, dims=("merge_ID", "parent_idx")),
                      "child_IDs": DataArray(Cc, dims=("merge_ID", "child_idx")),
                      "overlap_areas": DataArray(A, dims=("merge_ID", "parent_idx")),
                      "merge_time": DataArray(times, dims=("merge_ID",)),
                      "n_parents": DataArray(np.array([len(m[2]) for m in merges], np.int8), dims=("merge_ID",)),
                      "n_children": DataArray(np.array([len(m[3]) for m in merges], np.int8), dims=("merge_ID",))},
                     attrs={"fill_value": -1})
        return ds

    def _merge_time_index(self, merges_ds) -> np.ndarray:
        """Timestep of every merge of ``merges_ds``: the position of its ``merge_time`` on the time axis."""
        tpos = {v: i for i, v in enumerate(self.time_values.tolist())}
        return np.array([tpos[v] for v in np.asarray(merges_ds["merge_time"].values).tolist()], dtype=np.int64)

    def _cluster_rename_events(self, eng, ids, overlaps, merges_ds, merge_tidx, device_pass, field_dims, field_shape):
        """cluster_rename_objects_and_props (track.py:2809-3335) around the device pass, for grids and meshes alike: the
        events are the connected components of the overlap pairs over the IDs of the field and of the pair list, numbered
        by their smallest ID; ``device_pass(lut, N, spans)`` (``spans``: :meth:`HotPath.id_spans` of the field) relabels ``ids`` (int32 ``[T, C]`` on the device) in place through the
        ID -> event table and returns ``(gid, area, lat, lon)`` over the ``[T, N]`` (timestep, event) slots -- the largest
        original ID (0: the event is absent), float32 area and the centroid in degrees, whatever they hold where the event
        is absent.  Presence, time_start / time_end and the merge ledger follow from ``gid`` and ``merges_ds``.  Returns
        ``(events Dataset, N)``."""
        from .xr_compat import DataArray, Dataset

        T = ids.shape[0]
        sp = eng.id_spans(ids)
        present = np.nonzero(sp[1] >= 0)[0] if sp is not None else np.zeros(0, np.int64)
        present = present[present > 0]
        ov = np.asarray(overlaps, dtype=np.int64).reshape(-1, 2)
        valid = np.unique(np.concatenate([present, ov.reshape(-1)]))
        valid = valid[valid > 0]
        comp = _components(valid.size, np.searchsorted(valid, ov[:, 0]), np.searchsorted(valid, ov[:, 1]))
        N = int(comp.max()) + 1 if comp.size else 0
        lut = np.zeros(int(present[-1]) + 1 if present.size else 1, np.int32)
        keep = valid < lut.size
        lut[valid[keep]] = comp[keep] + 1
        coords = {self.timecoord: (self.timedim, self.time_values), "ID": ("ID", np.arange(1, N + 1, dtype=np.int32))}
        if N == 0:
            gid = np.zeros((T, 0), np.int32)
            area_all, lat_all, lon_all = (np.zeros((T, 0), np.float32) for _ in range(3))
        else:
            gid, area_all, lat_all, lon_all = device_pass(lut, N, sp)
        ev = ids
        pres = gid > 0
        t_first = np.argmax(pres, axis=0)
        t_last = T - 1 - np.argmax(pres[::-1], axis=0)
        area = np.where(pres, area_all, np.float32(np.nan))
        cen = np.full((2, T, N), np.nan, np.float32)
        cen[0][pres] = lat_all[pres]
        cen[1][pres] = lon_all[pres]
        P = np.asarray(merges_ds["parent_IDs"].values)
        ledger = np.full((T, N + 1, P.shape[1]), -1, np.int32)
        newP = lut[np.clip(np.where(P > 0, P, 0), 0, lut.size - 1)]
        for row, t in zip(newP, np.asarray(merge_tidx).tolist()):
            p = row[row > 0]
            ledger[t, p, :] = p[:, None]  # the reference's broadcast: [t, P, :] = P (track.py:3106-3112)
        tc = {self.timecoord: coords[self.timecoord]}
        idc = {"ID": coords["ID"]}
        tid = dict(tc, **idc)
        data = {
            "ID_field": DataArray(self._ids_to_host(eng, ev).reshape(field_shape), dims=field_dims, coords=tc),
            "global_ID": DataArray(gid, dims=(self.timedim, "ID"), coords=tid),
            "area": DataArray(area, dims=(self.timedim, "ID"), coords=tid),
            "centroid": DataArray(cen, dims=("component", self.timedim, "ID"),
                                  coords=dict(tid, component=("component", np.array([0, 1])))),
            "presence": DataArray(pres, dims=(self.timedim, "ID"), coords=tid),
            "time_start": DataArray(self.time_values[t_first], dims=("ID",), coords=idc),
            "time_end": DataArray(self.time_values[t_last], dims=("ID",), coords=idc),
            "merge_ledger": DataArray(ledger[:, 1:, :], dims=(self.timedim, "ID", "sibling_ID"), coords=tid),
        }
        return Dataset(data), N

    def _cluster_rename(self, eng, ids, ny: int, nx: int, overlaps, merges_ds, merge_tidx):
        """cluster_rename_objects_and_props (track.py:2809-3335), grids, with ``ids`` on the device (relabelled in place
        to event IDs) by one pass, :meth:`HotPath.event_rename`: an event's span of timesteps is the union of the spans of
        its IDs, its compact slots are turned into area and centroid and scattered into the dense ``[T, N]`` host arrays."""
        import torch

        T = ids.shape[0]

        def device_pass(lut, N, spans):
            tmin, tmax = spans if spans is not None else (np.zeros(0, np.int32), np.zeros(0, np.int32))  # None: no ID > 0
            live = np.nonzero(tmax[:lut.size] >= 0)[0]
            live = live[(live > 0) & (lut[live] > 0)]
            ev_tmin = np.full(N + 1, _I32_MAX, np.int64)
            ev_tmax = np.full(N + 1, -1, np.int64)
            np.minimum.at(ev_tmin, lut[live], tmin[live])
            np.maximum.at(ev_tmax, lut[live], tmax[live])
            w = None if self._cell_weights is None else torch.from_numpy(self._cell_weights.reshape(-1)).to(eng.device)
            r = eng.event_rename(ids, ny, nx, lut, ev_tmin, ev_tmax, w)
            mom = r["mom"]
            cnt = mom[:, 0]
            with np.errstate(invalid="ignore", divide="ignore"):
                if self._cell_weights is None:
                    tot = cnt.astype(np.float64)
                    sy, sx, sxs = mom[:, 1], mom[:, 2], mom[:, 3]
                    area = cnt.astype(np.float32)
                else:
                    wm = r["wmom"]
                    tot = wm[:, 0].astype(np.float32).astype(np.float64)  # the reference's float32 np.sum of the cell areas
                    sy, sx, sxs = wm[:, 1], wm[:, 2], wm[:, 3]
                    area = wm[:, 0].astype(np.float32)
                cy = sy / tot
                cx = sx / tot
                if not self.regional_mode:
                    seam = (mom[:, 4] & 3) == 3
                    cxs = sxs / tot
                    cxs = np.where(cxs < 0, cxs + nx, cxs)
                    cx = np.where(seam, cxs, cx)
            lat, lon = np.asarray(self.lat), np.asarray(self.lon)
            # slot -> (timestep, event): event e owns off[e] .. off[e + 1] - 1, one slot per step from ev_tmin[e] on
            from ._stream import slot_index  # _stream imports this module

            e_of, t_of = slot_index(r["off"], ev_tmin, N)
            dense = []
            for v, dt in ((r["gid"], np.int32), (area, np.float32), (np.interp(cy, np.arange(len(lat)), lat), np.float64),
                          (np.interp(cx, np.arange(len(lon)), lon), np.float64)):
                d = np.zeros((T, N), dt)
                d[t_of, e_of - 1] = v
                dense.append(d)
            return tuple(dense)

        return self._cluster_rename_events(eng, ids, overlaps, merges_ds, merge_tidx, device_pass, self._out_dims(), (T, ny, nx))

    def _remap_merge_coordinates(self, events_ds):
        """_remap_coordinates (track.py:978-1021) of the merge tracker's Dataset: the input's lat / lon as coordinates and
        the centroids from degrees into the input's units and longitude range."""
        from .xr_compat import DataArray, Dataset

        lon0 = _host(self.lon_init)
        lo, hi = float(lon0.min()), float(lon0.max())
        cen = np.asarray(events_ds["centroid"].values)
        clat, clon = cen[0], cen[1]
        if self.coordinate_units == "radians":
            clat = clat * np.pi / 180.0
            clon = clon * np.pi / 180.0
            if lo >= 0 and hi > np.pi:
                clon = np.where(clon < 0, clon + 2 * np.pi, clon)
        elif lo >= 0 and hi > 180:
            clon = np.where(clon < 0, clon + 360, clon)
        cen = np.stack([clat, clon]).astype(np.float32)
        extra = self._latlon_coords()
        data = {}
        for k, v in events_ds.data_vars.items():
            c = {n: (tuple(cv.dims), np.asarray(cv.values)) for n, cv in v.coords.items()}
            if k == "ID_field":
                c.update(extra)
            data[k] = DataArray(cen if k == "centroid" else v.values, dims=tuple(v.dims), coords=c, name=k)
        out = Dataset(data)
        out.attrs.update(events_ds.attrs)
        return out

    def track_objects(self, data_bin):
        """Events with merging and splitting (track.py:2734-2807), gridded data, on the device: per-timestep objects,
        their properties, split_and_merge_objects and cluster_rename_objects_and_props.  Returns ``(events_ds, merges_ds,
        N_events)``.  On a mesh (with a known time chunking): per-timestep objects made unique in time, their area-weighted
        properties, split_and_merge_objects_parallel and the cluster renaming, chained on one device tensor."""
        import time

        if self.unstructured_grid:
            self._mesh_need_chunks("tracker.track_objects")
            return self._mesh_track_objects(data_bin)
        B = None
        if self.merge_block_steps is None:
            self._check_size(data_bin.shape)  # without merge_block_steps: fields of 2^31 - 1 cells and more stay refused
            eng = self._engine()
        else:
            eng = self._engine()
            T, ny, nx = (int(data_bin.shape[k]) for k in self._perm_of(data_bin))
            B, need = self._merge_plan(eng, T, ny, nx, resident=_tensor_of(data_bin) is not None)
            self._check_fits(eng, need, "tracker.track_objects")
        st = self._stage_times = {}
        t0 = time.perf_counter()
        x, T, ny, nx = self._device_u8(data_bin, eng)
        r = eng.label_objects_3d(x, ny, nx, wrap_x=not self.regional_mode, connect_t=False,
                                 max_block_cells=None if B is None else B * ny * nx)
        ids = r["ids"].reshape(T, ny * nx)
        del x, r
        m = eng.object_moments(ids, ny, nx, wrap=not self.regional_mode)
        props = _Props(m["id"], m["area"], m["centroid"][0], m["centroid"][1])
        eng.sync()
        st["objects"] = time.perf_counter() - t0
        t0 = time.perf_counter()
        overlaps, merges = self._split_and_merge(eng, ids, props, nx, block_steps=B)
        merges_ds = self._merges_dataset(merges)
        eng.sync()
        st["split_and_merge"] = time.perf_counter() - t0
        t0 = time.perf_counter()
        tidx = np.array([m[0] for m in merges], dtype=np.int64)
        events_ds, N = self._cluster_rename(eng, ids, ny, nx, overlaps, merges_ds, tidx)
        st["cluster_rename"] = time.perf_counter() - t0
        return events_ds, merges_ds, N

    # the reference's public stage methods (track.py:2554-2656, 2809-3335, 3337-3802)
    def consolidate_object_ids(self, data_t_minus_2, data_t_minus_1, object_props, timestep: int):
        """Rename the children at t - 1 of a parent at t - 2 that has several to the first of them (track.py:2554-2656).
        Returns ``(data_t_minus_1, object_props)`` (a new DataArray and Dataset); runs on the device."""
        import torch

        from .xr_compat import DataArray

        if self.unstructured_grid:
            raise _not_built("tracker.consolidate_object_ids")
        eng = self._engine()
        a, _, ny, nx = self._device_ids(data_t_minus_2, eng)
        b, _, _, _ = self._device_ids(data_t_minus_1, eng)
        ids = torch.cat([a, b], dim=0).contiguous()
        props = _Props.of(object_props)
        self._consolidate(eng, ids, 1, props, nx)
        out = DataArray(ids[1].cpu().numpy().reshape(ny, nx), dims=(self.ydim, self.xdim), name="ID_field")
        return out, props.dataset()

    def split_and_merge_objects(self, object_id_field_unique, object_props):
        """split_and_merge_objects (track.py:3337-3802), gridded data, on the device: returns ``(object_id_field,
        object_props, overlap_objects_list (n, 2), merge_events)``.  IDs must be unique across time."""
        from .xr_compat import DataArray

        if self.unstructured_grid:
            raise _not_built("tracker.split_and_merge_objects")
        eng = self._engine()
        ids, T, ny, nx = self._device_ids(object_id_field_unique, eng)
        ids = ids.clone()
        props = _Props.of(object_props)
        ov, merges = self._split_and_merge(eng, ids, props, nx)
        field = DataArray(ids.cpu().numpy().reshape(T, ny, nx), dims=self._out_dims(),
                          coords={self.timecoord: (self.timedim, self.time_values[:T])}, name="ID_field")
        return field, props.dataset(), ov, self._merges_dataset(merges)

    def cluster_rename_objects_and_props(self, object_id_field_unique, object_props, overlap_objects_list, merge_events):
        """Events as connected components of the overlap pairs, numbered by their smallest ID, with global_ID, presence,
        time_start / time_end, area, centroid (degrees, before _remap_coordinates) and merge_ledger
        (track.py:2809-3335), on the device.  ``merge_events`` are the merge records of :meth:`split_and_merge_objects`; each
        merge is placed on the time axis by its ``merge_time``."""
        if self.unstructured_grid:
            self._mesh_need_chunks("tracker.cluster_rename_objects_and_props")
            return self._mesh_cluster_rename_stage(object_id_field_unique, overlap_objects_list, merge_events)
        eng = self._engine()
        ids, T, ny, nx = self._device_ids(object_id_field_unique, eng)
        ids = ids.clone()
        ds, _ = self._cluster_rename(eng, ids, ny, nx, overlap_objects_list, merge_events,
                                     self._merge_time_index(merge_events))
        return ds
