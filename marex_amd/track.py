"""Event tracking without merging on the device: ``marEx.tracker(..., allow_merging=False).run()`` for gridded data
(marEx/track.py:1162-1232, 1370-1497).

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

from .exceptions import ConfigurationError, TrackingError, create_data_validation_error

logger = logging.getLogger("marex_amd")

#: cells of one labelling (int32 parents; the limit of the 2-D labeller too)
MAX_CELLS = 2**31 - 1

#: regionprops names calculate_object_properties computes on the device
SUPPORTED_PROPERTIES = ("label", "area", "centroid")

_I32_MAX = 2**31 - 1


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


class tracker:  # noqa: N801 -- the reference's public name (marEx.tracker)
    """Identify extreme events as connected regions in (time, y, x) of a binary field on a grid.

    The constructor takes the reference's arguments (track.py:323-348).  Supported here: gridded data with
    ``allow_merging=False`` -- the reference's "basic" tracker.  ``allow_merging=True`` (the reference's default),
    ``unstructured_grid=True`` and ``checkpoint="save"`` / ``"load"`` raise :class:`ConfigurationError`.

    Accepted and ignored: ``grid_resolution`` and ``cell_areas`` (validated like the reference does; for gridded data the
    reference counts areas in cells anyway, track.py:1499-1518, 2337), ``temp_dir``, ``nn_partitioning``,
    ``max_iteration`` (merge tracking and meshes only), ``debug``, ``verbose``, ``quiet`` (logging) and
    ``coordinate_units`` (the output carries the input's lat / lon unchanged).  ``overlap_threshold`` is stored and used
    by :meth:`enforce_overlap_threshold`.

    The object stages of the reference's merge tracker are public methods here too (track.py:1499-1518, 2050-2552):
    :meth:`compute_area`, :meth:`calculate_centroid`, :meth:`calculate_object_properties` (on the device),
    :meth:`check_overlap_slice` and :meth:`find_overlapping_objects` (on the device) and :meth:`enforce_overlap_threshold`.

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
    ) -> None:
        supported = "gridded data with allow_merging=False and no checkpointing"
        if allow_merging:
            raise ConfigurationError("allow_merging=True is not supported on the device path",
                                     details=f"supported: {supported} (the reference's basic tracker)",
                                     suggestions=["Pass allow_merging=False"])
        if unstructured_grid:
            raise ConfigurationError("unstructured_grid=True is not supported by the device tracker",
                                     details=f"supported: {supported}; the reference tracks meshes with the merge tracker only")
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
        self.overlap_threshold = overlap_threshold
        self.unstructured_grid = unstructured_grid
        self.checkpoint = checkpoint
        self.data_attrs = dict(getattr(data_bin, "attrs", None) or {})
        self._validate_inputs(cell_areas, grid_resolution)
        self.lat_init = data_bin.coords[self.ycoord]
        self.lon_init = data_bin.coords[self.xcoord]
        self.time_values = np.asarray(data_bin.coords[self.timecoord].values)

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
            raise TrackingError("more than 2^31 - 1 cells; label the series in time blocks",
                                details=f"{n} cells: the device labelling holds one int32 parent per cell; time-blocked "
                                        "labelling with seam stitching is not built")

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
        """``run_preprocess`` -> ``run_tracking`` -> ``run_stats_attributes``; returns the events Dataset
        (``return_merges`` has nothing to return without merging)."""
        self._check_size(self.data_bin.shape)
        data_bin_preprocessed, object_stats = self.run_preprocess(checkpoint=checkpoint)
        events_ds, merges_ds, N_events_final = self.run_tracking(data_bin_preprocessed)
        return self.run_stats_attributes(events_ds, merges_ds, object_stats, N_events_final)

    def run_preprocess(self, checkpoint: Optional[str] = None) -> Tuple[object, Tuple[float, int, int, float, float, float]]:
        """Fill holes, fill time gaps and remove small objects (track.py:1234-1368), on the device.  Returns the filtered
        mask as a device-resident DataArray and ``(total_area_IDed, N_objects_prefiltered, N_objects_filtered,
        area_threshold, accepted_area_fraction, preprocessed_area_fraction)``, areas in cells."""
        import torch

        if checkpoint in ("save", "load"):
            raise ConfigurationError(f"checkpoint={checkpoint!r} is not supported by the device tracker")
        eng = self._engine()
        x, T, ny, nx = self._device_u8(self.data_bin, eng)
        mk = torch.from_numpy(self._mask_host.reshape(-1).astype(np.uint8)).to(eng.device)
        R = self.R_fill
        raw_area = float(x.sum(dtype=torch.int64).item())
        a = eng.fill_holes(x, mk, ny, nx, R, self.regional_mode)
        g = eng.fill_time_gaps(a, mk, ny, nx, R, int(self.T_fill), self.regional_mode)
        absolute = float(self.area_filter_absolute) if self._use_absolute_filtering else None
        r = eng.filter_small_objects(g, ny, nx, self.area_filter_quartile, absolute, self.regional_mode)
        areas = r["object_areas"].to(torch.float64)
        total = float(areas.sum().item())
        accepted = float(areas[areas > r["area_threshold"]].sum().item())  # strictly above, as track.py:1337
        processed = float(r["filtered"].sum(dtype=torch.int64).item())
        stats = (total, r["n_before"], r["n_after"], r["area_threshold"], accepted / total,
                 raw_area / processed if processed else float("nan"))
        return self._wrap_device(r["filtered"], T, ny, nx, "data_bin_preproc"), stats

    def identify_objects(self, data_bin, time_connectivity: bool):
        """Connected regions of ``data_bin`` (track.py:1912-2048, structured grid): 26-connected in (time, y, x) with
        ``time_connectivity``, else 8-connected per timestep; periodic in x unless ``regional_mode``.  Returns
        ``(ID_field int32, None, N_objects)``; IDs 1..N by first cell in C order, unique across time either way."""
        from .xr_compat import DataArray

        self._check_size(data_bin.shape)
        eng = self._engine()
        x, T, ny, nx = self._device_u8(data_bin, eng)
        r = eng.label_objects_3d(x, ny, nx, wrap_x=not self.regional_mode, connect_t=bool(time_connectivity))
        ids = r["ids"].cpu().numpy().reshape(T, ny, nx)
        N = int(r["n"].item())
        da = DataArray(ids, dims=self._out_dims(), coords={self.timedim: (self.timedim, self.time_values)}, name="ID_field")
        return da, None, N

    def run_tracking(self, data_bin_preprocessed):
        """Events without merging (track.py:1370-1412): ``identify_objects(time_connectivity=True)``; the time
        coordinate gets its own name back when it differs from the time dimension."""
        from .xr_compat import DataArray, Dataset

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
        print("Tracking Statistics:")
        print(f"   Binary Hobday to Processed Area Fraction: {preprocessed_area_fraction}")
        print(f"   Total Object Area IDed (cells): {total_area_IDed}")
        print(f"   Number of Initial Pre-Filtered Objects: {N_objects_prefiltered}")
        print(f"   Number of Final Filtered Objects: {N_objects_filtered}")
        print(f"   Area Cutoff Threshold (cells): {int(area_threshold)}")
        print(f"   Accepted Area Fraction: {accepted_area_fraction}")
        print(f"   Total Events Tracked: {N_events_final}")
        at.update(self.data_attrs)
        return self._remap_coordinates(events_ds)

    def _remap_coordinates(self, events_ds):
        """Re-assign the input's lat / lon coordinates (track.py:978-983)."""
        from .xr_compat import DataArray, Dataset

        v = events_ds["ID_field"]
        coords = {self.timecoord: (self.timedim, self.time_values),
                  self.ycoord: (_coord_dims(self.lat_init, (self.ydim,)), _host(self.lat_init)),
                  self.xcoord: (_coord_dims(self.lon_init, (self.xdim,)), _host(self.lon_init))}
        out = Dataset({"ID_field": DataArray(v.values, dims=tuple(v.dims), coords=coords, name="ID_field")})
        out.attrs.update(events_ds.attrs)
        return out

    # ------------------------------------------------------------------ object properties and overlaps (track.py:1499-1518, 2050-2552)
    def compute_area(self, data_bin):
        """Cells of ``data_bin`` per timestep (track.py:1499-1518, gridded: ``data_bin.sum(dim=[y, x])``), an int64
        DataArray over time.  ``data_bin`` may be device resident."""
        import torch

        from .xr_compat import DataArray

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
        one beyond int32 raises :class:`DataValidationError`."""
        from .xr_compat import DataArray, Dataset

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
        where both are > 0, sorted lexicographically; ``(0, 3)`` when there are none.  Computed on the device."""
        import torch

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
        that int32 cannot hold raises :class:`ProcessingError` instead of wrapping."""
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

        f0, a0 = lookup(ov[:, 0])
        f1, a1 = lookup(ov[:, 1])
        valid = f0 & f1
        if not np.any(valid):
            return empty
        valid_overlaps = ov[valid]
        overlap_fractions = valid_overlaps[:, 2].astype(float) / np.minimum(a0[valid], a1[valid])
        if np.any(overlap_fractions > 1.0):
            logger.warning(f"Found {np.sum(overlap_fractions > 1.0)} overlap fractions > 1.0")
            logger.warning(f"Max overlap fraction: {overlap_fractions.max()}")
        return valid_overlaps[overlap_fractions >= self.overlap_threshold]
