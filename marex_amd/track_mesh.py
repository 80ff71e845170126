"""The tracker on unstructured meshes (``marEx.tracker(unstructured_grid=True)``): the stages of ``track_objects``
(track.py:2734-2807) up to and including the overlap threshold -- per-timestep objects, IDs unique in time, area-weighted
object properties with centroids on the sphere, area-weighted time overlaps -- on the device.  The parallel
split-and-merge and the cluster renaming that follow (track.py:2809-3335, 3804-4826) are not built.

Arithmetic.  The reference sums cell areas and area-weighted unit vectors in float32 with ``np.add.at`` in cell order
(track.py:2190-2208, 2436-2439); a parallel float sum cannot reproduce that bit for bit, and float atomics differ from
run to run.  Here the weights are fixed point (:func:`mesh_weight_tables`), the device adds integers only, and the host
turns the sums into float32 values: every result is exact in the sense of that contract and bitwise reproducible, and
lies inside the rounding bound of the reference's own float32 sums (tests/test_mesh_tracker_host.py).
"""
from __future__ import annotations

from typing import List, Optional, Tuple

import numpy as np

from .exceptions import ConfigurationError, create_data_validation_error


def mesh_weight_tables(cell_areas, lat_deg, lon_deg) -> Tuple[int, np.ndarray]:
    """Fixed-point weights of a mesh of C cells, in NumPy float64 on the host: ``(e, q)`` with ``q`` int64 ``[4, C]``,

    * ``q[0] = rint(a * 2^e)`` and ``q[1], q[2], q[3] = rint(a * x * 2^e), rint(a * y * 2^e), rint(a * z * 2^e)``,
    * ``a = float64(cell_areas)``, ``x = cos(lat) cos(lon)``, ``y = cos(lat) sin(lon)``, ``z = sin(lat)`` of the
      coordinates in degrees converted with ``np.radians``,
    * ``e = 61 - ceil(log2(sum(a)))``, so that the sum of any row over all cells stays below 2^62 in magnitude (at most
      2^61 plus half a unit per cell) and 64-bit integer sums cannot overflow.

    An object's area is ``float32(S0 / 2^e)`` of its integer sum ``S0`` of ``q[0]``; its centroid is the direction of
    ``(S1, S2, S3)``.  :class:`DataValidationError` for an area that is negative or not finite, a coordinate that is not
    finite, or areas that sum to zero.  Needs no GPU."""
    a = np.ascontiguousarray(np.asarray(cell_areas, dtype=np.float64).reshape(-1))
    lat = np.asarray(lat_deg, dtype=np.float64).reshape(-1)
    lon = np.asarray(lon_deg, dtype=np.float64).reshape(-1)
    if lat.size != a.size or lon.size != a.size:
        raise create_data_validation_error("cell_areas, lat and lon must have one value per cell",
                                           details=f"{a.size} areas, {lat.size} latitudes, {lon.size} longitudes")
    if a.size == 0 or not np.isfinite(a).all() or (a < 0).any():
        raise create_data_validation_error("cell_areas must be finite and non-negative",
                                           details=f"{int((~np.isfinite(a)).sum())} non-finite and {int((a < 0).sum())} negative "
                                                   f"of {a.size} values")
    if not (np.isfinite(lat).all() and np.isfinite(lon).all()):
        raise create_data_validation_error("lat and lon must be finite on every cell of the mesh")
    total = float(a.sum())
    if not (total > 0 and np.isfinite(total)):
        raise create_data_validation_error("cell_areas must have a positive, finite sum", details=f"sum {total}")
    e = 61 - int(np.ceil(np.log2(total)))
    lat_r, lon_r = np.radians(lat), np.radians(lon)
    cl = np.cos(lat_r)
    q = np.empty((4, a.size), dtype=np.int64)
    q[0] = np.rint(np.ldexp(a, e))
    q[1] = np.rint(np.ldexp(a * (cl * np.cos(lon_r)), e))
    q[2] = np.rint(np.ldexp(a * (cl * np.sin(lon_r)), e))
    q[3] = np.rint(np.ldexp(a * np.sin(lat_r), e))
    return e, q


def _not_built(what: str) -> ConfigurationError:
    return ConfigurationError(
        f"{what} is not built for unstructured grids: the split-and-merge stage is missing",
        details="built on a mesh: run_preprocess, compute_area, identify_objects, unique_ids_in_time, "
                "calculate_object_properties, check_overlap_slice, find_overlapping_objects, enforce_overlap_threshold; the "
                "reference's split_and_merge_objects_parallel and cluster_rename_objects_and_props (track.py:2809-3335, "
                "3804-4826) are not",
        suggestions=["Use the stage methods up to enforce_overlap_threshold", "Track gridded data"])


class _MeshStages:
    """The mesh side of :class:`marex_amd.tracker`: constructor branch and stage methods (``self`` is the tracker)."""

    # ------------------------------------------------------------------ constructor (track.py:493-639, 1023-1089)
    def _init_mesh(self, data_bin, mask, R_fill, area_filter_quartile, area_filter_absolute, T_fill, allow_merging,
                   nn_partitioning, overlap_threshold, dimensions, coordinates, neighbours, cell_areas, grid_resolution,
                   max_iteration, checkpoint, regional_mode, coordinate_units, device) -> None:
        from .track import _host, _tensor_of

        if neighbours is None or cell_areas is None:
            raise ConfigurationError("unstructured_grid=True is not supported without neighbours and cell_areas",
                                     details="a mesh needs its connectivity (neighbours: ('nv', x), 3 rows, 1-based) and its "
                                             "cell areas (over x)",
                                     suggestions=["Pass neighbours= and cell_areas= of the mesh"])
        if checkpoint in ("save", "load"):
            raise ConfigurationError(f"checkpoint={checkpoint!r} is not supported by the device tracker",
                                     details="the pipeline stays in device memory", suggestions=["Pass checkpoint=None"])
        if regional_mode:
            raise NotImplementedError("regional_mode is not yet implemented for unstructured grids")
        self.data_bin = data_bin
        self.mask = mask
        self.regional_mode = False
        self.device = device
        dimensions = dimensions or {}
        self.timedim = dimensions.get("time", "time")
        self.xdim = dimensions.get("x", "lon")
        self.ydim = None
        coordinates = coordinates or {}
        self.timecoord = coordinates.get("time", self.timedim)
        self.xcoord = coordinates.get("x", self.xdim)
        self.ycoord = coordinates.get("y", dimensions.get("y", "lat"))
        self.R_fill = int(R_fill)
        self.T_fill = T_fill
        self._resolve_area_filtering_parameters(area_filter_quartile, area_filter_absolute)
        self.allow_merging = allow_merging
        self.nn_partitioning = bool(nn_partitioning)
        self.overlap_threshold = overlap_threshold
        self.unstructured_grid = True
        self.checkpoint = checkpoint
        self.max_iteration = max_iteration
        self.data_attrs = dict(getattr(data_bin, "attrs", None) or {})

        dims = tuple(getattr(data_bin, "dims", ()))
        want = (self.timedim, self.xdim)
        if len(dims) != 2 or set(dims) != set(want):
            raise create_data_validation_error(
                "Invalid dimensions for unstructured data",
                details=f"Expected 2D array with dimensions {want}, got {list(dims)}",
                suggestions=["Ensure data has time and cell dimensions only", "Check dimension mapping in function call"],
                data_info={"actual_dims": list(dims), "expected_dims": list(want)})
        self._perm = tuple(dims.index(k) for k in want)
        coords = getattr(data_bin, "coords", {})
        if self.timecoord not in coords or self.xcoord not in coords or self.ycoord not in coords:
            raise create_data_validation_error(
                "Missing required coordinates in unstructured data",
                details=f"Expected coordinates ({self.timecoord}, {self.xcoord}, {self.ycoord}), but found {list(coords)}",
                suggestions=["Ensure data_bin contains time, x, and y coordinates",
                             "Specify coordinates in the tracker initialisation with `coordinates` parameter."])
        t = _tensor_of(data_bin)
        dt = str(t.dtype).replace("torch.", "") if t is not None else str(np.asarray(data_bin.values).dtype)
        if dt != "bool" and not (t is not None and dt == "uint8"):  # a device mask may also be 0 / 1 bytes
            raise create_data_validation_error(
                "Input DataArray must be binary (boolean type)", details=f"Found dtype {dt}, expected bool",
                suggestions=["Convert data using da > threshold for binary events"],
                data_info={"actual_dtype": dt, "expected_dtype": "bool"})
        if grid_resolution is not None:
            raise create_data_validation_error(
                "grid_resolution parameter is not supported for unstructured grids",
                details="Grid resolution calculation requires structured (lat/lon) coordinates",
                suggestions=["Use cell_areas parameter directly for unstructured grids"])
        Cn = int(data_bin.shape[self._perm[1]])
        m = _host(mask)
        if m.dtype != bool:
            raise create_data_validation_error(
                "Mask must be binary (boolean type)", details=f"Found mask dtype {m.dtype}, expected bool",
                suggestions=["Convert mask using mask > 0 or mask.astype(bool)"], data_info={"mask_dtype": str(m.dtype)})
        if not m.any():
            raise create_data_validation_error(
                "Mask contains only False values", details="Mask should indicate valid regions with True values",
                suggestions=["Check mask orientation - it should mark valid (ocean) regions as True"])
        if m.shape != (Cn,):
            raise create_data_validation_error("Mask shape does not match the cells of data_bin",
                                               details=f"mask {m.shape}, data ({Cn},)")
        self._mask_host = np.ascontiguousarray(m)
        nb = _host(neighbours)
        if nb.ndim != 2 or nb.shape[0] != 3 or nb.shape[1] != Cn:
            raise create_data_validation_error(
                "Invalid neighbour array for triangular grid", details=f"Expected shape (3, {Cn}), got {nb.shape}",
                suggestions=["Ensure triangular grid connectivity", "Check neighbour array from grid file"],
                data_info={"actual_shape": tuple(nb.shape), "expected_shape": "(3, ncells)"})
        nb_dims = tuple(getattr(neighbours, "dims", ("nv", self.xdim)))
        if nb_dims != ("nv", self.xdim):
            raise create_data_validation_error(
                "Invalid neighbour array dimensions", details=f"Expected dimensions ('nv', '{self.xdim}'), got {nb_dims}",
                suggestions=["Check dimension names in grid file", "Verify coordinate mapping"],
                data_info={"actual_dims": nb_dims, "expected_dims": ("nv", self.xdim)})
        if nb.dtype.kind not in "iuf" or not np.isfinite(nb).all() or nb.max() > Cn:
            raise create_data_validation_error(  # the kernels index cells with these values
                "Invalid neighbour array for triangular grid",
                details=f"Expected 1-based cell numbers up to {Cn} (0 or less: no neighbour), largest value {nb.max()}")
        self._nbr_host = np.ascontiguousarray(np.maximum(nb.astype(np.int64) - 1, -1).astype(np.int32))  # track.py:1060
        ca = _host(cell_areas)
        ca_dims = tuple(getattr(cell_areas, "dims", (self.xdim,)))
        if ca_dims != (self.xdim,) or ca.shape != (Cn,):
            raise create_data_validation_error(
                "Invalid cell_areas dimensions for unstructured grid",
                details=f"Expected dimensions ('{self.xdim}',) of {Cn} cells, got {ca_dims} {ca.shape}",
                suggestions=["Ensure cell_areas has one value per cell of the mesh"])
        if not self._use_absolute_filtering:
            if self.area_filter_quartile < 0 or self.area_filter_quartile > 1:
                raise ConfigurationError("Invalid area_filter_quartile value",
                                         details=f"Value {self.area_filter_quartile} is outside valid range [0, 1]",
                                         suggestions=["Use values between 0.0 and 1.0"],
                                         context={"provided_value": self.area_filter_quartile, "valid_range": [0, 1]})
        elif self.area_filter_absolute <= 0:
            raise ConfigurationError("Invalid area_filter_absolute value",
                                     details=f"area_filter_absolute={self.area_filter_absolute} must be positive",
                                     suggestions=["Set area_filter_absolute to a positive integer (e.g., 5, 10, 50)"],
                                     context={"area_filter_absolute": self.area_filter_absolute})
        if self.T_fill % 2 != 0:
            raise ConfigurationError("T_fill must be even for temporal symmetry", details=f"Provided T_fill={self.T_fill} is odd",
                                     suggestions=["Use even values: 2, 4, 6, 8, etc."],
                                     context={"provided_value": self.T_fill, "requirement": "even number"})
        if self.R_fill < 0 or self.R_fill > 1024:
            raise ConfigurationError("R_fill must be between 0 and 1024 on a mesh", details=f"R_fill={self.R_fill}")
        self.lat_init = data_bin.coords[self.ycoord]
        self.lon_init = data_bin.coords[self.xcoord]
        if _host(self.lat_init).shape != (Cn,) or _host(self.lon_init).shape != (Cn,):
            raise create_data_validation_error("lat and lon must be coordinates over the cells of the mesh",
                                               details=f"lat {_host(self.lat_init).shape}, lon {_host(self.lon_init).shape}, {Cn} cells")
        self.time_values = np.asarray(data_bin.coords[self.timecoord].values)
        self.coordinate_units = coordinate_units
        self._unify_coordinates()  # self.lat / self.lon in degrees
        self.cell_area = ca.astype(np.float32)  # the reference's own copy (track.py:477)
        self._mesh_e, self._mesh_q = mesh_weight_tables(ca, self.lat, self.lon)
        self._mesh_dev_tables = None

    # ------------------------------------------------------------------ device plumbing
    def _mesh_tables(self, eng):
        """``(q int64 [4, C], nbr int32 [3, C], mask uint8 [C])`` on the engine's device, uploaded once."""
        import torch

        if self._mesh_dev_tables is None or self._mesh_dev_tables[0].device != eng.device:
            self._mesh_dev_tables = (torch.from_numpy(self._mesh_q).to(eng.device), torch.from_numpy(self._nbr_host).to(eng.device),
                                     torch.from_numpy(self._mask_host.astype(np.uint8)).to(eng.device))
        return self._mesh_dev_tables

    def _mesh_perm(self, field) -> bool:
        """Whether ``field`` (2-D) comes as (x, time) and has to be transposed."""
        dims = getattr(field, "dims", None)
        if dims is not None and len(dims) == 2 and tuple(dims) == (self.xdim, self.timedim):
            return True
        if dims is not None and len(dims) == 2 and set(dims) != {self.timedim, self.xdim}:
            raise create_data_validation_error(
                "Invalid dimensions for unstructured data",
                details=f"Expected dimensions {(self.timedim, self.xdim)}, got {list(dims)}", data_info={"actual_dims": list(dims)})
        return False

    def _mesh_device_u8(self, da, eng):
        """``da`` as a contiguous uint8 ``[T, C]`` device tensor; device data is not copied to the host."""
        import torch

        from .track import _tensor_of

        t = _tensor_of(da)
        if t is None and type(da).__module__.startswith("torch"):
            t = da
        swap = self._mesh_perm(da)
        if t is None:
            a = np.asarray(da.values if hasattr(da, "values") else da)
            t = torch.from_numpy(np.ascontiguousarray(a.T if swap else a).astype(np.uint8)).to(eng.device)
        else:
            if t.device != eng.device:
                t = t.to(eng.device)
            t = (t.t() if swap else t).contiguous()
            t = t.view(torch.uint8) if t.dtype == torch.bool else t.to(torch.uint8)
        if t.dim() != 2 or t.shape[1] != self._mesh_q.shape[1]:
            raise create_data_validation_error("Invalid dimensions for unstructured data",
                                               details=f"Expected (time, {self._mesh_q.shape[1]} cells), got {tuple(t.shape)}")
        return t

    def _mesh_device_ids(self, field, eng):
        """An ID field as a contiguous int32 ``[T, C]`` device tensor (a 1-D field is one slice)."""
        import torch

        from .track import _I32_MAX, _tensor_of

        t = _tensor_of(field)
        if t is None and type(field).__module__.startswith("torch"):
            t = field
        nd = len(field.shape)
        if nd not in (1, 2):
            raise create_data_validation_error("Invalid dimensions for an object ID field on a mesh",
                                               details=f"Expected (time, x) or (x,), got shape {tuple(field.shape)}")
        swap = nd == 2 and self._mesh_perm(field)
        if t is None:
            a = np.asarray(field.values if hasattr(field, "values") else field)
            if a.dtype.kind not in "iu":
                raise create_data_validation_error("Object IDs must be integers", details=f"Found dtype {a.dtype}",
                                                   data_info={"actual_dtype": str(a.dtype)})
            if a.dtype != np.int32 and a.size:
                lo, hi = int(a.min()), int(a.max())
                if lo < 0 or hi > _I32_MAX:
                    raise self._id_range_error(lo, hi)
            t = torch.from_numpy(np.ascontiguousarray(a.T if swap else a, dtype=np.int32)).to(eng.device)
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
            t = (t.t() if swap else t).contiguous()
        if t.dim() == 1:
            t = t.unsqueeze(0)
        if t.shape[1] != self._mesh_q.shape[1]:
            raise create_data_validation_error("Invalid dimensions for an object ID field on a mesh",
                                               details=f"Expected {self._mesh_q.shape[1]} cells per timestep, got {tuple(t.shape)}")
        return t

    def _mesh_wrap(self, t, name: str):
        from .zarr_io import DeviceDataArray

        return DeviceDataArray(t, (self.timedim, self.xdim), {self.timedim: self.time_values[:t.shape[0]]}, name=name)

    # ------------------------------------------------------------------ stages
    def _mesh_run_preprocess(self):
        """fill_holes(R) -> temporal closing -> fill_holes(R // 2) -> filter_small_objects on the mesh, and the statistics
        of track.py:1283-1351: object areas in cells, ``preprocessed_area_fraction`` from the area-weighted
        :meth:`compute_area`."""
        import torch

        eng = self._engine()
        x = self._mesh_device_u8(self.data_bin, eng)
        n = int(x.numel())
        need = {"hole-filled mask uint8": n, "labels int32": 4 * n, "sizes int32": 4 * n, "filtered mask uint8": n,
                "library scratch": 4 * n}
        if _is_host(self.data_bin):
            need["mask uint8"] = n
        if int(self.T_fill) > 0:
            need["time-closed and gap-filled masks uint8"] = 2 * n
        self._check_fits(eng, need, "tracker.run_preprocess")
        q, nbr, mk = self._mesh_tables(eng)
        raw_area = float(eng.mesh_area(x, q, self._mesh_e).sum())
        g = eng.fill_holes_mesh(x, mk, nbr, self.R_fill)
        if int(self.T_fill) > 0:
            g = eng.fill_holes_mesh(eng.time_closing(g, int(self.T_fill)), mk, nbr, self.R_fill // 2)
        absolute = float(self.area_filter_absolute) if self._use_absolute_filtering else None
        r = eng.filter_small_objects_mesh(g, mk, nbr, self.area_filter_quartile, absolute)
        eng.sync()
        areas = r["object_areas"].to(torch.float64)
        total = float(areas.sum().item())
        accepted = float(areas[areas > r["area_threshold"]].sum().item())  # strictly above, as track.py:1337
        processed = float(eng.mesh_area(r["filtered"], q, self._mesh_e).sum())
        stats = (total, r["n_before"], r["n_after"], r["area_threshold"], accepted / total,
                 raw_area / processed if processed else float("nan"))
        return self._mesh_wrap(r["filtered"], "data_bin_preproc"), stats

    def _mesh_compute_area(self, data_bin):
        from .xr_compat import DataArray

        eng = self._engine()
        x = self._mesh_device_u8(data_bin, eng)
        q, _, _ = self._mesh_tables(eng)
        area = eng.mesh_area(x, q, self._mesh_e)
        coords = {}
        c = getattr(data_bin, "coords", None) or {}
        if self.timecoord in c:
            coords[self.timecoord] = (self.timedim, np.asarray(c[self.timecoord].values))
        return DataArray(area, dims=(self.timedim,), coords=coords)

    def _mesh_identify_objects(self, data_bin, time_connectivity: bool):
        from .xr_compat import DataArray

        if time_connectivity:
            raise ConfigurationError("Time connectivity not supported for unstructured grids",
                                     details="Automatic time connectivity computation requires regular grids",
                                     suggestions=["Set time_connectivity=False for unstructured data"])
        eng = self._engine()
        x = self._mesh_device_u8(data_bin, eng)
        T, Cn = (int(k) for k in x.shape)
        q, nbr, mk = self._mesh_tables(eng)
        block = None if self.label_block_steps is None else self.label_block_steps * Cn
        r = eng.label_objects_mesh(x, mk, nbr, max_block_cells=block)
        ids = self._ids_to_host(eng, r["ids"])
        da = DataArray(ids, dims=(self.timedim, self.xdim), coords={self.timedim: (self.timedim, self.time_values[:T])},
                       name="ID_field")
        return da, None, 1  # the reference's placeholder: IDs restart in every timestep (track.py:2005)

    def unique_ids_in_time(self, object_id_field):
        """IDs that restart at 1 in every timestep (:meth:`identify_objects` on a mesh) made unique across time
        (track.py:2762-2764), on the device: every ID grows by the sum of the per-timestep maxima of the timesteps before
        it.  Returns an int32 DataArray like the input; :class:`TrackingError` above 2^31 - 2 objects."""
        from .xr_compat import DataArray

        if not self.unstructured_grid:
            raise ConfigurationError("unique_ids_in_time is a stage of the mesh tracker",
                                     details="identify_objects numbers gridded objects uniquely across time already")
        eng = self._engine()
        ids = self._mesh_device_ids(object_id_field, eng)
        if ids.numel() == 0:
            out = ids.cpu().numpy()
        else:
            out = self._ids_to_host(eng, eng.unique_ids_in_time(ids))
        coords = {}
        c = getattr(object_id_field, "coords", None) or {}
        if self.timedim in c:
            coords[self.timedim] = (self.timedim, np.asarray(c[self.timedim].values))
        return DataArray(out, dims=(self.timedim, self.xdim), coords=coords, name="ID_field")

    def _mesh_object_properties(self, object_id_field, properties: Optional[List[str]]):
        from .track import SUPPORTED_PROPERTIES
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
        ids = self._mesh_device_ids(object_id_field, eng)
        if ids.numel() == 0:
            r = {"id": np.zeros(0, np.int64), "area": np.zeros(0, np.float32), "centroid": np.zeros((2, 0), np.float32)}
        else:
            r = eng.mesh_object_moments(ids, self._mesh_tables(eng)[0], self._mesh_e)
        coord = {"ID": ("ID", r["id"])}
        data = {}
        if "area" in properties:
            data["area"] = DataArray(r["area"], dims=("ID",), coords=coord)
        if "centroid" in properties:
            data["centroid"] = DataArray(r["centroid"], dims=("component", "ID"), coords=coord)
        return Dataset(data, coords=coord)

    def _mesh_check_overlap_slice(self, ids_t0, ids_next) -> np.ndarray:
        import torch

        eng = self._engine()
        a, b = self._mesh_device_ids(ids_t0, eng), self._mesh_device_ids(ids_next, eng)
        if a.shape[0] != 1 or b.shape[0] != 1:
            raise create_data_validation_error("check_overlap_slice needs two 1-D slices over the cells of the mesh",
                                               details=f"got {tuple(ids_t0.shape)} and {tuple(ids_next.shape)}")
        return eng.mesh_overlap_pairs(torch.cat([a, b], dim=0), self._mesh_tables(eng)[0], self._mesh_e)

    def _mesh_find_overlapping_objects(self, object_id_field) -> np.ndarray:
        eng = self._engine()
        ids = self._mesh_device_ids(object_id_field, eng)
        if ids.numel() == 0:
            return np.zeros((0, 3), np.float32)
        return eng.mesh_overlap_pairs(ids, self._mesh_tables(eng)[0], self._mesh_e)

    def _mesh_enforce_overlap_threshold(self, overlap_objects_list, object_props) -> np.ndarray:
        """track.py:2526-2552 on a mesh: float32 areas, float64 fractions, float32 rows out."""
        ov = np.asarray(overlap_objects_list)
        empty = np.empty((0, 3), dtype=np.float32)
        if len(ov) == 0:
            return empty
        ids = np.asarray(object_props["ID"].values)
        area = np.asarray(object_props["area"].values, dtype=np.float32)
        order = np.argsort(ids, kind="stable")
        sid, sarea = ids[order], area[order]
        if sid.size > 1 and np.any(sid[1:] == sid[:-1]):
            raise create_data_validation_error(
                "object_props has repeated IDs", details="enforce_overlap_threshold needs one area per ID",
                suggestions=["Compute the properties of IDs that are unique in time (unique_ids_in_time)"])

        def lookup(col):
            col = col.astype(np.int64)
            pos = np.clip(np.searchsorted(sid, col), 0, max(sid.size - 1, 0))
            found = (sid[pos] == col) if sid.size else np.zeros(col.shape, dtype=bool)
            return found, (sarea[pos] if sid.size else np.zeros(col.shape, np.float32))

        (f0, a0), (f1, a1) = lookup(ov[:, 0]), lookup(ov[:, 1])
        valid = f0 & f1
        if not np.any(valid):
            return empty
        kept = ov[valid]
        fractions = kept[:, 2].astype(float) / np.minimum(a0[valid], a1[valid])
        if np.any(fractions > 1.0):
            from .track import logger

            logger.warning(f"Found {np.sum(fractions > 1.0)} overlap fractions > 1.0")
            logger.warning(f"Max overlap fraction: {fractions.max()}")
        return kept[fractions >= self.overlap_threshold]


def _is_host(da) -> bool:
    from .track import _tensor_of

    return _tensor_of(da) is None and not type(da).__module__.startswith("torch")
