"""marex_amd -- MI355X-native (gfx950) hot path behind marEx-style ``preprocess_data``.

Public names mirror the reference's re-exports for this path (marEx/__init__.py:36-42, 45-58).
Importing the package never touches the GPU; the HIP extension is loaded on the first compute call and
its absence is an error (no CPU fallback).

Beyond the reference: ``preprocess_data`` and ``identify_extremes`` take ``neighbour_rings_hobday=1 | 2`` with ``neighbours``
on unstructured meshes -- day-of-year thresholds pooled over the cell and one or two rings of its listed neighbours, the mesh
counterpart of ``window_spatial_hobday``.  ``event_categories`` and ``tracker.event_categories`` give the severity
categories (Hobday et al. 2018) of every tracked event and the category map of every timestep, from ``ID_field``,
``dat_anomaly`` and ``thresholds`` on the device.  ``compound_events`` joins two presence fields in one pass on the device:
joint, lagged and run-level coincidence per cell, by time group and by latitude class.  ``cell_trends`` gives the per-cell
trend of a series of annual maps -- Theil-Sen slope with confidence bounds, Mann-Kendall test, least squares -- on the device.
``regional_series`` gives, per timestep and region of any integer region map, the area in an extreme state as an exact
integer sum of fixed-point cell areas, its share of the region, the area-weighted intensity and the severity categories.
``event_composites`` gives the lagged composites (superposed-epoch analysis) of any float field around the onsets or the ends
of every cell's events: count, sum, sum of squares, mean, standard deviation and t statistic per lag, on the device.
``event_shapes`` and ``tracker.event_shapes`` give the shape and the movement of every tracked event on a grid: bounding box
and extent, exposed sides, perimeter and coastal contact, the axes, eccentricity and orientation of its second moments, and
the path, displacement and speed of its centroid -- integer sums on the device, float64 on the host; ``grid_edge_lengths``
gives the side lengths of a regular lat-lon grid for perimeters in km.  ``mesh_event_shapes`` -- and ``tracker.event_shapes`` of
a mesh tracker -- give the same on an unstructured mesh of three-sided cells: exposed, border, coast and contact sides over
the three neighbour slots, perimeter, a latitude / longitude box, axes from the second moments of the unit vectors on the
sphere, and the great-circle path of the centroid.
``event_exposure`` and ``tracker.event_exposure`` join the tracked events with any integer region map: per (event, region)
pair the steps, the cell-steps and area-steps, the largest extent and the intensity of the event inside the region, per
event its main region and the share outside every region, per region the events it saw -- a keyed accumulation on the device.
``event_matching`` and ``tracker.event_matching`` join the events of two trackings of the same cells: per pair of events the
steps, the cell-steps and area-steps of their overlap, its share of either event, the intersection over union and the onset
and end lags, per event its partners and its matched share, and the hit rate, false-alarm ratio and critical success index.
"""
from .detect import (
    compute_normalised_anomaly,
    identify_extremes,
    preprocess_data,
    rolling_climatology,
    smoothed_rolling_climatology,
)
from .exceptions import (
    ConfigurationError,
    DataValidationError,
    DependencyError,
    MarExError,
    ProcessingError,
    TrackingError,
    create_data_validation_error,
)
from .dask_adapter import preprocess_data_lazy
from .intensity import event_intensity
from .event_categories import event_categories
from .occurrence import event_occurrence
from .local_intensity import local_intensity
from .cell_events import cell_events
from .heat_stress import heat_stress, monthly_maximum_climatology
from .resample import nearest_cell_index, resample_nearest
from .compound import compound_events
from .composites import event_composites
from .trends import cell_trends
from .regional import regional_series
from .exposure import event_exposure
from .matching import event_matching
from .shapes import event_shapes, grid_edge_lengths
from .shapes_mesh import mesh_event_shapes
from .track import tracker
from .xr_compat import DataArray, Dataset

__all__ = [
    "preprocess_data", "preprocess_data_lazy", "compute_normalised_anomaly", "identify_extremes", "rolling_climatology",
    "smoothed_rolling_climatology", "MarExError", "DataValidationError", "ConfigurationError",
    "ProcessingError", "DependencyError", "create_data_validation_error", "DataArray", "Dataset",
    "tracker", "TrackingError", "event_intensity", "event_occurrence", "local_intensity",
    "cell_events", "event_categories", "compound_events", "cell_trends", "regional_series",
    "event_composites", "event_shapes", "grid_edge_lengths", "event_exposure", "event_matching",
    "mesh_event_shapes", "heat_stress", "monthly_maximum_climatology", "nearest_cell_index", "resample_nearest",
]
__version__ = "0.1.0"
