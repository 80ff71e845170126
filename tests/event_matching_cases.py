"""The shared cases of the event matching tests: pairs of ID fields at the edges of the kernel's layout, of its key and of its
table, and the comparison of an engine result or a Dataset with the oracle.  Not collected by pytest."""
import numpy as np

import event_matching_oracle as mo
from event_exposure_cases import blob_field, id_field  # noqa: F401  (the field builders of the exposure tests)

I31 = 2**31 - 1


def blob_pair(rng, T, C, n_ids=6, width=9):
    """Two blob fields drawn independently: events that overlap in part, in whole and not at all."""
    return blob_field(rng, T, C, n_ids, width), blob_field(rng, T, C, n_ids + 1, max(1, width - 2))


def random_pair(rng, T, C, n_ids=5):
    """Per-cell random IDs: nothing folds beyond chance, every (a, b) combination appears, 0 included."""
    return id_field(rng, T, C, 0.5, n_ids), id_field(rng, T, C, 0.4, n_ids + 2)


def shifted(x, steps=1):
    """``x`` moved ``steps`` later in time, the first steps empty."""
    y = np.zeros_like(x)
    y[steps:] = x[:x.shape[0] - steps]
    return y


def assert_same(r, recs):
    """An engine result against the oracle's records: every column an equal integer array of the same type."""
    exp = mo.as_arrays(recs)
    for k in ("t", "a", "b", "cells", "area"):
        assert r[k].dtype == exp[k].dtype and r[k].shape == exp[k].shape, (k, r[k].dtype, r[k].shape, exp[k].shape)
        assert np.array_equal(r[k], exp[k]), (k, np.flatnonzero(r[k] != exp[k])[:5])


def assert_dataset(ds, exp, tname="time"):
    """A Dataset against ``matching(...)``: the same variables, types and shapes; integers and times equal, floats equal with
    ``==`` (each is one division of exact integers), NaN where the oracle has NaN."""
    want, coords = exp
    assert sorted(ds.data_vars) == sorted(want), sorted(set(ds.data_vars) ^ set(want))
    for k, w in want.items():
        got, w = np.asarray(ds[k].values), np.asarray(w)
        assert got.shape == w.shape and got.dtype == w.dtype, (k, got.shape, w.shape, got.dtype, w.dtype)
        assert np.array_equal(got, w, equal_nan=got.dtype.kind in "fmM"), (k, got, w)
    assert np.array_equal(np.asarray(ds["a_steps"].coords["ID_a"].values), coords["ID_a"])
    assert np.array_equal(np.asarray(ds["b_steps"].coords["ID_b"].values), coords["ID_b"])
    assert tuple(ds["step_cells_both"].dims) == (tname,) and tuple(ds["pair_iou"].dims) == ("pair",) and tuple(ds["pod"].dims) == ()


def same_bytes(a, b):
    assert list(a.data_vars) == list(b.data_vars)
    for k in a.data_vars:
        x, y = np.asarray(a[k].values), np.asarray(b[k].values)
        assert x.tobytes() == y.tobytes() and x.dtype == y.dtype and tuple(a[k].dims) == tuple(b[k].dims), k
