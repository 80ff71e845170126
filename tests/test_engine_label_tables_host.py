"""``engine.label_tables``, the one check of the label vectors of the per-cell streaming calls (no device)."""
import numpy as np
import pytest

from marex_amd.engine import label_tables
from marex_amd.exceptions import ProcessingError

WHATS = ["occurrence", "local_intensity"]


def refused(what, specs, message, details):
    with pytest.raises(ProcessingError) as exc:
        label_tables(what, specs)
    assert exc.value.message == message and exc.value.details == details


@pytest.mark.parametrize("what", WHATS)
def test_anything_but_an_integer_vector_of_the_length_is_refused(what):
    refused(what, [("grp", np.zeros(4, np.float32), None)], f"{what}: grp must be a vector of int32 values", "got float32 (4,)")
    refused(what, [("sgrp", np.zeros((2, 3), np.int32), None)], f"{what}: sgrp must be a vector of int32 values",
            "got int32 (2, 3)")
    refused(what, [("grp", None, None), ("cls", np.zeros(6, np.int32), 7)],
            f"{what}: cls must be a vector of int32 values of length 7", "got int32 (6,)")


@pytest.mark.parametrize("what", WHATS)
@pytest.mark.parametrize("value", [2**31, -2**31 - 1])
def test_a_value_outside_int32_is_refused(what, value):
    refused(what, [("doy", np.array([0, value, 1], np.int64), None)], f"{what}: doy must be a vector of int32 values",
            "got int64 (3,)")
    refused(what, [("cls", np.array([0, value, 1], np.int64), 3)], f"{what}: cls must be a vector of int32 values of length 3",
            "got int64 (3,)")


@pytest.mark.parametrize("what", WHATS)
def test_integers_in_range_become_int32_and_none_passes_through(what):
    v = np.array([-2**31, -1, 0, 7, 2**31 - 1], np.int64)
    tabs = label_tables(what, [("grp", v, None), ("sgrp", None, None), ("cls", [3, 1, 2], 3),
                               ("doy", np.zeros(0, np.uint16), None)])
    assert list(tabs) == ["grp", "sgrp", "cls", "doy"] and tabs["sgrp"] is None
    assert tabs["grp"].dtype == np.int32 and tabs["grp"].tolist() == v.tolist()
    assert tabs["cls"].dtype == np.int32 and tabs["cls"].tolist() == [3, 1, 2]
    assert tabs["doy"].dtype == np.int32 and tabs["doy"].shape == (0,)
    assert v.dtype == np.int64  # the caller's array is not touched
