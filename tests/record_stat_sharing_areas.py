"""Writes tests/golden/stat_sharing_areas.npz, the fixture of tests/test_stat_sharing_host.py: what every front end hands the
host engines for ``cell_areas``, per grid.  It was run once on the code in which every front end still parsed ``cell_areas``
itself (``event_shapes`` refused the transposed form there); run on later code it records only what that code does, which is
not what the test is for.  Not collected by pytest."""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from marex_amd.exceptions import DataValidationError  # noqa: E402
from test_stat_sharing_host import GOLDEN, _case, _forms, _pairs, _reaches_engine  # noqa: E402

out = {}
for front, grid in _pairs():
    first = None
    for form, areas in _forms(grid, _case(grid)[2]).items():
        try:
            got = _reaches_engine(front, grid, areas)
        except DataValidationError as err:  # a form this front end did not take yet
            print(f"{front} {grid} {form}: refused ({err.message})")
            continue
        first = first or got
        assert all(got[k].tobytes() == first[k].tobytes() for k in first), (front, grid, form)
    out.update({f"{front}/{grid}/{k}": v for k, v in first.items()})
np.savez_compressed(GOLDEN, **out)
print(f"{len(out)} arrays, {os.path.getsize(GOLDEN)} bytes")
