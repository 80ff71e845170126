"""GPU parity of the grid partition and relabel kernels of the merge tracker (k_mrg_part_centroid, k_mrg_nn_buckets,
k_mrg_scan, k_mrg_part_nn, k_mrg_relabel) against the host oracle on the hand-placed cases of
tests/merge_partition_cases.py: bucket counts of 1 to 3 and partial last buckets, parents shared between children, both
rules in one child, exact ties and the distance cap, bucket totals around the scan's width, a slice larger than one
launch, and the edges of the relabel tables.  Every comparison is exact (int32 fields).  tests/test_merge_partition_host.py
shows on the host that each of eleven plausible kernel mistakes changes the expected result of some case here.

The engine methods refuse tables a kernel would read past or search in vain; those refusals are tested without a launch.
"""
import os
import sys

import numpy as np
import pytest
import torch

from marex_amd.exceptions import ProcessingError

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import merge_partition_cases as mc  # noqa: E402

pytestmark = pytest.mark.gpu


def _dev(hot, a):
    return torch.from_numpy(np.ascontiguousarray(a).reshape(-1).copy()).to(hot.device)


def _partition(hot, c, nn):
    cur, prev = _dev(hot, c.cur), _dev(hot, c.prev)
    if nn:
        hot.partition_nn(cur, prev, c.ny, c.nx, c.child_keys, c.off, c.parents, c.pcy, c.pcx, c.lab, c.maxd, c.wrap)
    else:
        hot.partition_centroid(cur, c.ny, c.nx, c.child_keys, c.off, c.pcy, c.pcx, c.lab, c.wrap)
    return cur.cpu().numpy().reshape(c.ny, c.nx), prev.cpu().numpy().reshape(c.ny, c.nx)


@pytest.mark.parametrize("nn", [False, True], ids=["centroid", "nearest-cell"])
@pytest.mark.parametrize("name", mc.NAMES)
def test_partition_equals_the_oracle(hot, name, nn):
    mc.check_coverage(name)
    c = mc.get(name)
    want, _ = mc.expected(name, nn)
    got, prev = _partition(hot, c, nn)
    bad = np.argwhere(got != want)
    assert bad.size == 0, (name, len(bad), "first (y, x):", bad[0].tolist(), "got", int(got[tuple(bad[0])]),
                           "want", int(want[tuple(bad[0])]))
    other = ~np.isin(c.cur, c.child_keys)
    assert np.array_equal(got[other], c.cur[other])  # part of the comparison above, stated on its own
    assert np.array_equal(prev, c.prev)
    again, _ = _partition(hot, c, nn)  # the bucket fill orders a bucket's cells by atomics: the result must not depend on it
    assert again.tobytes() == got.tobytes()


@pytest.mark.parametrize("name", mc.RELABEL_NAMES)
def test_relabel_equals_numpy(hot, name):
    ids, vals, keys, want = mc.relabel_cases()[name]
    d = _dev(hot, ids)
    hot.relabel(d, vals, keys)
    got = d.cpu().numpy()
    bad = np.nonzero(got != want)[0]
    assert bad.size == 0, (name, len(bad), "first:", int(bad[0]), int(ids[bad[0]]), int(got[bad[0]]), int(want[bad[0]]))


@pytest.fixture
def no_library_call(hot, monkeypatch):
    def reached(name, *args):
        raise AssertionError(f"{name} was reached with arguments that should have been refused")

    monkeypatch.setattr(hot, "call", reached)
    return hot


def test_partitions_check_their_arguments_before_the_launch(no_library_call):
    hot = no_library_call
    c = mc.get("a-7x64-wrap-k3")
    cur, prev = _dev(hot, c.cur), _dev(hot, c.prev)
    ok = dict(ny=c.ny, nx=c.nx, child_keys=c.child_keys, off=c.off, parents=c.parents, pcy=c.pcy, pcx=c.pcx, lab=c.lab,
              maxd=c.maxd)

    def centroid(cur=cur, **kw):
        a = {**ok, **kw}
        hot.partition_centroid(cur, a["ny"], a["nx"], a["child_keys"], a["off"], a["pcy"], a["pcx"], a["lab"], c.wrap)

    def nearest(cur=cur, prev=prev, **kw):
        a = {**ok, **kw}
        hot.partition_nn(cur, prev, a["ny"], a["nx"], a["child_keys"], a["off"], a["parents"], a["pcy"], a["pcx"], a["lab"],
                         a["maxd"], c.wrap)

    slices = {"an int64 slice": dict(cur=cur.to(torch.int64)), "a short slice": dict(cur=cur[:-1]),
              "a strided slice": dict(cur=torch.zeros(2 * c.ny * c.nx, dtype=torch.int32, device=hot.device)[::2]),
              "a slice on the host": dict(cur=cur.cpu())}
    def untouched():
        return cur.cpu().numpy().tobytes() == c.cur.tobytes() and prev.cpu().numpy().tobytes() == c.prev.tobytes()

    for what, kw in {**mc.bad_tables(c), **slices}.items():
        for fn in (centroid, nearest):
            with pytest.raises(ProcessingError):
                fn(**kw)
                pytest.fail(f"{fn.__name__}: {what} was accepted")
            assert untouched(), (fn.__name__, what)
    for what, kw in {**mc.bad_nn_tables(c), "an int64 prev": dict(prev=prev.to(torch.int64)), "a short prev": dict(prev=prev[1:]),
                     "a float prev": dict(prev=prev.to(torch.float32))}.items():
        with pytest.raises(ProcessingError):
            nearest(**kw)
            pytest.fail(f"nearest: {what} was accepted")
        assert untouched(), what


def test_relabel_checks_its_arguments_before_the_launch(no_library_call):
    hot = no_library_call
    ids = np.arange(-3, 40, dtype=np.int32)
    d = _dev(hot, ids)
    keys, vals = np.array([3, 7, 19], np.int32), np.array([1, 2, 3], np.int32)
    bads = {what: (lambda a=a: hot.relabel(d, *a)) for what, a in mc.bad_relabel_tables().items()}
    bads.update({"int64 ids": lambda: hot.relabel(d.to(torch.int64), vals, keys),
                 "strided ids": lambda: hot.relabel(d[::2], vals, keys)})
    for what, bad in bads.items():
        with pytest.raises(ProcessingError):
            bad()
            pytest.fail(f"relabel: {what} was accepted")
        assert d.cpu().numpy().tobytes() == ids.tobytes(), what


def test_accepted_forms_of_the_tables(hot):
    """Lists, int64 arrays and a [T, C] field's row are what the tracker passes: the checks must not refuse them."""
    c = mc.get("a-7x64-wrap-k3")
    want, _ = mc.expected(c.name, True)
    field = torch.from_numpy(np.stack([c.prev, c.cur]).reshape(2, -1).copy()).to(hot.device)
    hot.partition_nn(field[1], field[0], np.int64(c.ny), np.int64(c.nx), c.child_keys.astype(np.int64), c.off.tolist(),
                     c.parents.astype(np.int64), c.pcy.tolist(), c.pcx.tolist(), c.lab.tolist(), c.maxd.tolist(), c.wrap)
    assert np.array_equal(field[1].cpu().numpy().reshape(c.ny, c.nx), want)
    ids = np.array([[1, 2, 3], [3, 0, 9]], np.int32)
    d = torch.from_numpy(ids.copy()).to(hot.device)
    hot.relabel(d, [7, 8], [2, 3])
    assert np.array_equal(d.cpu().numpy(), np.array([[1, 7, 8], [8, 0, 9]], np.int32))
    hot.relabel(d, np.zeros(0, np.int32), np.zeros(0, np.int32))  # nothing to rename
    hot.relabel(d, [])
    assert np.array_equal(d.cpu().numpy(), np.array([[1, 7, 8], [8, 0, 9]], np.int32))
