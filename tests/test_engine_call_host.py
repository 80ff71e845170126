"""``HotPath.call``, the one way from the engine to ``libmarex_hip.so``, against a recording stub (no device)."""
import pytest
import torch

from marex_amd.engine import HotPath
from marex_amd.exceptions import ProcessingError


class _Ctx:
    handle = object()

    def __init__(self, log):
        self.log = log

    def check(self, rc, what):
        self.log.append(("check", rc, what))
        if rc != 0:
            raise ProcessingError(f"{what} failed (code {rc})", details="stub")


class _Lib:
    def __init__(self, log, rc=0):
        self.log, self.rc = log, rc

    def __getattr__(self, name):
        if not name.startswith("marex_"):
            raise AttributeError(name)

        def fn(*args):
            self.log.append((name, args))
            return self.rc

        return fn


def _engine(device="cpu", rc=0):
    log = []
    hot = HotPath.__new__(HotPath)
    hot.device = torch.device(device)
    hot.ctx, hot.lib = _Ctx(log), _Lib(log, rc)
    hot._bind_stream = lambda: log.append("bind")
    return hot, log


def test_handle_first_tensors_as_addresses_none_as_null_and_the_rest_untouched():
    hot, log = _engine()
    a = torch.arange(12, dtype=torch.float32).reshape(3, 4)
    row = torch.zeros((5, 4), dtype=torch.int32)[2]  # a row slice: contiguous, not at the start of its storage
    assert hot.call("marex_xyz", a, 3, None, row, 0.25, int(bool(True))) is None
    assert log == ["bind", ("marex_xyz", (hot.ctx.handle, a.data_ptr(), 3, None, row.data_ptr(), 0.25, 1)),
                   ("check", 0, "marex_xyz")]
    assert row.data_ptr() != row.untyped_storage().data_ptr()


def test_the_stream_is_bound_before_every_call():
    hot, log = _engine()
    hot.call("marex_one", torch.zeros(2))
    hot.call("marex_two")
    assert [e if e == "bind" else e[0] for e in log] == ["bind", "marex_one", "check", "bind", "marex_two", "check"]


def test_an_error_code_raises_with_the_name_of_the_called_function():
    hot, log = _engine(rc=3)
    with pytest.raises(ProcessingError, match=r"marex_fixed_baseline_sub_f32 failed \(code 3\)"):
        hot.call("marex_fixed_baseline_sub_f32", torch.zeros(4), 4)
    assert log[1][0] == "marex_fixed_baseline_sub_f32" and log[-1] == ("check", 3, "marex_fixed_baseline_sub_f32")


@pytest.mark.parametrize("bad", ["transposed", "strided", "column"])
def test_a_non_contiguous_tensor_never_reaches_the_library(bad):
    hot, log = _engine()
    base = torch.zeros((6, 8))
    t = {"transposed": base.t(), "strided": base[::2], "column": base[:, 1]}[bad]
    assert not t.is_contiguous()
    with pytest.raises(ProcessingError, match=r"marex_xyz: argument 2 must be a contiguous tensor on cpu"):
        hot.call("marex_xyz", base, t, 7)
    assert log == ["bind"]


@pytest.mark.parametrize("device", ["cuda:0", "meta"])
def test_a_tensor_of_another_device_never_reaches_the_library(device):
    hot, log = _engine(device)
    other = torch.zeros(4)
    with pytest.raises(ProcessingError, match=r"marex_xyz: argument 1 must be a contiguous tensor on " + device) as exc:
        hot.call("marex_xyz", other, None)
    assert "cpu" in str(exc.value.details)
    assert log == ["bind"]
    if device == "cuda:0":  # and a meta tensor (an address of nothing) against the cuda:0 engine
        with pytest.raises(ProcessingError, match="argument 3"):
            hot.call("marex_xyz", None, 1, torch.zeros(4, device="meta"))
        assert log == ["bind", "bind"]


def test_an_unknown_function_is_an_error_not_a_fallback():
    hot, log = _engine()
    with pytest.raises(AttributeError):
        hot.call("not_a_library_function", 1)
