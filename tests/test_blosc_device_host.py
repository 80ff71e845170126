"""Device Blosc encoder, host side: the C entry points are declared, bound and exported, and the rule the device relies on
-- encode every stream once without a cap, record its peak demand, then decide compressed / stored stream / stored frame
in one scan over the frame (tests/blosc_frame_model.py) -- reproduces ``marex_blosc_compress_h`` byte for byte, on inputs
that put peaks exactly at and one past a stream's cap and run out of room partway through a frame.  No GPU needed."""
import ctypes as C
import os
import random
import sys

import pytest

from marex_amd import _lib

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import blosc_frame_model as bfm  # noqa: E402

NEW = ("marex_blosc_compress_d", "marex_blosc_compress_work_bytes")


def host_compress(buf: bytes, typesize: int, shuffle: int = 1, blocksize: int = 0) -> bytes:
    lib = _lib.load()
    out = C.create_string_buffer(len(buf) + 16)
    n = C.c_int64(0)
    assert lib.marex_blosc_compress_h(buf, len(buf), typesize, shuffle, blocksize, out, len(buf) + 16, C.byref(n)) == 0
    return out.raw[: n.value]


def test_device_encoder_symbols_are_declared_bound_and_exported():
    from marex_amd.csrc import build

    src = open(os.path.join(os.path.dirname(HERE), "include", "marex_hip.h")).read()
    build.build(verbose=False)
    lib = _lib.load()
    for name in NEW:
        assert f"{name}(" in src, name
        assert name in _lib.PROTOTYPES, name
        assert hasattr(lib, name), name


def test_work_bytes_cover_planes_scratch_and_stream_tables():
    lib = _lib.load()
    out = C.c_int64(0)
    nb = 25 * 720 * 1440 * 4
    assert lib.marex_blosc_compress_work_bytes(nb, 4, 1, 0, 3, C.byref(out)) == 0
    streams = 3 * (nb // (256 * 1024) * 4 + 1)
    assert out.value >= 2 * 3 * nb + 16 * streams
    assert lib.marex_blosc_compress_work_bytes(nb, 1, 1, 0, 3, C.byref(out)) == 0  # typesize 1: no byte planes
    assert 3 * nb <= out.value < 2 * 3 * nb
    assert lib.marex_blosc_compress_work_bytes(-1, 4, 1, 0, 1, C.byref(out)) != 0
    assert lib.marex_blosc_compress_work_bytes(16, 0, 1, 0, 1, C.byref(out)) != 0


def _mixed(rng: random.Random, n: int, p_random: float) -> bytes:
    """Runs of random bytes and of repeats, about ``p_random`` of them random: a peak demand anywhere near the cap."""
    b = bytearray()
    while len(b) < n:
        k = rng.randint(1, 40)
        if rng.random() < p_random or len(b) < 8:
            b += bytes(rng.getrandbits(8) for _ in range(k))
        else:
            o = rng.randint(1, min(len(b), 300))
            for _ in range(k):
                b.append(b[-o])
    return bytes(b[:n])


@pytest.mark.parametrize("typesize,blocksize", [(1, 0), (4, 0), (1, 512), (2, 256), (8, 1024), (17, 0), (300, 0)])
def test_peak_and_room_scan_reproduce_the_host_encoder(typesize, blocksize):
    rng = random.Random(1000 * typesize + blocksize)
    for n in [0, 1, 4, 5, 12, 13, 14, 17, 100, 257, 1000, 1001, 2048, 3001]:
        for p in (0.0, 0.3, 0.6, 0.8, 1.0):
            buf = _mixed(rng, n, p)
            frame, _ = bfm.compress_frame(buf, typesize, 1, blocksize)
            assert frame == host_compress(buf, typesize, 1, blocksize), (n, p)


def test_peaks_at_the_cap_and_one_past_it():
    """Single-stream frames (typesize 1): room = nbytes + 16 - (16 + 4) - 4, so the stream's cap is n - 8.  Inputs are
    searched whose peak is exactly the cap (compressed) and the cap + 1 (stored frame: a stored stream needs n bytes)."""
    rng = random.Random(7)
    found = {0: 0, 1: 0}
    for _ in range(4000):
        n = rng.randint(13, 400)
        buf = _mixed(rng, n, rng.uniform(0.5, 1.0))
        d = bfm.stream_peak(buf) - (n - 8)
        if d in found:
            frame, kinds = bfm.compress_frame(buf, 1)
            assert kinds == (["lz4"] if d == 0 else ["frame"])
            assert frame == host_compress(buf, 1)
            found[d] += 1
        if min(found.values()) >= 3:
            break
    assert min(found.values()) >= 3, found


def test_room_runs_out_partway_through_a_frame():
    """Compressible blocks first, random blocks after: some random streams are still stored, then the room is gone."""
    rng = random.Random(11)
    seen = set()
    for lead in range(0, 9):
        buf = bytes(lead * 512) + bytes(rng.getrandbits(8) for _ in range(16 * 512 - lead * 512))
        frame, kinds = bfm.compress_frame(buf, 1, 1, 512)
        assert frame == host_compress(buf, 1, 1, 512), lead
        seen.add("frame" if kinds == ["frame"] else ("stored" if "stored" in kinds else "lz4"))
    assert seen == {"frame", "stored"}
