"""GPU: the device Blosc / LZ4 encoder (marex_blosc_compress_d, both variants: one wave per stream and one lane per
stream) writes every frame byte-identical to the host encoder ``marex_blosc_compress_h`` -- typesizes 1 .. 300,
blocksizes around the split rule, sizes 0 .. a few blocks, zeros / constants / random / half-random data, periods at the
LZ4 offset limit, run lengths at the token boundaries, peaks at and one past a stream's cap, frames that run out of room
partway, and seeded fuzzing -- and frames decode with pyarrow's ``lz4_raw`` codec."""
import os
import random
import sys

import numpy as np
import pytest
import torch

from marex_amd import zarr_io

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import blosc_frame_model as bfm  # noqa: E402
from test_blosc_device_host import _mixed, host_compress  # noqa: E402

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def hot():
    from marex_amd.detect import get_engine

    return get_engine(0)


def check(hot, bufs, typesize, blocksize=0, shuffle=1):
    """Equal-sized chunks in one device call, both variants, against the host encoder chunk by chunk."""
    n = len(bufs[0])
    assert all(len(b) == n for b in bufs)
    rows = torch.from_numpy(np.frombuffer(b"".join(bufs), np.uint8).reshape(len(bufs), n).copy()).to(hot.device)
    want = [host_compress(b, typesize, shuffle, blocksize) for b in bufs]
    for variant in (0, 1):
        got = zarr_io.compress_chunks_device(rows, typesize, hot, blocksize, shuffle, variant)
        for i, (g, w) in enumerate(zip(got, want)):
            assert g == w, f"variant {variant}, chunk {i}: {n} bytes, typesize {typesize}, blocksize {blocksize}"
    return want


def kinds(rng, n):
    r = bytes(rng.getrandbits(8) for _ in range(n))
    f = np.frombuffer(rng.randbytes(4 * (n // 4 + 1)), np.uint32)
    floaty = ((f & 0x007FFFFF) | 0x41200000).astype(np.uint32).tobytes()[:n]  # equal exponents, random mantissas
    return [bytes(n), b"\xab" * n, r, r[: n // 2] + bytes(n - n // 2), floaty]


@pytest.mark.parametrize("typesize", [1, 2, 4, 8, 16, 17, 300])
def test_typesizes_blocksizes_and_sizes(hot, typesize):
    rng = random.Random(typesize)
    for blocksize in (0, 4096, 128 * typesize - 1, 128 * typesize):
        for n in (0, 7, 12, 13, 5003, 3 * 4096 + 5, 300001):
            check(hot, kinds(rng, n), typesize, blocksize)


def test_unshuffled_frames(hot):
    rng = random.Random(3)
    for ts in (1, 4, 8):
        check(hot, kinds(rng, 70001), ts, 0, shuffle=0)


@pytest.mark.parametrize("period", [65535, 65536, 65537])
def test_periods_at_the_offset_limit(hot, period):
    rng = random.Random(period)
    pat = rng.randbytes(period)
    n = 256 * 1024
    buf = (pat * (n // period + 1))[:n]
    check(hot, [buf, buf[::-1]], 1)
    check(hot, [(pat * 9)[: 8 * 65536]], 4)


def test_run_lengths_at_token_and_extension_boundaries(hot):
    rng = random.Random(5)
    edges = [1, 3, 4, 5, 14, 15, 16, 17, 18, 19, 20, 268, 269, 270, 271, 272, 273, 274, 524, 525, 526, 527, 528, 529, 1000]
    bufs = []
    for lit in edges:
        b = bytearray(rng.randbytes(300))
        for m in edges:
            b += rng.randbytes(lit)
            start = len(b) - 300
            for i in range(m):
                b.append(b[start + i])
        bufs.append(bytes(b))
    n = min(len(b) for b in bufs)
    check(hot, [b[:n] for b in bufs], 1)
    check(hot, [b[:n] for b in bufs], 1, 4096)


def test_peaks_at_the_cap_and_one_past(hot):
    rng = random.Random(7)
    found = {0: [], 1: []}
    for _ in range(6000):
        n = rng.randint(13, 400)
        buf = _mixed(rng, n, rng.uniform(0.5, 1.0))
        d = bfm.stream_peak(buf) - (n - 8)
        if d in found and len(found[d]) < 6:
            found[d].append(buf)
        if min(len(v) for v in found.values()) >= 6:
            break
    assert min(len(v) for v in found.values()) >= 6
    for d, bufs in found.items():
        for b in bufs:
            frame = check(hot, [b], 1)[0]
            assert (frame[2] & 0x2) == (0x2 if d == 1 else 0)


def test_room_runs_out_partway(hot):
    rng = random.Random(11)
    bufs = [bytes(lead * 512) + rng.randbytes(16 * 512 - lead * 512) for lead in range(9)]
    frames = check(hot, bufs, 1, 512)
    assert any(f[2] & 0x2 for f in frames) and not all(f[2] & 0x2 for f in frames)
    # float-like streams with a few compressible planes: stored streams inside compressed frames
    check(hot, [kinds(rng, 64 * 1024)[4] for _ in range(4)], 4, 4096)


def test_seeded_fuzz(hot):
    rng = random.Random(2024)
    for _ in range(60):
        ts = rng.choice([1, 2, 3, 4, 8, 12, 16, 17, 300])
        n = rng.choice([rng.randint(0, 64), rng.randint(13, 5000), rng.randint(5000, 600000)])
        bs = rng.choice([0, 0, rng.randint(1, 70000)])
        bufs = [_mixed(rng, n, rng.random()) if n < 20000 else
                np.repeat(np.frombuffer(rng.randbytes(n // 7 + 1), np.uint8), 7)[:n].tobytes() for _ in range(rng.randint(1, 4))]
        check(hot, bufs, ts, bs, shuffle=rng.choice([0, 1]))


def test_frames_decode_with_pyarrow_and_the_host_decoder(hot):
    pytest.importorskip("pyarrow")
    from test_zarr_write import independent_decode

    rng = np.random.default_rng(9)
    x = rng.normal(size=(6, 72, 144)).astype(np.float32)
    x[:, :10] = np.nan
    x[x > 1.5] = 0
    rows = torch.from_numpy(x.view(np.uint8).reshape(6, -1).copy()).to(hot.device)
    for i, f in enumerate(zarr_io.compress_chunks_device(rows, 4, hot)):
        assert independent_decode(f) == x[i].tobytes()
        assert zarr_io._decompress(f, x[i].nbytes) == x[i].tobytes()


def test_many_chunks_in_one_call(hot):
    """A batch of float32 chunks shaped like the reference's output chunks (25 x 72 x 144 here): chunk offsets and
    per-chunk frame placement."""
    rng = np.random.default_rng(1)
    x = np.round(rng.normal(size=(12, 25, 72, 144)), 1).astype(np.float32)
    x[rng.random(x.shape) < 0.5] = 0
    x[3] = np.nan
    x[7] = rng.random(x[7].shape).astype(np.float32)
    bufs = [x[i].tobytes() for i in range(12)]
    check(hot, bufs, 4)
    m = (rng.random((9, 25, 72, 144)) < 0.05)
    check(hot, [m[i].tobytes() for i in range(9)], 1)
