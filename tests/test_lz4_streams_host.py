"""CPU: the hand-built LZ4 streams of ``lz4_streams.py`` are valid by an independent decoder (liblz4 through pyarrow, where
present), the host chunk decoder ``marex_blosc_decompress_h`` reads them inside Blosc-1 frames of every layout, the host
model of the device kernel decodes them and stays inside its buffers on the streams the kernel must reject, and the
planner / reader in front of the device decoder refuse what they cannot place -- before anything reaches a GPU."""
import json
import os
import struct
import sys

import numpy as np
import pytest

from marex_amd import zarr_io
from marex_amd.exceptions import DataValidationError, DependencyError

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import lz4_streams as lz  # noqa: E402


def test_case_list_covers_what_it_claims():
    cs, dec = lz.cases(), lz.decoded()
    for off in lz.OFFSETS:
        for ml in lz.MATCH_LENGTHS:
            assert len(dec[f"off{off}_ml{ml}"]) in (off + ml + 12, off + ml + 15)
    assert max(len(dec[f"off{o}_ml{m}"]) for o in lz.OFFSETS for m in lz.MATCH_LENGTHS) == 205547
    for n in lz.RAW_SIZES:
        assert len(dec[f"raw{n}"]) == n
    assert len(dec["ringwrap"]) == 332677
    assert sum(k.startswith("chain") for k in cs) == 300
    for k, s in cs.items():  # cs == raw would mean "stored" to Blosc and to the device decoder's tables
        assert len(s) != len(dec[k]), k
    assert {lz.ring_class(len(d)) for d in dec.values()} == set(range(len(lz.RING_CLASSES)))


def test_reference_decoder_equals_liblz4():
    pa = pytest.importorskip("pyarrow")
    codec = pa.Codec("lz4_raw")
    dec = lz.decoded()
    for k, s in lz.cases().items():
        assert codec.decompress(s, decompressed_size=len(dec[k])).to_pybytes() == dec[k], k


def tier_of(raw: int):
    """Common raw size the case is extended to inside a frame (an extension adds 0 or >= 4 bytes)."""
    return next((r for r in (2048, 16384, 70016, 205552) if raw == r or raw <= r - 4), None)


def names_in_tier(r):
    return [k for k, d in lz.decoded().items() if tier_of(len(d)) == r]


def whole_blocks(streams, per):
    return streams + streams[: (-len(streams)) % per]


@pytest.mark.parametrize("typesize,shuffled,dont_split", [(1, 0, 0), (2, 1, 0), (2, 0, 0), (4, 1, 0), (4, 0, 0), (8, 1, 0), (8, 0, 0),
                                                          (4, 1, 1), (8, 0, 1)])
def test_host_decoder_reads_small_streams_in_every_frame_layout(typesize, shuffled, dont_split):
    """Several blocks of ``typesize`` streams (or of one, under the 0x10 flag) and a leftover block with a ragged tail."""
    dec = lz.decoded()
    streams = whole_blocks(lz.padded(names_in_tier(2048), 2048, seed=typesize), 1 if dont_split else typesize)
    assert len(streams) >= 150
    left = (lz.cases()["lit525"], dec["lit525"])  # 571 bytes: not a multiple of 2, 4 or 8
    frame, plain = lz.blosc_frame(streams, typesize, bool(shuffled), 2048, leftover=left, dont_split=bool(dont_split))
    assert zarr_io._decompress(frame, len(plain)) == plain


@pytest.mark.parametrize("raw,typesize,shuffled,dont_split", [(16384, 4, 1, 0), (70016, 8, 1, 1), (205552, 2, 0, 0)])
def test_host_decoder_reads_long_streams(raw, typesize, shuffled, dont_split):
    streams = whole_blocks(lz.padded(names_in_tier(raw), raw, seed=raw), 1 if dont_split else typesize)
    assert len(streams) >= 20
    frame, plain = lz.blosc_frame(streams, typesize, bool(shuffled), raw, dont_split=bool(dont_split))
    assert zarr_io._decompress(frame, len(plain)) == plain


def test_host_decoder_reads_the_ring_wrap_stream_and_no_case_is_left_out():
    dec = lz.decoded()
    assert [k for k, d in dec.items() if tier_of(len(d)) is None] == ["ringwrap"]
    frame, plain = lz.blosc_frame([(lz.cases()["ringwrap"], dec["ringwrap"])], 1, False, len(dec["ringwrap"]))
    assert plain == dec["ringwrap"] and zarr_io._decompress(frame, len(plain)) == plain


def test_kernel_model_decodes_the_cases_within_its_buffers():
    """The restated control flow of k_lz4_streams (ring, 64-byte steps, 8192-byte pieces) gives the reference's bytes with
    the ring its launcher picks; every index is asserted inside the model.  Streams up to 9000 bytes and the ring-wrap
    stream (pure Python: the long ones are left to the GPU test)."""
    dec = lz.decoded()
    n = 0
    for k, s in lz.cases().items():
        raw = len(dec[k])
        if raw > 9000 and k != "ringwrap":
            continue
        for ring in {lz.launcher_ring(raw), lz.launcher_ring(lz.RING_CLASSES[lz.ring_class(raw)]), 65536}:
            got, bad = lz.kernel_model(s, raw, ring)
            assert not bad and got == dec[k], (k, ring)
        n += 1
    assert n > 300


def test_kernel_model_rejects_the_malformed_streams_without_leaving_their_slots():
    for name, s, raw in lz.rejected_streams():
        try:
            ok = len(lz.ref_decode(s)) == raw
        except ValueError:
            ok = False
        assert not ok, name
        for ring in (1024, 65536):
            slot, bad = lz.kernel_model(s, raw, ring)  # asserts every read in [0, cs) and every write in [0, raw)
            assert bad and len(slot) == raw, name


# ------------------------------------------------------------------------------------------------ plan_blosc_frame
def expected_stream_count(frame):
    """The split rule as ``independent_decode`` of test_zarr_write.py applies it."""
    _, _, flags, typesize, nbytes, blocksize, _ = struct.unpack("<BBBBIII", frame[:16])
    nblocks = (nbytes + blocksize - 1) // blocksize
    n = 0
    for j in range(nblocks):
        bsize = nbytes - j * blocksize if j == nblocks - 1 else blocksize
        leftover = bsize != blocksize
        n += typesize if (not flags & 0x10 and not leftover and typesize <= 16 and blocksize // typesize >= 128) else 1
    return n


@pytest.mark.parametrize("typesize,shuffled,dont_split,with_leftover", [(4, 1, 0, 1), (4, 0, 0, 0), (4, 1, 1, 1), (8, 0, 1, 0), (1, 0, 0, 1),
                                                                       (2, 1, 0, 0)])
def test_planner_finds_every_stream_of_split_unsplit_and_unshuffled_frames(typesize, shuffled, dont_split, with_leftover):
    names = names_in_tier(2048)[:24]
    streams = lz.padded(names, 2048)
    left = lz.padded(["lit270"], 320)[0] if with_leftover else None  # 316 -> 320 bytes: whole elements
    frame, plain = lz.blosc_frame(streams, typesize, bool(shuffled), 2048, leftover=left, dont_split=bool(dont_split))
    sh, plan, blocks = zarr_io.plan_blosc_frame(frame, typesize, len(plain))
    assert sh == (bool(shuffled) and typesize > 1)
    assert len(plan) == expected_stream_count(frame) == len(streams) + (1 if with_leftover else 0)
    pairs = streams + ([left] if with_leftover else [])
    dst = 0
    for (p, cb, d, raw), (c, dd) in zip(plan, pairs):
        assert (d, raw) == (dst, len(dd)) and frame[p: p + cb] == (c if len(c) < len(dd) else dd)
        dst += raw
    per = 1 if dont_split else typesize
    assert [b[3] for b in blocks] == [2048 * per] * (len(streams) // per) + ([320] if with_leftover else [])
    assert [b[1] for b in blocks] == [j * 2048 * per // typesize for j in range(len(blocks))]


def test_planner_refuses_blocks_that_do_not_hold_whole_elements():
    """blocksize % typesize != 0: the host decoder reads such a frame (its ``rest`` copy), the device placement cannot;
    ``DataValidationError``, as for every frame whose numbers do not fit together."""
    names = [k for k, d in lz.decoded().items() if len(d) <= 998][:4]
    streams = lz.padded(names, 1002)
    frame, plain = lz.blosc_frame(streams, 1, False, 1002, dont_split=True)
    frame = frame[:3] + b"\x04" + frame[4:]  # typesize 4: nbytes 4008 holds whole elements, blocksize 1002 does not
    assert len(plain) == 4008 and zarr_io._decompress(frame, 4008) == plain
    with pytest.raises(DataValidationError):
        zarr_io.plan_blosc_frame(frame, 4, 4008)


def test_planner_hands_a_memcpyed_frame_over_as_it_is():
    rng = np.random.default_rng(2)
    a = rng.integers(-2**31, 2**31, 3000, dtype=np.int64).astype(np.int32)
    frame = zarr_io._compress(a, 4)
    assert frame[2] & 0x2 and len(frame) == 16 + a.nbytes
    assert zarr_io.plan_blosc_frame(frame, 4, a.nbytes) == (None, [], [])
    other_codec = frame[:2] + bytes([(frame[2] & 0x1F) | (4 << 5)]) + frame[3:]  # c-blosc keeps the codec bits of the compressor asked for
    assert zarr_io.plan_blosc_frame(other_codec, 4, a.nbytes) == (None, [], [])
    with pytest.raises(DataValidationError):
        zarr_io.plan_blosc_frame(frame[:-1], 4, a.nbytes)
    cut = frame[:12] + struct.pack("<I", len(frame) - 8) + frame[16:-8]
    with pytest.raises(DataValidationError):
        zarr_io.plan_blosc_frame(cut, 4, a.nbytes)
    with pytest.raises(DependencyError):
        zarr_io.plan_blosc_frame(frame, 8, a.nbytes)


# ------------------------------------------------------------------------------------------------ read_array_to_device
class NoKernelEngine:
    """Stands in for the device engine where nothing may be launched."""

    def __init__(self):
        import torch

        self.device = torch.device("cpu")

    def call(self, name, *args):
        pytest.fail(f"{name} was called")

    def sync(self):
        pytest.fail("sync was called")


@pytest.mark.parametrize("dtype", [">f4", ">f8", ">i4", ">i2", ">i8", "<u2", "<u4", "<u8", "<f2", "<c8", "<M8[D]"])
def test_device_reader_refuses_byte_orders_and_dtypes_before_it_opens_a_chunk(tmp_path, dtype):
    """A ``.zarray`` beside no chunk files: with nothing to decode, only the check up front can raise."""
    p = tmp_path / "a"
    p.mkdir()
    meta = {"zarr_format": 2, "shape": [6, 5], "chunks": [2, 5], "dtype": dtype, "order": "C", "filters": None, "fill_value": None,
            "compressor": {"id": "blosc", "cname": "lz4", "clevel": 5, "shuffle": 1, "blocksize": 0}}
    (p / ".zarray").write_text(json.dumps(meta))
    with pytest.raises(DependencyError):
        zarr_io.read_array_to_device(str(p), NoKernelEngine())


@pytest.mark.parametrize("lead", [None, 1, 3, 4, 6, 8, 11, 12, 30])
def test_store_of_memcpyed_frames_is_read_without_a_kernel(tmp_path, lead):
    """Every chunk incompressible: the frames carry flag 0x2, and the reader places their payloads itself."""
    rng = np.random.default_rng(4)
    a = rng.integers(-2**31, 2**31, (12, 50), dtype=np.int64).astype(np.int32)
    p = str(tmp_path / "a")
    zarr_io.write_array(p, a, chunks=(4, 50))
    for ci in range(3):
        assert open(os.path.join(p, f"{ci}.0"), "rb").read()[2] & 0x2
    os.remove(os.path.join(p, "1.0"))  # a missing chunk among them: fill value null -> 0
    host = zarr_io.read_array(p)
    assert np.array_equal(host[:4], a[:4]) and np.array_equal(host[8:], a[8:])  # rows 4 .. 7: whatever np.empty held
    want = a.copy()
    want[4:8] = 0
    want = want[: lead]
    got = zarr_io.read_array_to_device(p, NoKernelEngine(), lead).numpy()
    assert got.dtype == want.dtype and got.shape == want.shape and np.array_equal(got, want)
