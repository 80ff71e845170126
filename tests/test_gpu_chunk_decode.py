"""GPU: the device chunk decoder -- ``marex_lz4_decode_streams`` (k_lz4_streams, k_stored_streams) and
``marex_unshuffle_place`` -- bit for bit against the plain decoder of ``lz4_streams.py`` and NumPy, on hand-built streams
that no encoder of ours writes: every offset class of the kernel against match lengths around its piece cut, runs longer
than the ring, sources across a ring wrap, raw sizes at every ring size, seeded chains; streams it must reject (cleared by
the host model first); tables of more than 65 535 streams / blocks; and ``read_array_to_device`` on stores assembled from
such frames, for every dtype, chunking, ``lead``, separator, fill value, and a store with a memcpyed frame in it."""
import json
import os
import random
import struct
import sys

import numpy as np
import pytest
import torch

from marex_amd import zarr_io
from marex_amd.exceptions import DataValidationError

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import lz4_streams as lz  # noqa: E402

pytestmark = pytest.mark.gpu

GUARD = 64
SENTINEL = 0xCD


def decode_streams(hot, items, seed=0):
    """One ``marex_lz4_decode_streams`` call.  ``items``: ``(stream bytes, raw size)``; a stream as long as its raw size is
    a stored one.  Streams sit at unaligned offsets of the compressed buffer, slots are ``GUARD`` sentinel bytes apart.
    Returns ``(planes as NumPy, status, slot offsets)``."""
    rng = random.Random(seed)
    blob, src = bytearray(), []
    for c, _ in items:
        blob += rng.randbytes(rng.randint(1, 7))
        src.append(len(blob))
        blob += c
    blob += rng.randbytes(3)
    dst, pos = [], GUARD
    for _, raw in items:
        dst.append(pos)
        pos += raw + GUARD
    dev = hot.device
    planes = torch.full((pos,), SENTINEL, dtype=torch.uint8, device=dev)
    status = torch.zeros(1, dtype=torch.int32, device=dev)
    comp = torch.frombuffer(blob, dtype=torch.uint8).to(dev)
    tab = lambda a, dt: torch.from_numpy(np.asarray(a, dtype=dt)).to(dev)  # noqa: E731
    raws = [raw for _, raw in items]
    hot.call("marex_lz4_decode_streams", comp, tab(src, np.int64), tab([len(c) for c, _ in items], np.int32), tab(dst, np.int64),
             tab(raws, np.int32), len(items), max(raws), planes, status)
    hot.sync()
    return planes.cpu().numpy(), int(status.item()), dst


def assert_slots(planes, dst, want, names):
    """Every slot holds its expected bytes and every byte between the slots is still the sentinel."""
    guard = np.ones(planes.size, dtype=bool)
    for o, w, n in zip(dst, want, names):
        got = planes[o: o + len(w)].tobytes()
        if got != w:
            bad = next(i for i in range(len(w)) if got[i] != w[i])
            raise AssertionError(f"{n}: {len(w)} bytes, first difference at byte {bad}")
        guard[o: o + len(w)] = False
    assert (planes[guard] == SENTINEL).all(), "a guard band was written"


def with_stored(names, max_raw, seed):
    """``(labels, items, expected)``: the cases ``names`` with a stored stream (random bytes, ``csize == rawsz``) after
    the second of every four."""
    rng = random.Random(seed)
    cs, dec = lz.cases(), lz.decoded()
    labels, items, want = [], [], []
    for i, n in enumerate(names):
        labels.append(n)
        items.append((cs[n], len(dec[n])))
        want.append(dec[n])
        if i % 4 == 1:
            b = rng.randbytes(rng.choice((1, 63, 64, 255, 256, 257, min(max_raw, 70001), rng.randint(1, min(max_raw, 70001)))))
            labels.append(f"stored after {n}")
            items.append((b, len(b)))
            want.append(b)
    return labels, items, want


@pytest.mark.parametrize("klass", range(len(lz.RING_CLASSES)))
def test_streams_of_one_ring_class_in_one_call(hot, klass):
    """All cases whose raw size picks this ring, so ``max_raw`` is the class's largest (1024 .. 65 536 exactly; the last
    class keeps the 64 KiB ring under streams of up to 332 677 bytes)."""
    dec = lz.decoded()
    names = [k for k, d in dec.items() if lz.ring_class(len(d)) == klass]
    top = max(len(dec[k]) for k in names)
    assert top == (lz.RING_CLASSES[klass] if klass < 7 else 332677) and lz.launcher_ring(top) == min(1024 << klass, 65536)
    labels, items, want = with_stored(names, top, klass)
    assert len(names) >= 6 and any(len(c) == r for c, r in items)
    planes, status, dst = decode_streams(hot, items, seed=klass)
    assert status == 0
    assert_slots(planes, dst, want, labels)


def test_a_tiny_stream_under_the_64k_ring(hot):
    dec = lz.decoded()
    names = ["raw5", "off65535_ml140000", "raw1"]
    assert len(dec[names[1]]) == 205547
    planes, status, dst = decode_streams(hot, [(lz.cases()[n], len(dec[n])) for n in names], seed=9)
    assert status == 0
    assert_slots(planes, dst, [dec[n] for n in names], names)


def test_rejected_streams_are_counted_and_stay_in_their_slots(hot):
    """The status contract behind ``read_array_to_device``'s ``DataValidationError``.  Every malformed stream is first run
    through the host model of the kernel (its reads within the stream, its writes within the slot, and counted); the device
    must count all six, leave what the model leaves in their slots, and decode the valid streams around them."""
    dec = lz.decoded()
    valid = ["lit15", "off64_ml65", "raw1023", "off3_ml273", "chain0", "raw5", "lit270"]
    labels, items, want = [], [], []
    rejected = lz.rejected_streams()
    for n, (name, s, raw) in zip(valid, rejected):
        labels += [n, name]
        items += [(lz.cases()[n], len(dec[n])), (s, raw)]
        want += [dec[n], None]
    labels.append(valid[-1])
    items.append((lz.cases()[valid[-1]], len(dec[valid[-1]])))
    want.append(dec[valid[-1]])
    ring = lz.launcher_ring(max(r for _, r in items))
    for i, (s, raw) in enumerate(items):
        slot, bad = lz.kernel_model(s, raw, ring)  # asserts the indices
        assert bad == (want[i] is None), labels[i]
        if bad:
            want[i] = slot
    assert sum(w is not None for w in want) == len(items) and len(rejected) == 6
    planes, status, dst = decode_streams(hot, items, seed=11)
    assert status == 6
    assert_slots(planes, dst, want, labels)


def test_seventy_thousand_streams_in_one_call(hot):
    """More streams than a grid's y extent holds (65 535): 16 raw bytes each, every seventh stored."""
    rng = random.Random(70000)
    kinds = []
    for _ in range(251):
        s = lz.seq(rng.randbytes(1), 1, 9) + lz.seq(rng.randbytes(6))
        kinds.append((s, lz.ref_decode(s)))
        b = rng.randbytes(16)
        kinds.append((b, b))
    assert all(len(d) == 16 for _, d in kinds)
    n = 70000
    pick = [2 * ((i * 7919) % 251) + (1 if i % 7 == 6 else 0) for i in range(n)]
    items = [(kinds[k][0], 16) for k in pick]
    planes, status, dst = decode_streams(hot, items, seed=1)
    assert status == 0
    want = np.frombuffer(b"".join(kinds[k][1] for k in pick), np.uint8).reshape(n, 16)
    slots = planes[GUARD:].reshape(n, 16 + GUARD)
    assert dst[1] - dst[0] == 16 + GUARD
    assert np.array_equal(slots[:, :16], want)
    assert (slots[:, 16:] == SENTINEL).all() and (planes[:GUARD] == SENTINEL).all()


# ------------------------------------------------------------------------------------------------ marex_unshuffle_place
def place(hot, planes, blocks, typesize, shuffled, n_out):
    """One ``marex_unshuffle_place`` call over ``blocks`` = ``(plane offset, first element, elements, valid elements)``
    into ``n_out`` poisoned elements; returns ``(device result, NumPy expectation)`` as ``[n_out, typesize]`` bytes."""
    dev = hot.device
    for off, e0, ne, valid in blocks:  # the kernel trusts its tables
        assert 0 <= valid <= ne and off >= 0 and off + ne * typesize <= planes.size and e0 >= 0 and e0 + valid <= n_out
    want = np.full((n_out, typesize), SENTINEL, np.uint8)
    for off, e0, ne, valid in blocks:
        p = planes[off: off + ne * typesize]
        el = p.reshape(typesize, ne).T if shuffled else p.reshape(ne, typesize)
        want[e0: e0 + valid] = el[:valid]
    out = torch.full((n_out * typesize,), SENTINEL, dtype=torch.uint8, device=dev)
    tab = lambda k, dt: torch.from_numpy(np.asarray([b[k] for b in blocks], dtype=dt)).to(dev)  # noqa: E731
    hot.call("marex_unshuffle_place", torch.from_numpy(planes).to(dev), tab(0, np.int64), tab(1, np.int64), tab(2, np.int32),
             tab(3, np.int32), len(blocks), max(b[2] for b in blocks), typesize, int(shuffled), out)
    hot.sync()
    return out.cpu().numpy().reshape(n_out, typesize), want


@pytest.mark.parametrize("shuffled", [1, 0])
@pytest.mark.parametrize("typesize", [1, 2, 3, 4, 8, 16])
def test_unshuffle_place_against_numpy(hot, typesize, shuffled):
    """Blocks of different sizes in one call (the largest, 1000 elements, is no multiple of 256), valid counts 0, 1,
    ne - 1 and ne, destinations out of order with gaps; what no block covers keeps the poison."""
    rng = np.random.default_rng(typesize * 2 + shuffled)
    nes = [300, 1, 257, 1000, 77, 513, 256, 2, 64, 999]
    valids = [300, 1, 0, 999, 1, 513, 255, 0, 63, 1]
    assert all(v in (0, 1, ne - 1, ne) for v, ne in zip(valids, nes))
    offs, pos = [], 5
    for ne in nes:  # planes of the blocks with odd gaps between them
        offs.append(pos)
        pos += ne * typesize + 3
    planes = rng.integers(0, 256, pos, dtype=np.uint8)
    order = [7, 2, 9, 0, 4, 1, 8, 3, 6, 5]
    e0s, e = [0] * len(nes), 2
    for b in order:  # destinations: in this order, three free elements between them
        e0s[b] = e
        e += nes[b] + 3
    got, want = place(hot, planes, list(zip(offs, e0s, nes, valids)), typesize, shuffled, e + 4)
    assert (want == SENTINEL).all(axis=1).sum() >= 3 * len(nes)
    assert np.array_equal(got, want)


def test_seventy_thousand_blocks_in_one_call(hot):
    n, ts = 70000, 4
    rng = np.random.default_rng(7)
    planes = rng.integers(0, 256, n * ts, dtype=np.uint8)
    e0 = rng.permutation(n)
    got, want = place(hot, planes, [(ts * b, int(e0[b]), 1, 1) for b in range(n)], ts, 1, n)
    assert np.array_equal(got, want)


# ------------------------------------------------------------------------------------------------ read_array_to_device
R = 2048  # bytes per stream of the stores below: every case up to 2044 bytes, extended to 2048


def pool():
    return lz.padded([k for k, d in lz.decoded().items() if len(d) == R or len(d) <= R - 4], R, seed=1)


def write_store(path, dtype, shape, chunks, frames, sep=".", fill=None):
    """A Zarr v2 array directory around ready-made chunk files (``frames[ci]`` None: no file)."""
    os.makedirs(path, exist_ok=True)
    dt = np.dtype(dtype)
    zd = "|b1" if dt == np.bool_ else (dt.str if dt.itemsize > 1 else "|" + dt.str[1:])
    meta = {"zarr_format": 2, "shape": list(shape), "chunks": list(chunks), "dtype": zd, "order": "C", "filters": None,
            "fill_value": fill, "compressor": {"id": "blosc", "cname": "lz4", "clevel": 5, "shuffle": 1, "blocksize": 0}}
    if sep != ".":
        meta["dimension_separator"] = sep
    with open(os.path.join(path, ".zarray"), "w") as f:
        json.dump(meta, f)
    for ci, fr in enumerate(frames):
        if fr is None:
            continue
        name = os.path.join(path, *sep.join([str(ci)] + ["0"] * (len(shape) - 1)).split("/"))
        os.makedirs(os.path.dirname(name), exist_ok=True)
        with open(name, "wb") as f:
            f.write(fr)


def hand_built(dtype, T, ct, start=0, shuffled=True, dont_split=False, one_d=False):
    """Chunks of ``ct`` rows of 2048 elements (1-D: ``ct`` elements, a multiple of 2048): every row is one block of
    ``itemsize`` hand-built streams of 2048 bytes.  Returns ``(frames, source array [T, 2048] or [T])``."""
    ts = np.dtype(dtype).itemsize
    p = pool()
    rows = ct // R if one_d else ct
    nchunks = (T + ct - 1) // ct
    frames, plains = [], []
    for ci in range(nchunks):
        streams = [p[(start + (ci * rows * ts + i) * 5) % len(p)] for i in range(rows * ts)]
        # split: a row is one block of itemsize streams; under the 0x10 flag it is itemsize blocks of one stream
        fr, plain = lz.blosc_frame(streams, ts, shuffled, R, dont_split=dont_split)
        frames.append(fr)
        plains.append(plain)
    a = np.frombuffer(b"".join(plains), np.dtype(dtype))
    return frames, (a[:T] if one_d else a.reshape(-1, R)[:T])


def same_bytes(dev, host):
    """Bit for bit (NaN payloads and bool bytes included)."""
    d = dev.cpu().numpy()
    assert d.dtype == host.dtype and d.shape == host.shape, (d.dtype, d.shape, host.dtype, host.shape)
    return np.array_equal(np.ascontiguousarray(d).view(np.uint8), np.ascontiguousarray(host).view(np.uint8))


@pytest.mark.parametrize("dtype", ["float32", "float64", "int32", "int64", "int16", "int8", "uint8", "bool"])
def test_store_of_hand_built_frames_for_every_dtype(hot, tmp_path, dtype):
    T, ct = 7, 3
    frames, a = hand_built(dtype, T, ct, start=len(dtype))
    p = str(tmp_path / "a")
    write_store(p, dtype, (T, R), (ct, R), frames)
    host = zarr_io.read_array(p)
    assert same_bytes(torch.from_numpy(host), a)
    for lead in (None, 4):
        dev = zarr_io.read_array_to_device(p, hot, lead)
        assert dev.is_cuda and same_bytes(dev, a[:lead]), lead


@pytest.mark.parametrize("ct", [1, 3, 10])
def test_chunk_lengths_and_leads(hot, tmp_path, ct):
    """Chunks of one step, of a length that does not divide T, and longer than T; ``lead`` of 1, inside a chunk, at a chunk
    boundary, T, and beyond T."""
    T = 7
    frames, a = hand_built("float32", T, ct, start=ct)
    p = str(tmp_path / "a")
    write_store(p, "float32", (T, R), (ct, R), frames, fill="NaN")
    host = zarr_io.read_array(p)
    assert same_bytes(torch.from_numpy(host), a)
    for lead in (None, 1, 2, 4, 5, {1: 3, 3: 6, 10: 7}[ct], T, T + 1, 100):
        dev = zarr_io.read_array_to_device(p, hot, lead)
        assert same_bytes(dev, a[:lead]), lead


def test_one_dimensional_arrays_and_the_slash_separator(hot, tmp_path):
    T = 5000
    frames, a = hand_built("int32", T, R, one_d=True)
    assert len(frames) == 3
    p = str(tmp_path / "one_d")
    write_store(p, "int32", (T,), (R,), frames)
    assert same_bytes(torch.from_numpy(zarr_io.read_array(p)), a)
    for lead in (None, 1, 2048, 3000, T):
        assert same_bytes(zarr_io.read_array_to_device(p, hot, lead), a[:lead]), lead
    frames, a = hand_built("int16", 5, 2, start=3)
    p = str(tmp_path / "slash")
    write_store(p, "int16", (5, R), (2, R), frames, sep="/")
    assert os.path.exists(os.path.join(p, "2", "0"))
    assert same_bytes(torch.from_numpy(zarr_io.read_array(p)), a)
    for lead in (None, 3):
        assert same_bytes(zarr_io.read_array_to_device(p, hot, lead), a[:lead]), lead


def test_unshuffled_and_unsplit_frames_in_a_store(hot, tmp_path):
    for k, (shuffled, dont_split) in enumerate([(False, False), (True, True), (False, True)]):
        frames, a = hand_built("float64", 5, 2, start=k, shuffled=shuffled, dont_split=dont_split)
        p = str(tmp_path / f"a{k}")
        write_store(p, "float64", (5, R), (2, R), frames)
        assert same_bytes(torch.from_numpy(zarr_io.read_array(p)), a)
        assert same_bytes(zarr_io.read_array_to_device(p, hot), a), (shuffled, dont_split)


def test_frames_of_another_encoder_in_a_store(hot, tmp_path):
    """Streams of liblz4's encoder (through pyarrow, where that package is present; the hand-built frames of the tests
    around this one need nothing) and, in any case, frames of our own host encoder around the same field."""
    rng = np.random.default_rng(3)
    a = np.round(rng.normal(size=(64, 1024)), 1).astype(np.float32)
    p = str(tmp_path / "ours")
    zarr_io.write_array(p, a, chunks=(16, 1024))
    assert same_bytes(zarr_io.read_array_to_device(p, hot, 40), a[:40])
    try:
        import pyarrow as pa
    except ImportError:
        return
    codec = pa.Codec("lz4_raw")
    frames = []
    for ci in range(4):
        planes = a[16 * ci: 16 * ci + 16].view(np.uint8).reshape(-1, 4).T.copy()
        streams = [(codec.compress(planes[k].tobytes(), asbytes=True), planes[k].tobytes()) for k in range(4)]
        fr, plain = lz.blosc_frame(streams, 4, True, planes.shape[1])
        assert plain == a[16 * ci: 16 * ci + 16].tobytes()
        frames.append(fr)
    p = str(tmp_path / "theirs")
    write_store(p, "float32", a.shape, (16, 1024), frames, fill="NaN")
    assert same_bytes(torch.from_numpy(zarr_io.read_array(p)), a)
    for lead in (None, 17):
        assert same_bytes(zarr_io.read_array_to_device(p, hot, lead), a[:lead])


@pytest.mark.parametrize("dtype,fill,value", [("float32", None, np.nan), ("float32", "NaN", np.nan), ("float32", 2.5, 2.5),
                                              ("float64", "-Infinity", -np.inf), ("int32", None, 0), ("int32", 7, 7), ("uint8", 255, 255)])
def test_missing_chunk_files_take_the_fill_value(hot, tmp_path, dtype, fill, value):
    T, ct = 8, 3
    frames, a = hand_built(dtype, T, ct, start=2)
    want = a.copy()
    want[3:6] = value
    frames[1] = None
    p = str(tmp_path / "a")
    write_store(p, dtype, (T, R), (ct, R), frames, fill=fill)
    host = zarr_io.read_array(p)  # without a fill value the host reader leaves the rows of a missing chunk as allocated
    rows = [0, 1, 2, 6, 7] if fill is None else list(range(T))
    assert same_bytes(torch.from_numpy(host[rows]), want[rows])
    for lead in (None, 4, 2):
        assert same_bytes(zarr_io.read_array_to_device(p, hot, lead), want[:lead]), lead
    write_store(p + "_none", dtype, (T, R), (ct, R), [None] * 3, fill=fill)
    assert same_bytes(zarr_io.read_array_to_device(p + "_none", hot), np.full((T, R), value, np.dtype(dtype)))


def test_store_with_a_memcpyed_frame_among_lz4_frames(hot, tmp_path):
    """What ``write_array`` writes for a field with one incompressible chunk reads back on the device."""
    rng = np.random.default_rng(8)
    a = rng.integers(0, 3, (14, 3000)).astype(np.int32)
    a[4:8] = rng.integers(-2**31, 2**31, (4, 3000), dtype=np.int64).astype(np.int32)
    p = str(tmp_path / "a")
    zarr_io.write_array(p, a, chunks=(4, 3000))
    flags = [open(os.path.join(p, f"{ci}.0"), "rb").read()[2] for ci in range(4)]
    assert flags[1] & 0x2 and not any(f & 0x2 for f in (flags[0], flags[2], flags[3])) and flags[0] & 0x1
    host = zarr_io.read_array(p)
    assert np.array_equal(host, a)
    for lead in (None, 4, 5, 7, 8, 9, 14):
        dev = zarr_io.read_array_to_device(p, hot, lead)
        assert same_bytes(dev, a[:lead]), lead


def test_a_stream_that_ends_short_raises_from_the_reader(hot, tmp_path):
    """One launch: a frame whose only stream decodes to 40 of its 50 bytes (cleared by the host model) ->
    ``DataValidationError``."""
    name, s, raw = lz.rejected_streams()[-1]
    assert name == "ends_short_of_rawsz"
    slot, bad = lz.kernel_model(s, raw, lz.launcher_ring(raw))
    assert bad and len(slot) == raw
    frame = struct.pack("<BBBBIII", 2, 1, 0x20, 1, raw, raw, 16 + 4 + 4 + len(s)) + struct.pack("<ii", 20, len(s)) + s
    p = str(tmp_path / "a")
    write_store(p, "uint8", (1, raw), (1, raw), [frame])
    with pytest.raises(DataValidationError):
        zarr_io.read_array_to_device(p, hot)
