"""Hand-built LZ4 block-format streams for the chunk decoders (host ``marex_blosc_decompress_h``, device ``k_lz4_streams``
in marex_amd/csrc/marex_blosc.hip): a sequence builder, a plain decoder written from the format -- THE REFERENCE of the
decoder tests, it never calls a library -- the list of cases, a Blosc-1 frame builder around such streams, and a host
model of the device kernel's control flow with every index asserted (what ``blosc_frame_model.py`` is to the encoder).

The streams do not depend on any encoder's choices: offsets 1 .. 65 535 on both sides of the kernel's ``offset >= 64``
split, match lengths around the 8192-byte piece cut, runs longer than the 64 KiB ring, sources that straddle a ring wrap,
literal runs at the extension-byte boundaries, raw sizes at every ring size the launcher can choose."""
import functools
import random
import struct

import numpy as np

OFFSETS = (1, 2, 3, 4, 7, 63, 64, 65, 127, 128, 1023, 1024, 4095, 8191, 8192, 65534, 65535)
MATCH_LENGTHS = (4, 5, 18, 19, 20, 63, 64, 65, 273, 274, 8191, 8192, 8193, 16385, 70000, 140000)
LITERAL_LENGTHS = (0, 1, 14, 15, 16, 63, 64, 65, 269, 270, 271, 525, 70000)
#: raw sizes at the ring sizes of marex_lz4_decode_streams (1 KiB .. 64 KiB, doubling); 1 and 5 are literals only
RAW_SIZES = (1, 5, 1023, 1024, 1025, 2048, 2049, 4096, 4097, 8192, 8193, 16384, 16385, 32768, 32769, 40000, 50001, 60002,
             65535, 65536, 65537)
#: largest ``max_raw`` of every ring class: ``<= 1024`` .. ``<= 65536``, then everything longer (the ring stays at 64 KiB)
RING_CLASSES = (1024, 2048, 4096, 8192, 16384, 32768, 65536, 1 << 30)


def _ext(n: int) -> bytes:
    """Extension bytes of a length whose 4-bit field is saturated: 255 each, then the remainder (0 included)."""
    n -= 15
    return b"\xff" * (n // 255) + bytes([n % 255])


def seq(literals: bytes, offset=None, mlen=None) -> bytes:
    """One LZ4 sequence: token, literal-length extension, literals, 2-byte little-endian offset, match-length extension.
    ``offset=None``: the final sequence of a block, which ends after its literals."""
    lit = len(literals)
    m = 0 if offset is None else mlen - 4
    assert m >= 0 and (offset is None or 0 <= offset <= 0xFFFF)
    out = bytearray([(min(lit, 15) << 4) | min(m, 15)])
    if lit >= 15:
        out += _ext(lit)
    out += literals
    if offset is not None:
        out += struct.pack("<H", offset)
        if m >= 15:
            out += _ext(m)
    return bytes(out)


def ref_decode(stream: bytes) -> bytes:
    """LZ4 block -> bytes, from the format alone; matches are copied a byte at a time, so overlaps repeat as they must.
    Raises ``ValueError`` for a stream that is not a valid block."""
    out = bytearray()
    ip, n = 0, len(stream)
    while True:
        if ip >= n:
            raise ValueError("no token")
        token = stream[ip]
        ip += 1
        lit = token >> 4
        if lit == 15:
            while True:
                if ip >= n:
                    raise ValueError("cut in a literal length")
                b = stream[ip]
                ip += 1
                lit += b
                if b != 255:
                    break
        if ip + lit > n:
            raise ValueError("literals past the end")
        out += stream[ip: ip + lit]
        ip += lit
        if ip == n:
            return bytes(out)
        if ip + 2 > n:
            raise ValueError("cut in an offset")
        offset = stream[ip] | (stream[ip + 1] << 8)
        ip += 2
        mlen = (token & 15) + 4
        if mlen == 19:
            while True:
                if ip >= n:
                    raise ValueError("cut in a match length")
                b = stream[ip]
                ip += 1
                mlen += b
                if b != 255:
                    break
        if offset == 0 or offset > len(out):
            raise ValueError("offset outside the output")
        for _ in range(mlen):
            out.append(out[-offset])


def extend(stream: bytes, k: int, filler: bytes) -> bytes:
    """A valid stream that decodes to ``k`` more bytes (k == 0 or k >= 4): the final sequence of ``stream`` carries match
    nibble 0, so two offset bytes turn it into a 4-byte match (at offset 1), and ``k - 4`` literals of ``filler`` end it."""
    if k == 0:
        return stream
    assert k >= 4 and len(filler) >= k - 4
    return stream + struct.pack("<H", 1) + seq(filler[: k - 4])


def _tail(rng, n=12):
    return seq(rng.randbytes(n))


def _finish(rng, body: bytes, raw: int) -> bytes:
    """``body`` + a final literals-only sequence of 12 bytes -- of 15 where the stream would otherwise be exactly as long
    as its output: ``compressed size == raw size`` is how Blosc (and the device decoder's tables) mark a STORED stream."""
    s = body + _tail(rng)
    if len(s) == raw + 12:
        s = body + _tail(rng, 15)
    return s


@functools.lru_cache(maxsize=None)
def cases():
    """``{name: stream}``.  Treat the dict as read-only (it is cached)."""
    out = {}
    rng = random.Random(20240607)
    # offset x match length: `offset` literals, one match, the tail
    for off in OFFSETS:
        for ml in MATCH_LENGTHS:
            out[f"off{off}_ml{ml}"] = _finish(rng, seq(rng.randbytes(off), off, ml), off + ml)
    # literal lengths in a middle sequence
    for ll in LITERAL_LENGTHS:
        body = seq(rng.randbytes(20), 5, 8) + seq(rng.randbytes(ll), 11 if ll % 2 else 64 if ll >= 64 else 28, 6)
        out[f"lit{ll}"] = _finish(rng, body, 20 + 8 + ll + 6)
    # ring wrap: positions are taken modulo 65 536 in the kernel's ring
    body = seq(rng.randbytes(70000), 65535, 61040)          # op 70 000 -> 131 040
    body += seq(b"", 65535, 64)                             # dst 131 040 .. 131 104 and src 65 505 .. 65 569 straddle
    body += seq(rng.randbytes(3), 65535, 65447)             # -> 196 554
    body += seq(b"", 65530, 100)                            # dst 196 554 .. 196 654, src 131 024 .. 131 124 straddle
    body += seq(rng.randbytes(5), 65535, 66000)             # longer than the ring
    body += seq(rng.randbytes(2), 1, 70000)                 # a run longer than the ring
    body += seq(b"", 65535, 4)                              # right after it
    out["ringwrap"] = body + _tail(rng)
    # raw sizes at the ring sizes
    for n in RAW_SIZES:
        if n < 100:
            out[f"raw{n}"] = seq(rng.randbytes(n))
            continue
        m1 = (n - 70 - 12) // 2
        out[f"raw{n}"] = seq(rng.randbytes(70), 70, m1) + seq(b"", 3, n - 82 - m1) + _tail(rng)
    # seeded chains of sequences: offsets and lengths from the sets above plus uniform values
    for c in range(300):
        body, produced = bytearray(), 0
        budget = rng.choice((900, 1900, 3900, 8000, 16000, 32000, 65000, 90000))
        for _ in range(rng.randint(1, 8)):
            ll = rng.choice(LITERAL_LENGTHS[:-1]) if rng.random() < 0.6 else rng.randint(0, 600)
            if produced == 0 and ll == 0:
                ll = 1
            offs = [o for o in OFFSETS if o <= produced + ll]
            off = rng.choice(offs) if rng.random() < 0.6 else rng.randint(1, min(produced + ll, 65535))
            ml = rng.choice(MATCH_LENGTHS[:-2]) if rng.random() < 0.6 else rng.randint(4, 700)
            if produced + ll + ml > budget:
                ml = rng.randint(4, 40)
            body += seq(rng.randbytes(ll), off, ml)
            produced += ll + ml
        out[f"chain{c}"] = _finish(rng, bytes(body), produced)
    return out


@functools.lru_cache(maxsize=None)
def decoded():
    """``{name: ref_decode(stream)}`` of every case (cached: the reference is plain Python)."""
    return {k: ref_decode(s) for k, s in cases().items()}


def ring_class(raw: int) -> int:
    """Index into RING_CLASSES of a call whose ``max_raw`` is ``raw``."""
    return next(i for i, r in enumerate(RING_CLASSES) if raw <= r)


# ------------------------------------------------------------------------------------------------ Blosc-1 frames
def unshuffle(block: bytes, typesize: int) -> bytes:
    """NumPy un-shuffle of one block: plane k holds byte k of every element; a tail shorter than an element is as it is."""
    ne = len(block) // typesize
    body = np.frombuffer(block[: ne * typesize], np.uint8).reshape(typesize, ne).T.tobytes()
    return body + block[ne * typesize:]


def blosc_frame(streams, typesize: int, shuffled: bool, raw: int, leftover=None, dont_split: bool = False):
    """Blosc-1 / LZ4 frame around hand-built streams.  ``streams``: ``(compressed, decoded)`` pairs, every ``decoded``
    ``raw`` bytes long.  Split frames (``raw >= 128``, no 0x10 flag) put ``typesize`` streams in a block of
    ``typesize * raw`` bytes; with ``dont_split`` (flag 0x10) every block is one stream of ``raw`` bytes.  ``leftover``:
    one more pair, shorter than a block, as the last block (never split).  A stream that is not shorter than its output is
    stored (``cs == raw``).  Returns ``(frame, decoded bytes of the frame)``."""
    per = 1 if dont_split else typesize
    assert dont_split or raw >= 128
    assert len(streams) % per == 0 and all(len(d) == raw for _, d in streams)
    blocksize = per * raw
    assert blocksize % typesize == 0
    blocks = [streams[i: i + per] for i in range(0, len(streams), per)]
    if leftover is not None:
        assert 0 < len(leftover[1]) < blocksize
        blocks.append([leftover])
    nbytes = sum(len(d) for b in blocks for _, d in b)
    flags = (1 << 5) | (1 if shuffled else 0) | (0x10 if dont_split else 0)
    table_end = 16 + 4 * len(blocks)
    body, table, plain = bytearray(), [], bytearray()
    for b in blocks:
        table.append(table_end + len(body))
        planes = b"".join(d for _, d in b)
        for c, d in b:
            payload = c if len(c) < len(d) else d
            body += struct.pack("<i", len(payload)) + payload
        plain += unshuffle(planes, typesize) if shuffled and typesize > 1 else planes
    frame = struct.pack("<BBBBIII", 2, 1, flags, typesize, nbytes, blocksize, table_end + len(body))
    return frame + struct.pack(f"<{len(table)}i", *table) + bytes(body), bytes(plain)


def padded(names, raw: int, seed: int = 0):
    """The cases ``names`` as ``(compressed, decoded)`` pairs that all decode to ``raw`` bytes (``extend``)."""
    rng = random.Random(seed)
    cs, dec = cases(), decoded()
    filler = rng.randbytes(4096)
    out = []
    for n in names:
        k = raw - len(dec[n])
        fill = (filler * (k // 4096 + 1))[: max(k - 4, 0)]
        s = extend(cs[n], k, fill)
        out.append((s, dec[n] + (dec[n][-1:] * 4 + fill if k else b"")))
    return out


# ------------------------------------------------------------------------------------------------ host model of k_lz4_streams
def kernel_model(src: bytes, raw: int, ring_size: int):
    """The control flow of ``k_lz4_streams`` for one stream, line for line (the 64 lanes of a step are walked in order:
    every step of the kernel reads all its sources before it writes), with every index asserted: reads of the compressed
    bytes in ``[0, cs)``, writes to the slot in ``[0, raw)``.  Returns ``(slot bytes, counted in status)``; slot bytes the
    kernel does not write are 0xCD."""
    cs = len(src)
    mask = ring_size - 1
    assert ring_size & mask == 0
    ring = bytearray(ring_size)
    dst = bytearray(b"\xcd" * raw)

    def byte_at(p):
        assert 0 <= p < cs, f"read of compressed byte {p} outside [0, {cs})"
        return src[p]

    def put(p, v):
        assert 0 <= p < raw, f"write of output byte {p} outside [0, {raw})"
        ring[p & mask] = v
        dst[p] = v

    ip = op = 0
    bad = False
    while ip < cs:
        token = byte_at(ip)
        ip += 1
        lit = token >> 4
        if lit == 15:
            b = 255
            while b == 255 and ip < cs:
                b = byte_at(ip)
                ip += 1
                lit += b
        if lit > cs - ip or lit > raw - op:
            bad = True
            break
        for i in range(lit):
            put(op + i, byte_at(ip + i))
        ip += lit
        op += lit
        if ip >= cs:
            break
        if cs - ip < 2:
            bad = True
            break
        offset = byte_at(ip) | (byte_at(ip + 1) << 8)
        ip += 2
        mlen = (token & 15) + 4
        if token & 15 == 15:
            b = 255
            while b == 255 and ip < cs:
                b = byte_at(ip)
                ip += 1
                mlen += b
        if offset == 0 or offset > op or mlen > raw - op:
            bad = True
            break
        if offset >= 64:
            for base in range(0, mlen, 64):
                hi = min(base + 64, mlen)
                vals = [ring[(op - offset + i) & mask] for i in range(base, hi)]
                for i, v in zip(range(base, hi), vals):
                    put(op + i, v)
        else:
            done = 0
            while done < mlen:
                piece = min(mlen - done, 8192)
                o = op + done
                for i0 in range(0, piece, 64):
                    hi = min(i0 + 64, piece)
                    vals = [ring[(o - offset + (i % offset)) & mask] for i in range(i0, hi)]
                    for i, v in zip(range(i0, hi), vals):
                        put(o + i, v)
                done += piece
        op += mlen
    return bytes(dst), bool(bad or op != raw)


def launcher_ring(max_raw: int) -> int:
    """Ring bytes ``marex_lz4_decode_streams`` picks for ``max_raw``."""
    ring = 1024
    while ring < max_raw and ring < 65536:
        ring <<= 1
    return ring


def rejected_streams():
    """``[(name, stream, raw size of its slot)]``: streams the device decoder must count in ``status``."""
    rng = random.Random(5)
    good = seq(rng.randbytes(16), 4, 12) + seq(rng.randbytes(12))  # decodes to 40 bytes
    out = [
        ("offset_zero", seq(rng.randbytes(8), 0, 4) + seq(rng.randbytes(15)), 27),
        ("offset_before_start", seq(rng.randbytes(8), 9, 4) + seq(rng.randbytes(15)), 27),
        ("literals_past_the_stream", seq(rng.randbytes(200))[:12], 300),
        ("match_past_rawsz", seq(rng.randbytes(16), 4, 100) + seq(rng.randbytes(12)), 60),
        ("cut_in_the_offset", seq(rng.randbytes(8), 4, 4)[:-1], 24),
        ("ends_short_of_rawsz", good, 50),
    ]
    assert all(len(s) != raw for _, s, raw in out)  # equal sizes would mean "stored"
    return out
