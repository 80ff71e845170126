"""NumPy-free restatement of how ``marex_blosc_compress_h`` (marex_amd/csrc/marex_blosc.hip) builds a Blosc-1 / LZ4 frame,
written the way the device encoder builds it: every LZ4 stream is encoded once WITHOUT a cap while its peak demand
(max over emits of bytes written + the emit's upper bound) is recorded, and one scan over the streams of the frame then
applies the room rule.  Pure Python, for small inputs: the CPU tests check it against the host encoder, and the GPU tests
use it to find inputs whose peak demand sits exactly at a stream's cap."""
import struct

HLOG = 13


def _rd32(b, i):
    return b[i] | (b[i + 1] << 8) | (b[i + 2] << 16) | (b[i + 3] << 24)


def _hash(v):
    return ((v * 2654435761) & 0xFFFFFFFF) >> (32 - HLOG)


def lz4_encode_uncapped(src: bytes):
    """``(compressed bytes, peak demand)`` of lz4_block_encode on ``src`` with an unlimited cap."""
    n = len(src)
    table = [-1] * (1 << HLOG)
    out = bytearray()
    peak = 0
    anchor = ip = 0

    def emit(lit, mlen, offset):
        nonlocal peak
        need = 1 + lit // 255 + 1 + lit + (2 + mlen // 255 + 1 if mlen else 0)
        peak = max(peak, len(out) + need)
        m = mlen - 4 if mlen else 0
        out.append((min(lit, 15) << 4) | (min(m, 15) if mlen else 0))
        if lit >= 15:
            r = lit - 15
            out.extend(b"\xff" * (r // 255))
            out.append(r % 255)
        out.extend(src[anchor: anchor + lit])
        if mlen:
            out.extend(struct.pack("<H", offset))
            if m >= 15:
                r = m - 15
                out.extend(b"\xff" * (r // 255))
                out.append(r % 255)

    if n >= 13:
        mflimit, matchlimit = n - 12, n - 5
        misses = 0
        while ip <= mflimit:
            v = _rd32(src, ip)
            h = _hash(v)
            cand = table[h]
            table[h] = ip
            if cand < 0 or ip - cand > 65535 or _rd32(src, cand) != v:
                ip += 1 + (misses >> 6)
                misses += 1
                continue
            misses = 0
            s, c = ip, cand
            while s > anchor and c > 0 and src[s - 1] == src[c - 1]:
                s -= 1
                c -= 1
            e, ce = ip + 4, cand + 4
            while e < matchlimit and src[e] == src[ce]:
                e += 1
                ce += 1
            emit(s - anchor, e - s, s - c)
            anchor = ip = e
            if ip - 2 > cand and ip - 2 <= mflimit:
                table[_hash(_rd32(src, ip - 2))] = ip - 2
    emit(n - anchor, 0, 0)
    return bytes(out), peak


def geometry(nbytes: int, typesize: int, shuffle: int = 1, blocksize: int = 0):
    """The frame rules: ``(typesize, blocksize, do_shuffle, [(block offset, block bytes, streams)])``."""
    if typesize > 255:
        typesize = 1
    if blocksize <= 0:
        blocksize = 256 * 1024
    if blocksize > nbytes > 0:
        blocksize = nbytes
    if blocksize > typesize:
        blocksize -= blocksize % typesize
    do_shuffle = bool(shuffle) and typesize > 1
    blocks = []
    nblocks = (nbytes + blocksize - 1) // blocksize if nbytes else 0
    for j in range(nblocks):
        bsize = nbytes - j * blocksize if (j == nblocks - 1 and nbytes % blocksize) else blocksize
        leftover = bsize != blocksize
        split = not leftover and typesize <= 16 and blocksize // typesize >= 128 and bsize % typesize == 0
        blocks.append((j * blocksize, bsize, typesize if split else 1))
    return typesize, blocksize, do_shuffle, blocks


def shuffle_block(b: bytes, typesize: int) -> bytes:
    ne = len(b) // typesize
    out = bytearray(len(b))
    for k in range(typesize):
        out[k * ne: (k + 1) * ne] = b[k: ne * typesize: typesize]
    out[ne * typesize:] = b[ne * typesize:]
    return bytes(out)


def compress_frame(src: bytes, typesize: int, shuffle: int = 1, blocksize: int = 0):
    """``(frame, kinds)``: the frame ``marex_blosc_compress_h(src, ..., dstcap = len(src) + 16)`` writes, built from the
    uncapped peaks and the room scan; ``kinds`` lists per stream ``"lz4"`` / ``"stored"``, or is ``["frame"]`` for a
    stored frame."""
    nbytes = len(src)
    typesize, blocksize, do_shuffle, blocks = geometry(nbytes, typesize, shuffle, blocksize)
    flags = (1 << 5) | (1 if do_shuffle else 0)

    def header(fl, cbytes):
        return struct.pack("<BBBBIII", 2, 1, fl, typesize, nbytes, blocksize, cbytes)

    def stored_frame():
        return header(flags | 0x2, nbytes + 16) + src, ["frame"]

    pos = 16 + 4 * len(blocks)
    if nbytes == 0 or pos >= nbytes + 16:
        return stored_frame()
    table, body, kinds = [], bytearray(), []
    for off, bsize, nsplits in blocks:
        blk = src[off: off + bsize]
        if do_shuffle:
            blk = shuffle_block(blk, typesize)
        neblock = bsize // nsplits
        table.append(pos)
        for s in range(nsplits):
            stream = blk[s * neblock: (s + 1) * neblock]
            room = nbytes + 16 - pos - 4
            comp, peak = lz4_encode_uncapped(stream)
            if room > 0 and peak <= min(room, neblock - 1):
                payload = comp
                kinds.append("lz4")
            else:
                if neblock > room:
                    return stored_frame()
                payload = stream
                kinds.append("stored")
            body += struct.pack("<i", len(payload)) + payload
            pos += 4 + len(payload)
    frame = header(flags, pos) + struct.pack(f"<{len(table)}I", *table) + bytes(body)
    assert len(frame) == pos
    return frame, kinds


def stream_peak(src: bytes) -> int:
    return lz4_encode_uncapped(src)[1]
