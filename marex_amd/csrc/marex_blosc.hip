// marex_blosc.hip -- host-side decoder for the chunk format of the reference's Zarr v2 stores (first
// step): Blosc-1 frames with the LZ4 codec and byte shuffle, which is what `run_detect.py` / the reference's own test
// fixtures are written with (.zarray: {"id": "blosc", "cname": "lz4", "shuffle": 1}).  Restated from the published
// formats (Blosc 1.x header / block layout, LZ4 block format); no third-party code.  Host pointers only ("_h").
#include "marex_common.hip.h"

namespace {

// LZ4 block format: sequences of [token][literal length+][literals][offset16][match length+]; the last sequence ends
// after its literals.  Returns the number of bytes written or -1 on malformed input / overflow.
long lz4_block_decode(const unsigned char* src, long srclen, unsigned char* dst, long dstcap) {
    const unsigned char* ip = src;
    const unsigned char* const iend = src + srclen;
    unsigned char* op = dst;
    unsigned char* const oend = dst + dstcap;
    while (ip < iend) {
        const unsigned token = *ip++;
        long lit = token >> 4;
        if (lit == 15) {
            unsigned b;
            do {
                if (ip >= iend) return -1;
                b = *ip++;
                lit += b;
            } while (b == 255);
        }
        if (lit > iend - ip || lit > oend - op) return -1;
        memcpy(op, ip, (size_t)lit);
        ip += lit;
        op += lit;
        if (ip >= iend) break;  // last sequence: literals only
        if (iend - ip < 2) return -1;
        const long offset = (long)ip[0] | ((long)ip[1] << 8);
        ip += 2;
        if (offset == 0 || offset > op - dst) return -1;
        long mlen = (long)(token & 15u) + 4;
        if ((token & 15u) == 15u) {
            unsigned b;
            do {
                if (ip >= iend) return -1;
                b = *ip++;
                mlen += b;
            } while (b == 255);
        }
        if (mlen > oend - op) return -1;
        const unsigned char* m = op - offset;
        for (long i = 0; i < mlen; ++i) op[i] = m[i];  // byte-wise: matches may overlap their own output
        op += mlen;
    }
    return (long)(op - dst);
}

inline unsigned rd32(const unsigned char* p) { return (unsigned)p[0] | ((unsigned)p[1] << 8) | ((unsigned)p[2] << 16) | ((unsigned)p[3] << 24); }
inline void wr32(unsigned char* p, unsigned v) {
    p[0] = (unsigned char)v;
    p[1] = (unsigned char)(v >> 8);
    p[2] = (unsigned char)(v >> 16);
    p[3] = (unsigned char)(v >> 24);
}

// Blosc splits a block into `typesize` streams when this holds (c-blosc 1.x blosc_d, also the rule of the releases
// that predate the "dont_split" flag -- frames written this way decode everywhere)
inline bool blosc_splits(unsigned flags, long typesize, long blocksize, bool leftover) {
    return !(flags & 0x10) && !leftover && typesize <= 16 && blocksize / typesize >= 128;
}

// LZ4 block compressor: greedy, one hash probe per position, matches extended eight bytes at a time.  Honours the
// format's end-of-block rules (the last match starts at least 12 bytes before the end, the last 5 bytes are
// literals).  Returns the compressed size, or -1 when the output would not fit in `cap` bytes.
long lz4_block_encode(const unsigned char* src, long n, unsigned char* dst, long cap) {
    constexpr int HLOG = 13;
    int table[1 << HLOG];
    for (int i = 0; i < (1 << HLOG); ++i) table[i] = -1;
    unsigned char* op = dst;
    unsigned char* const oend = dst + cap;
    long anchor = 0, ip = 0;
    auto emit = [&](long lit, long mlen, long offset) -> bool {  // mlen == 0: final literals
        const long need = 1 + lit / 255 + 1 + lit + (mlen ? 2 + mlen / 255 + 1 : 0);
        if (need > oend - op) return false;
        unsigned char* token = op++;
        *token = (unsigned char)((lit < 15 ? lit : 15) << 4);
        if (lit >= 15) {
            long r = lit - 15;
            for (; r >= 255; r -= 255) *op++ = 255;
            *op++ = (unsigned char)r;
        }
        memcpy(op, src + anchor, (size_t)lit);
        op += lit;
        if (mlen) {
            *op++ = (unsigned char)offset;
            *op++ = (unsigned char)(offset >> 8);
            const long m = mlen - 4;
            *token |= (unsigned char)(m < 15 ? m : 15);
            if (m >= 15) {
                long r = m - 15;
                for (; r >= 255; r -= 255) *op++ = 255;
                *op++ = (unsigned char)r;
            }
        }
        return true;
    };
    if (n >= 13) {
        const long mflimit = n - 12, matchlimit = n - 5;
        long misses = 0;
        while (ip <= mflimit) {
            const unsigned v = rd32(src + ip);
            const unsigned h = (v * 2654435761u) >> (32 - HLOG);
            const long cand = table[h];
            table[h] = (int)ip;
            if (cand < 0 || ip - cand > 65535 || rd32(src + cand) != v) {
                ip += 1 + (misses++ >> 6);  // incompressible stretches: widen the step
                continue;
            }
            misses = 0;
            long s = ip, c = cand;
            while (s > anchor && c > 0 && src[s - 1] == src[c - 1]) {  // extend backwards over pending literals
                --s;
                --c;
            }
            long e = ip + 4, ce = cand + 4;
            while (e + 8 <= matchlimit) {
                unsigned long long a, b;
                memcpy(&a, src + e, 8);
                memcpy(&b, src + ce, 8);
                if (a != b) {
                    const long same = __builtin_ctzll(a ^ b) >> 3;
                    e += same;
                    ce += same;
                    goto extended;
                }
                e += 8;
                ce += 8;
            }
            while (e < matchlimit && src[e] == src[ce]) {
                ++e;
                ++ce;
            }
        extended:
            if (!emit(s - anchor, e - s, s - c)) return -1;
            anchor = ip = e;
            if (ip - 2 > cand && ip - 2 <= mflimit) table[(rd32(src + ip - 2) * 2654435761u) >> (32 - HLOG)] = (int)(ip - 2);
        }
    }
    if (!emit(n - anchor, 0, 0)) return -1;
    return (long)(op - dst);
}

}  // namespace

// Compress `nbytes` bytes into one Blosc-1 frame (LZ4 codec, byte shuffle when shuffle != 0 and typesize > 1) -- what the
// reference's `Dataset.to_zarr` writes through numcodecs' default Blosc compressor.  blocksize <= 0 picks 256 KiB.  Data
// that LZ4 cannot shrink is stored (per stream, or the whole frame as a "memcpyed" frame), so dstcap >= nbytes + 16 always
// suffices.  0 = OK and *out_len = frame bytes; -1 bad argument, -4 destination too small.
extern "C" int marex_blosc_compress_h(const void* src_v, int64_t nbytes, int typesize, int shuffle, int64_t blocksize,
                                      void* dst_v, int64_t dstcap, int64_t* out_len) {
    if (!src_v || !dst_v || !out_len || nbytes < 0 || nbytes > 0x7fffffff - 16 || typesize < 1) return -1;
    if (dstcap < nbytes + 16) return -4;
    if (typesize > 255) typesize = 1;  // as Blosc: such items are treated as bytes
    const unsigned char* src = static_cast<const unsigned char*>(src_v);
    unsigned char* dst = static_cast<unsigned char*>(dst_v);
    if (blocksize <= 0) blocksize = 256 * 1024;
    if (blocksize > nbytes && nbytes > 0) blocksize = nbytes;
    if (blocksize > typesize) blocksize -= blocksize % typesize;  // whole elements per block; a ragged tail becomes the leftover block
    const bool do_shuffle = shuffle && typesize > 1;
    unsigned flags = (1u << 5) | (do_shuffle ? 0x1u : 0u);
    dst[0] = 2;  // Blosc format version
    dst[1] = 1;  // LZ4 format version
    dst[3] = (unsigned char)typesize;
    wr32(dst + 4, (unsigned)nbytes);
    wr32(dst + 8, (unsigned)blocksize);
    auto stored_frame = [&]() {
        dst[2] = (unsigned char)(flags | 0x2u);
        memcpy(dst + 16, src, (size_t)nbytes);
        wr32(dst + 12, (unsigned)(nbytes + 16));
        *out_len = nbytes + 16;
        return 0;
    };
    if (nbytes == 0) return stored_frame();
    const long nblocks = (long)((nbytes + blocksize - 1) / blocksize);
    long pos = 16 + 4 * nblocks;
    if (pos >= dstcap) return stored_frame();
    std::vector<unsigned char> tmp(do_shuffle ? (size_t)blocksize : 0);
    for (long j = 0; j < nblocks; ++j) {
        const long bsize = (j == nblocks - 1 && nbytes % blocksize) ? (long)(nbytes % blocksize) : (long)blocksize;
        const bool leftover = bsize != blocksize;
        const unsigned char* in = src + j * blocksize;
        if (do_shuffle) {  // plane k holds byte k of every element; a tail shorter than one element is copied
            const long ne = bsize / typesize;
            for (long k = 0; k < typesize; ++k) {
                unsigned char* plane = tmp.data() + k * ne;
                for (long i = 0; i < ne; ++i) plane[i] = in[i * typesize + k];
            }
            const long rest = bsize - ne * typesize;
            if (rest) memcpy(tmp.data() + ne * typesize, in + ne * typesize, (size_t)rest);
            in = tmp.data();
        }
        const long nsplits = blosc_splits(flags, typesize, (long)blocksize, leftover) && bsize % typesize == 0 ? typesize : 1;
        const long neblock = bsize / nsplits;
        wr32(dst + 16 + 4 * j, (unsigned)pos);
        for (long s = 0; s < nsplits; ++s) {
            // the frame may not grow past nbytes + 16: a stream that does not fit is the signal to store everything
            const long room = (long)(nbytes + 16) - pos - 4;
            long cb = room > 0 ? lz4_block_encode(in + s * neblock, neblock, dst + pos + 4, room < neblock - 1 ? room : neblock - 1) : -1;
            if (cb < 0) {  // not compressible: stored stream, marked by cbytes == raw size
                if (neblock > room) return stored_frame();
                memcpy(dst + pos + 4, in + s * neblock, (size_t)neblock);
                cb = neblock;
            }
            wr32(dst + pos, (unsigned)cb);
            pos += 4 + cb;
        }
    }
    dst[2] = (unsigned char)flags;
    wr32(dst + 12, (unsigned)pos);
    *out_len = pos;
    return 0;
}

// Decompress one Blosc-1 frame.  Returns 0 and the decoded size in *out_len, or a negative code:
//  -1 bad argument, -5 malformed frame, -6 unsupported codec / filter (anything but LZ4 or memcpy, byte shuffle or none)
extern "C" int marex_blosc_decompress_h(const void* src_v, int64_t srclen, void* dst_v, int64_t dstcap, int64_t* out_len) {
    if (!src_v || !dst_v || !out_len || srclen < 16) return -1;
    const unsigned char* src = static_cast<const unsigned char*>(src_v);
    unsigned char* dst = static_cast<unsigned char*>(dst_v);
    const unsigned flags = src[2];
    const long typesize = src[3];
    const long nbytes = rd32(src + 4), blocksize = rd32(src + 8), cbytes = rd32(src + 12);
    if (cbytes > srclen || nbytes > dstcap || typesize < 1) return -5;
    *out_len = nbytes;
    if (nbytes == 0) return 0;
    if (flags & 0x2) {  // memcpyed frame
        if (16 + nbytes > srclen) return -5;
        memcpy(dst, src + 16, (size_t)nbytes);
        return 0;
    }
    if (flags & 0x4) return -6;             // bit shuffle
    const unsigned codec = flags >> 5;      // 0 blosclz, 1 lz4 / lz4hc, 2 snappy, 3 zlib, 4 zstd
    if (codec != 1) return -6;
    if (blocksize <= 0) return -5;
    const bool shuffle = (flags & 0x1) && typesize > 1;
    const long nblocks = (nbytes + blocksize - 1) / blocksize;
    if (16 + 4 * nblocks > srclen) return -5;
    std::vector<unsigned char> tmp((size_t)blocksize);
    for (long j = 0; j < nblocks; ++j) {
        const long bsize = (j == nblocks - 1 && nbytes % blocksize) ? nbytes % blocksize : blocksize;
        const bool leftover = bsize != blocksize;
        const long nsplits = (blosc_splits(flags, typesize, blocksize, leftover) && bsize % typesize == 0) ? typesize : 1;
        const long neblock = bsize / nsplits;
        long pos = rd32(src + 16 + 4 * j);
        unsigned char* out = shuffle ? tmp.data() : dst + j * blocksize;
        for (long s = 0; s < nsplits; ++s) {
            if (pos + 4 > srclen) return -5;
            const long cb = rd32(src + pos);
            pos += 4;
            if (cb < 0 || pos + cb > srclen) return -5;
            if (cb == neblock) {
                memcpy(out + s * neblock, src + pos, (size_t)neblock);
            } else if (lz4_block_decode(src + pos, cb, out + s * neblock, neblock) != neblock) {
                return -5;
            }
            pos += cb;
        }
        if (shuffle) {  // undo the byte shuffle: plane k of the block holds byte k of every element
            unsigned char* d = dst + j * blocksize;
            const long ne = bsize / typesize;
            for (long k = 0; k < typesize; ++k) {
                const unsigned char* plane = tmp.data() + k * ne;
                for (long i = 0; i < ne; ++i) d[i * typesize + k] = plane[i];
            }
            const long rest = bsize - ne * typesize;
            if (rest) memcpy(d + ne * typesize, tmp.data() + ne * typesize, (size_t)rest);
        }
    }
    return 0;
}

// ------------------------------------------------------------------------------------------------
// Device side: decode many LZ4 streams at once (one wave per stream) and undo the byte shuffle while placing the
// elements in the destination array -- compressed chunks go over PCIe, the float field is born in HBM.
//
// A wave walks its stream's sequences in lock step (token / lengths / offset are wave-uniform); literal and match
// copies are spread over the 64 lanes.  Matches are served from an LDS ring that mirrors the last RING bytes of the
// output (RING >= 64 KiB whenever the stream is longer than that: LZ4 offsets reach 65 535 bytes back), so nothing is
// ever re-read from global memory and the wave never waits for its own global stores; every step reads all its sources
// before it writes (the LDS queue of a wave is in order), and long overlapping matches
// (runs) are cut into pieces so that their source bytes are still in the ring.
// ------------------------------------------------------------------------------------------------
// stored (incompressible) splits: plain copies, spread over many threads
__global__ void __launch_bounds__(256)
k_stored_streams(const unsigned char* __restrict__ comp, const long* __restrict__ src_off, const int* __restrict__ csize,
                 const long* __restrict__ dst_off, const int* __restrict__ rawsz, int n_streams, unsigned char* __restrict__ out) {
    const int i = (int)blockIdx.x * 256 + threadIdx.x;
    for (int s = blockIdx.y; s < n_streams; s += gridDim.y) {  // a grid's y extent ends at 65 535: more streams are strided over
        const int raw = rawsz[s];
        if (csize[s] == raw && i < raw) out[dst_off[s] + i] = comp[src_off[s] + i];
    }
}

__global__ void __launch_bounds__(64)
k_lz4_streams(const unsigned char* __restrict__ comp, const long* __restrict__ src_off, const int* __restrict__ csize,
              const long* __restrict__ dst_off, const int* __restrict__ rawsz, int ring_mask,
              unsigned char* __restrict__ out, int* __restrict__ status) {
    extern __shared__ unsigned char ring[];
    const int s = blockIdx.x, lane = threadIdx.x;
    const unsigned char* src = comp + src_off[s];
    unsigned char* dst = out + dst_off[s];
    const int cs = csize[s], raw = rawsz[s];
    if (cs == raw) return;  // stored split: k_stored_streams
    auto byte_at = [&](int p) -> unsigned { return src[p]; };  // wave-uniform address: one broadcast load (L1 resident)
    int ip = 0, op = 0;
    bool bad = false;
    while (ip < cs) {
        const unsigned token = byte_at(ip++);
        int lit = (int)(token >> 4);
        if (lit == 15) {
            unsigned b = 255;
            while (b == 255 && ip < cs) {
                b = byte_at(ip++);
                lit += (int)b;
            }
        }
        if (lit > cs - ip || lit > raw - op) {
            bad = true;
            break;
        }
        for (int i = lane; i < lit; i += 64) {
            const unsigned char c = (unsigned char)byte_at(ip + i);
            ring[(op + i) & ring_mask] = c;
            dst[op + i] = c;
        }
        ip += lit;
        op += lit;
        if (ip >= cs) break;  // last sequence: literals only
        if (cs - ip < 2) {
            bad = true;
            break;
        }
        const unsigned o_lo = byte_at(ip), o_hi = byte_at(ip + 1);
        const int offset = (int)(o_lo | (o_hi << 8));
        ip += 2;
        int mlen = (int)(token & 15u) + 4;
        if ((token & 15u) == 15u) {
            unsigned b = 255;
            while (b == 255 && ip < cs) {
                b = byte_at(ip++);
                mlen += (int)b;
            }
        }
        if (offset == 0 || offset > op || mlen > raw - op) {
            bad = true;
            break;
        }
        __builtin_amdgcn_s_waitcnt(0xC07F);  /* lgkmcnt(0): LDS only, never the global stores */  // the literals are in the ring before anybody reads them back
        if (offset >= 64) {
            for (int base = 0; base < mlen; base += 64) {
                const int i = base + lane;
                unsigned char v = 0;
                if (i < mlen) v = ring[(op - offset + i) & ring_mask];
                __builtin_amdgcn_s_waitcnt(0xC07F);  /* lgkmcnt(0): LDS only, never the global stores */
                if (i < mlen) {
                    ring[(op + i) & ring_mask] = v;
                    dst[op + i] = v;
                }
                __builtin_amdgcn_s_waitcnt(0xC07F);  /* lgkmcnt(0): LDS only, never the global stores */
            }
        } else {  // the last `offset` bytes repeat: pieces short enough that their source stays in the ring
            int done = 0;
            while (done < mlen) {
                const int piece = mlen - done < 8192 ? mlen - done : 8192;
                const int o = op + done;
                for (int i = lane; i < piece; i += 64) {
                    const unsigned char v = ring[(o - offset + (i % offset)) & ring_mask];
                    ring[(o + i) & ring_mask] = v;
                    dst[o + i] = v;
                }
                __builtin_amdgcn_s_waitcnt(0xC07F);  /* lgkmcnt(0): LDS only, never the global stores */
                done += piece;
            }
        }
        op += mlen;
    }
    if (lane == 0 && (bad || op != raw)) atomicAdd(status, 1);
}

// byte planes of a shuffled block -> elements at their place in the destination (typesize bytes each)
__global__ void __launch_bounds__(256)
k_unshuffle_place(const unsigned char* __restrict__ planes, const long* __restrict__ blk_off, const long* __restrict__ blk_elem0,
                  const int* __restrict__ blk_ne, const int* __restrict__ blk_valid, int n_blocks, int typesize, int shuffled,
                  unsigned char* __restrict__ out) {
    const int e = (int)blockIdx.x * 256 + threadIdx.x;
    for (int b = blockIdx.y; b < n_blocks; b += gridDim.y) {  // as k_stored_streams: more than 65 535 blocks are strided over
        if (e >= blk_valid[b]) continue;
        const int ne = blk_ne[b];
        const unsigned char* p = planes + blk_off[b];
        unsigned char* o = out + (size_t)(blk_elem0[b] + e) * typesize;
        if (shuffled) {
            for (int k = 0; k < typesize; ++k) o[k] = p[(size_t)k * ne + e];
        } else {
            for (int k = 0; k < typesize; ++k) o[k] = p[(size_t)e * typesize + k];
        }
    }
}

extern "C" int marex_lz4_decode_streams(marex_ctx* ctx, const uint8_t* comp, const int64_t* src_off, const int32_t* csize,
                                        const int64_t* dst_off, const int32_t* rawsz, int n_streams, int max_raw,
                                        uint8_t* planes, int32_t* status) {
    if (!ctx) return -1;
    if (!comp || !src_off || !csize || !dst_off || !rawsz || !planes || !status || n_streams <= 0 || max_raw <= 0)
        return fail(ctx, -1, "marex_lz4_decode_streams: null pointer or empty table");
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    int ring = 1024;
    while (ring < max_raw && ring < 65536) ring <<= 1;  // power of two: ring positions are masked
    if (ring > 48 * 1024)
        HIP_TRY(ctx, hipFuncSetAttribute((const void*)k_lz4_streams, hipFuncAttributeMaxDynamicSharedMemorySize, ring));
    hipLaunchKernelGGL(k_stored_streams, dim3((unsigned)((max_raw + 255) / 256), (unsigned)std::min(n_streams, 65535)), dim3(256), 0,
                       ctx->stream, comp, reinterpret_cast<const long*>(src_off), csize, reinterpret_cast<const long*>(dst_off), rawsz,
                       n_streams, planes);
    hipLaunchKernelGGL(k_lz4_streams, dim3((unsigned)n_streams), dim3(64), (size_t)ring, ctx->stream, comp,
                       reinterpret_cast<const long*>(src_off), csize, reinterpret_cast<const long*>(dst_off), rawsz, ring - 1, planes,
                       status);
    HIP_TRY(ctx, hipGetLastError());
    return 0;
}

extern "C" int marex_unshuffle_place(marex_ctx* ctx, const uint8_t* planes, const int64_t* blk_off, const int64_t* blk_elem0,
                                     const int32_t* blk_ne, const int32_t* blk_valid, int n_blocks, int max_ne, int typesize,
                                     int shuffled, uint8_t* out) {
    if (!ctx) return -1;
    if (!planes || !blk_off || !blk_elem0 || !blk_ne || !blk_valid || !out || n_blocks <= 0 || max_ne <= 0 || typesize < 1)
        return fail(ctx, -1, "marex_unshuffle_place: null pointer or empty table");
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    hipLaunchKernelGGL(k_unshuffle_place, dim3((unsigned)((max_ne + 255) / 256), (unsigned)std::min(n_blocks, 65535)), dim3(256), 0,
                       ctx->stream, planes, reinterpret_cast<const long*>(blk_off), reinterpret_cast<const long*>(blk_elem0), blk_ne,
                       blk_valid, n_blocks, typesize, shuffled, out);
    HIP_TRY(ctx, hipGetLastError());
    return 0;
}

// ------------------------------------------------------------------------------------------------
// Device side: compress many equal-sized chunks into Blosc-1 / LZ4 frames that are byte-identical to what
// marex_blosc_compress_h(chunk, nbytes, typesize, shuffle, blocksize, dst, nbytes + 16, ...) writes.  Four passes:
//   1. k_blosc_shuffle     byte planes of every block (plane k = byte k of every element; a ragged tail is copied)
//   2. k_lz4_encode_wave / k_lz4_encode_lane
//                          every stream encoded WITHOUT the frame's cap into a scratch slot of its own size, recording the
//                          peak demand max(bytes written + need) over its emits -- lz4_block_encode(cap) fails exactly when
//                          that peak exceeds cap (the encoder's output does not depend on cap otherwise)
//   3. k_blosc_plan        one thread per frame: the room rule of marex_blosc_compress_h over the recorded peaks decides
//                          per stream compressed / stored, or a stored frame; writes header, block table and positions
//   4. k_blosc_gather      streams (or the raw chunk of a stored frame) copied to their place in the frame
// ------------------------------------------------------------------------------------------------
namespace {

constexpr int LZ4_HLOG = 13;

// chunk geometry shared by the host entry points and the kernels (restates the frame rules of marex_blosc_compress_h)
struct BloscGeom {
    long nbytes;        // bytes per chunk
    long blocksize;     // after the host's clamps (written to the header)
    int typesize;       // after "> 255 -> 1"
    int shuffle;        // byte shuffle applied (shuffle != 0 && typesize > 1)
    long nblocks;       // blocks per chunk (0 when nbytes == 0)
    long nfull;         // blocks of exactly blocksize bytes
    long lastsize;      // bytes of the last block (== blocksize unless it is a leftover block)
    int nsplits;        // streams per full block
    long spc;           // streams per chunk
    bool early_stored;  // nbytes == 0 or the block table alone reaches nbytes + 16: stored frame without encoding
};

BloscGeom blosc_geom(long nbytes, int typesize, int shuffle, long blocksize) {
    BloscGeom g{};
    if (typesize > 255) typesize = 1;
    if (blocksize <= 0) blocksize = 256 * 1024;
    if (blocksize > nbytes && nbytes > 0) blocksize = nbytes;
    if (blocksize > typesize) blocksize -= blocksize % typesize;
    g.nbytes = nbytes;
    g.blocksize = blocksize;
    g.typesize = typesize;
    g.shuffle = (shuffle && typesize > 1) ? 1 : 0;
    const unsigned flags = (1u << 5) | (g.shuffle ? 0x1u : 0u);
    g.nblocks = nbytes > 0 ? (nbytes + blocksize - 1) / blocksize : 0;
    g.nfull = nbytes / blocksize;
    g.lastsize = nbytes % blocksize ? nbytes % blocksize : blocksize;
    g.nsplits = (blosc_splits(flags, typesize, blocksize, false) && blocksize % typesize == 0) ? typesize : 1;
    g.spc = g.nfull * g.nsplits + (g.nblocks > g.nfull ? 1 : 0);
    g.early_stored = nbytes == 0 || 16 + 4 * g.nblocks >= nbytes + 16;
    return g;
}

// stream q of a chunk -> (byte offset in the chunk, bytes); leftover blocks are never split
__device__ __forceinline__ void stream_span(const BloscGeom& g, long q, long& off, long& n) {
    const long nfs = g.nfull * g.nsplits;
    if (q < nfs) {
        n = g.blocksize / g.nsplits;
        off = q * n;
    } else {
        n = g.nbytes - g.nfull * g.blocksize;
        off = g.nfull * g.blocksize;
    }
}

__device__ __forceinline__ unsigned rd32_d(const unsigned char* p) {
    return (unsigned)p[0] | ((unsigned)p[1] << 8) | ((unsigned)p[2] << 16) | ((unsigned)p[3] << 24);
}
__device__ __forceinline__ unsigned lz4_hash(unsigned v) { return (v * 2654435761u) >> (32 - LZ4_HLOG); }

// sum_{i < x} (i >> 6): the encoder's miss steps are 1 + (misses++ >> 6)
__device__ __forceinline__ long miss_sum(long x) {
    const long a = x >> 6, b = x & 63;
    return 32 * a * (a - 1) + a * b;
}

}  // namespace

__global__ void __launch_bounds__(256)
k_blosc_shuffle(const unsigned char* __restrict__ src, BloscGeom g, unsigned char* __restrict__ planes) {
    const long blk = blockIdx.x;  // chunk * nblocks + block
    const long c = blk / g.nblocks, j = blk - c * g.nblocks;
    const long bsize = (j == g.nblocks - 1) ? g.lastsize : g.blocksize;
    const long ne = bsize / g.typesize, rest = bsize - ne * g.typesize;
    const unsigned char* in = src + c * g.nbytes + j * g.blocksize;
    unsigned char* out = planes + c * g.nbytes + j * g.blocksize;
    for (long i = (long)blockIdx.y * 256 + threadIdx.x; i < ne || i < rest; i += (long)gridDim.y * 256) {
        if (i < ne)
            for (int k = 0; k < g.typesize; ++k) out[k * ne + i] = in[i * g.typesize + k];
        if (i < rest) out[ne * g.typesize + i] = in[ne * g.typesize + i];
    }
}

// One lane per stream (the device reference): lane 0 of the wave runs lz4_block_encode verbatim with cap = n - 1,
// the table in LDS.  peak[s] = the peak demand (> n - 1 once the stream cannot be compressed at all); csize[s] = bytes.
__global__ void __launch_bounds__(64)
k_lz4_encode_lane(const unsigned char* __restrict__ base, BloscGeom g, unsigned char* __restrict__ scratch,
                  int* __restrict__ peak, int* __restrict__ csize) {
    __shared__ int table[1 << LZ4_HLOG];
    const long sidx = blockIdx.x;
    const long c = sidx / g.spc, q = sidx - c * g.spc;
    long off, n;
    stream_span(g, q, off, n);
    for (int i = threadIdx.x; i < (1 << LZ4_HLOG); i += 64) table[i] = -1;
    __syncthreads();
    if (threadIdx.x != 0) return;
    const unsigned char* src = base + c * g.nbytes + off;
    unsigned char* dst = scratch + c * g.nbytes + off;
    const long cap = n - 1;
    long op = 0, pk = 0, anchor = 0, ip = 0;
    auto emit = [&](long lit, long mlen, long offset) -> bool {
        const long need = 1 + lit / 255 + 1 + lit + (mlen ? 2 + mlen / 255 + 1 : 0);
        if (op + need > pk) pk = op + need;
        if (op + need > cap) return false;
        long t = op++;
        unsigned char token = (unsigned char)((lit < 15 ? lit : 15) << 4);
        if (lit >= 15) {
            long r = lit - 15;
            for (; r >= 255; r -= 255) dst[op++] = 255;
            dst[op++] = (unsigned char)r;
        }
        for (long i = 0; i < lit; ++i) dst[op + i] = src[anchor + i];
        op += lit;
        if (mlen) {
            dst[op++] = (unsigned char)offset;
            dst[op++] = (unsigned char)(offset >> 8);
            const long m = mlen - 4;
            token |= (unsigned char)(m < 15 ? m : 15);
            if (m >= 15) {
                long r = m - 15;
                for (; r >= 255; r -= 255) dst[op++] = 255;
                dst[op++] = (unsigned char)r;
            }
        }
        dst[t] = token;
        return true;
    };
    bool ok = true;
    if (n >= 13) {
        const long mflimit = n - 12, matchlimit = n - 5;
        long misses = 0;
        while (ip <= mflimit) {
            const unsigned v = rd32_d(src + ip);
            const unsigned h = lz4_hash(v);
            const long cand = table[h];
            table[h] = (int)ip;
            if (cand < 0 || ip - cand > 65535 || rd32_d(src + cand) != v) {
                ip += 1 + (misses++ >> 6);
                continue;
            }
            misses = 0;
            long s = ip, cc = cand;
            while (s > anchor && cc > 0 && src[s - 1] == src[cc - 1]) {
                --s;
                --cc;
            }
            long e = ip + 4, ce = cand + 4;
            while (e < matchlimit && src[e] == src[ce]) {
                ++e;
                ++ce;
            }
            if (!emit(s - anchor, e - s, s - cc)) {
                ok = false;
                break;
            }
            anchor = ip = e;
            if (ip - 2 > cand && ip - 2 <= mflimit) table[lz4_hash(rd32_d(src + ip - 2))] = (int)(ip - 2);
        }
    }
    if (ok) ok = emit(n - anchor, 0, 0);
    peak[sidx] = (int)(ok ? pk : n);
    csize[sidx] = (int)(ok ? op : -1);
}

// One wave per stream.  The greedy loop is run speculatively: with no match, the next 64 positions it visits follow from
// ip and misses alone, so lane k hashes position p_k = ip + k + miss_sum(misses + k) - miss_sum(misses); its candidate
// is the latest earlier lane with the same hash, else the LDS table.  The first lane whose candidate verifies is the
// match; the table writes of the lanes up to and including it are committed (for a hash shared by several of them, the
// last one's).  Extensions compare 64 positions (forward: 64 x 8 bytes) per step; literals are copied by all lanes.
__global__ void __launch_bounds__(64)
k_lz4_encode_wave(const unsigned char* __restrict__ base, BloscGeom g, unsigned char* __restrict__ scratch,
                  int* __restrict__ peak, int* __restrict__ csize) {
    __shared__ int table[1 << LZ4_HLOG];
    const long sidx = blockIdx.x;
    const long c = sidx / g.spc, q = sidx - c * g.spc;
    const int lane = threadIdx.x;
    long off, n;
    stream_span(g, q, off, n);
    for (int i = lane; i < (1 << LZ4_HLOG); i += 64) table[i] = -1;
    __syncthreads();
    const unsigned char* src = base + c * g.nbytes + off;
    unsigned char* dst = scratch + c * g.nbytes + off;
    const long cap = n - 1;
    long op = 0, pk = 0, anchor = 0, ip = 0;
    // all lanes hold the same op / pk / anchor; bytes are written by the lanes in turn
    auto put_len = [&](long o, long nff, long r) {  // nff bytes of 255, then r, at dst[o ..]
        for (long i = lane; i <= nff; i += 64) dst[o + i] = (unsigned char)(i < nff ? 255 : r);
    };
    auto emit = [&](long lit, long mlen, long offset) -> bool {
        const long need = 1 + lit / 255 + 1 + lit + (mlen ? 2 + mlen / 255 + 1 : 0);
        if (op + need > pk) pk = op + need;
        if (op + need > cap) return false;
        const long m = mlen ? mlen - 4 : 0;
        const unsigned char token = (unsigned char)(((lit < 15 ? lit : 15) << 4) | (mlen ? (m < 15 ? m : 15) : 0));
        if (lane == 0) dst[op] = token;
        op += 1;
        if (lit >= 15) {
            const long nff = (lit - 15) / 255;
            put_len(op, nff, (lit - 15) % 255);
            op += nff + 1;
        }
        for (long i = lane; i < lit; i += 64) dst[op + i] = src[anchor + i];
        op += lit;
        if (mlen) {
            if (lane == 0) {
                dst[op] = (unsigned char)offset;
                dst[op + 1] = (unsigned char)(offset >> 8);
            }
            op += 2;
            if (m >= 15) {
                const long nff = (m - 15) / 255;
                put_len(op, nff, (m - 15) % 255);
                op += nff + 1;
            }
        }
        return true;
    };
    bool ok = true;
    if (n >= 13) {
        const long mflimit = n - 12, matchlimit = n - 5;
        long misses = 0;
        while (ip <= mflimit) {
            const long p = ip + lane + miss_sum(misses + lane) - miss_sum(misses);
            const bool valid = p <= mflimit;
            const unsigned v = valid ? rd32_d(src + p) : 0u;
            const int h = valid ? (int)lz4_hash(v) : -1 - lane;  // invalid lanes never share a hash
            int prev = -1, next = 64;
#pragma unroll
            for (int j = 0; j < 64; ++j) {
                const int hj = __builtin_amdgcn_readlane(h, j);
                if (hj == h) {
                    if (j < lane) prev = j;
                    else if (j > lane && next == 64) next = j;
                }
            }
            const long pprev = __shfl((int)p, prev < 0 ? lane : prev);
            long cand = -1;
            if (valid) cand = prev >= 0 ? pprev : (long)table[h];
            const bool hit = valid && cand >= 0 && p - cand <= 65535 && rd32_d(src + cand) == v;
            const unsigned long long hits = __ballot(hit);
            if (!hits) {
                const unsigned long long vm = __ballot(valid);
                const int nvalid = __popcll(vm);
                if (valid && next == 64) table[h] = (int)p;
                ip = ip + nvalid + miss_sum(misses + nvalid) - miss_sum(misses);
                misses += nvalid;
                __syncthreads();
                continue;
            }
            const int ks = __builtin_ctzll(hits);
            if (lane <= ks && next > ks) table[h] = (int)p;
            ip = __shfl((int)p, ks);
            const long mcand = __shfl((int)cand, ks);
            misses = 0;
            // backward over the pending literals: s - 1 - k >= anchor, c - 1 - k >= 0, bytes equal
            long s = ip, cc = mcand;
            for (;;) {
                const long t = s - 1 - lane, u = cc - 1 - lane;
                const bool same = t >= anchor && u >= 0 && src[t] == src[u];
                const unsigned long long miss = __ballot(!same);
                if (!miss) {
                    s -= 64;
                    cc -= 64;
                    continue;
                }
                const int f = __builtin_ctzll(miss);
                s -= f;
                cc -= f;
                break;
            }
            // forward from ip + 4: the first position >= matchlimit or with a differing byte, 8 positions per lane
            const long d = ip - mcand;
            long e = ip + 4;
            for (;;) {
                const long x0 = e + 8 * (long)lane;
                unsigned diff = 0;  // bit b: position x0 + b stops the match (all 16 loads issued before any test)
#pragma unroll
                for (int b = 0; b < 8; ++b) {
                    const long x = x0 + b;
                    const bool in = x < matchlimit;
                    const unsigned char u = in ? src[x] : 0, w = in ? src[x - d] : 1;
                    diff |= (unsigned)(u != w) << b;
                }
                const int stop = diff ? __builtin_ctz(diff) : 8;
                const unsigned long long st = __ballot(stop < 8);
                if (!st) {
                    e += 512;
                    continue;
                }
                const int f = __builtin_ctzll(st);
                e = e + 8 * (long)f + __shfl(stop, f);
                break;
            }
            if (!emit(s - anchor, e - s, s - cc)) {
                ok = false;
                break;
            }
            anchor = ip = e;
            if (lane == 0 && ip - 2 > mcand && ip - 2 <= mflimit) table[lz4_hash(rd32_d(src + ip - 2))] = (int)(ip - 2);
            __syncthreads();
        }
    }
    if (ok) ok = emit(n - anchor, 0, 0);
    if (lane == 0) {
        peak[sidx] = (int)(ok ? pk : n);
        csize[sidx] = (int)(ok ? op : -1);
    }
}

namespace {
__device__ __forceinline__ void wr32_d(unsigned char* p, unsigned v) {
    p[0] = (unsigned char)v;
    p[1] = (unsigned char)(v >> 8);
    p[2] = (unsigned char)(v >> 16);
    p[3] = (unsigned char)(v >> 24);
}
}  // namespace

// one thread per frame: the room rule of marex_blosc_compress_h.  cb[s] = compressed size or n (stored stream),
// pos[s] = where its 4-byte size goes; stored[c] = 1 for a stored frame; len[c] = frame bytes.
__global__ void __launch_bounds__(64)
k_blosc_plan(BloscGeom g, long n_chunks, const int* __restrict__ peak, const int* __restrict__ csize, int* __restrict__ cb,
             int* __restrict__ pos_out, int* __restrict__ stored, unsigned char* __restrict__ dst, long long* __restrict__ len) {
    const long c = (long)blockIdx.x * 64 + threadIdx.x;
    if (c >= n_chunks) return;
    unsigned char* f = dst + c * (g.nbytes + 16);
    const unsigned flags = (1u << 5) | (g.shuffle ? 0x1u : 0u);
    f[0] = 2;
    f[1] = 1;
    f[3] = (unsigned char)g.typesize;
    wr32_d(f + 4, (unsigned)g.nbytes);
    wr32_d(f + 8, (unsigned)g.blocksize);
    bool st = g.early_stored;
    long pos = 16 + 4 * g.nblocks;
    for (long q = 0; q < g.spc && !st; ++q) {
        const long s = c * g.spc + q;
        const long nfs = g.nfull * g.nsplits;
        const long neblock = q < nfs ? g.blocksize / g.nsplits : g.nbytes - g.nfull * g.blocksize;
        if (q < nfs ? q % g.nsplits == 0 : true) wr32_d(f + 16 + 4 * (q < nfs ? q / g.nsplits : g.nfull), (unsigned)pos);
        const long room = g.nbytes + 16 - pos - 4;
        const long capq = room < neblock - 1 ? room : neblock - 1;
        long b;
        if (room > 0 && peak[s] <= capq) {
            b = csize[s];
        } else {
            if (neblock > room) {
                st = true;
                break;
            }
            b = neblock;
        }
        cb[s] = (int)b;
        pos_out[s] = (int)pos;
        pos += 4 + b;
    }
    stored[c] = st ? 1 : 0;
    f[2] = (unsigned char)(st ? (flags | 0x2u) : flags);
    const long total = st ? g.nbytes + 16 : pos;
    wr32_d(f + 12, (unsigned)total);
    len[c] = total;
}

// grid (x: stream, y: pieces of 4096 bytes): [cb][stream bytes] of every stream of a frame that is not stored
__global__ void __launch_bounds__(256)
k_blosc_gather_streams(BloscGeom g, const unsigned char* __restrict__ planes, const unsigned char* __restrict__ scratch,
                       const int* __restrict__ cb, const int* __restrict__ pos_in, const int* __restrict__ stored,
                       unsigned char* __restrict__ dst) {
    const long s = blockIdx.x;
    const long c = s / g.spc, q = s - c * g.spc;
    if (stored[c]) return;
    long off, n;
    stream_span(g, q, off, n);
    const long b = cb[s];
    unsigned char* f = dst + c * (g.nbytes + 16) + pos_in[s];
    const unsigned char* from = (b == n ? planes : scratch) + c * g.nbytes + off;
    if (blockIdx.y == 0 && threadIdx.x == 0) wr32_d(f, (unsigned)b);
    for (long i0 = (long)blockIdx.y * 4096; i0 < b; i0 += (long)gridDim.y * 4096)
        for (long i = i0 + threadIdx.x; i < i0 + 4096 && i < b; i += 256) f[4 + i] = from[i];
}

// grid (x: pieces of 4096 bytes, y: chunks), both strided: the raw chunk into a stored frame
__global__ void __launch_bounds__(256)
k_blosc_gather_stored(BloscGeom g, long n_chunks, const unsigned char* __restrict__ src, const int* __restrict__ stored,
                      unsigned char* __restrict__ dst) {
    for (long c = blockIdx.y; c < n_chunks; c += gridDim.y) {
        if (!stored[c]) continue;
        for (long i0 = (long)blockIdx.x * 4096; i0 < g.nbytes; i0 += (long)gridDim.x * 4096)
            for (long i = i0 + threadIdx.x; i < i0 + 4096 && i < g.nbytes; i += 256)
                dst[c * (g.nbytes + 16) + 16 + i] = src[c * g.nbytes + i];
    }
}

namespace {
// work layout: [planes: n_chunks * nbytes when shuffling][scratch: n_chunks * nbytes][peak, csize, cb, pos: int32 per
// stream][stored: int32 per chunk], every part 256-byte aligned
struct BloscWork {
    long planes, scratch, peak, csize, cb, pos, stored, total;
};
BloscWork blosc_work(const BloscGeom& g, long n_chunks) {
    auto al = [](long v) { return (v + 255) / 256 * 256; };
    const long ns = g.spc * n_chunks;
    BloscWork w{};
    long o = 0;
    w.planes = o;
    o += al(g.shuffle ? n_chunks * g.nbytes : 0);
    w.scratch = o;
    o += al(n_chunks * g.nbytes);
    w.peak = o;
    o += al(4 * ns);
    w.csize = o;
    o += al(4 * ns);
    w.cb = o;
    o += al(4 * ns);
    w.pos = o;
    o += al(4 * ns);
    w.stored = o;
    o += al(4 * n_chunks);
    w.total = o;
    return w;
}
}  // namespace

extern "C" int marex_blosc_compress_work_bytes(int64_t nbytes, int typesize, int shuffle, int64_t blocksize, int64_t n_chunks,
                                               int64_t* out) {
    if (!out || nbytes < 0 || nbytes > 0x7fffffff - 16 || typesize < 1 || n_chunks < 0) return -1;
    const BloscGeom g = blosc_geom((long)nbytes, typesize, shuffle, (long)blocksize);
    *out = blosc_work(g, (long)n_chunks).total;
    return 0;
}

extern "C" int marex_blosc_compress_d(marex_ctx* ctx, const uint8_t* src, int64_t nbytes, int64_t n_chunks, int typesize,
                                      int shuffle, int64_t blocksize, int variant, uint8_t* work, int64_t work_bytes,
                                      uint8_t* dst, int64_t* out_len) {
    if (!ctx) return -1;
    if ((!src && nbytes > 0) || !work || !dst || !out_len || nbytes < 0 || nbytes > 0x7fffffff - 16 || typesize < 1 || n_chunks <= 0 ||
        (variant != 0 && variant != 1))
        return fail(ctx, -1, "marex_blosc_compress_d: bad argument");
    const BloscGeom g = blosc_geom((long)nbytes, typesize, shuffle, (long)blocksize);
    const BloscWork w = blosc_work(g, (long)n_chunks);
    if (work_bytes < w.total) return fail(ctx, -4, "marex_blosc_compress_d: work holds %lld bytes, %ld needed", (long long)work_bytes, w.total);
    const long ns = g.spc * (long)n_chunks;
    if (ns > 0x7fffffffL) return fail(ctx, -1, "marex_blosc_compress_d: %ld streams in one call", ns);
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    unsigned char* planes = g.shuffle ? work + w.planes : const_cast<unsigned char*>(src);
    int* peak = reinterpret_cast<int*>(work + w.peak);
    int* csize = reinterpret_cast<int*>(work + w.csize);
    int* cb = reinterpret_cast<int*>(work + w.cb);
    int* pos = reinterpret_cast<int*>(work + w.pos);
    int* stored = reinterpret_cast<int*>(work + w.stored);
    if (!g.early_stored) {
        if (g.shuffle) {
            const long ne_max = g.blocksize / g.typesize + 1;
            const unsigned gy = (unsigned)std::min<long>((ne_max + 255) / 256, 64);
            hipLaunchKernelGGL(k_blosc_shuffle, dim3((unsigned)(g.nblocks * n_chunks), gy), dim3(256), 0, ctx->stream, src, g, planes);
        }
        if (variant == 0)
            hipLaunchKernelGGL(k_lz4_encode_wave, dim3((unsigned)ns), dim3(64), 0, ctx->stream, planes, g, work + w.scratch, peak, csize);
        else
            hipLaunchKernelGGL(k_lz4_encode_lane, dim3((unsigned)ns), dim3(64), 0, ctx->stream, planes, g, work + w.scratch, peak, csize);
    }
    hipLaunchKernelGGL(k_blosc_plan, dim3((unsigned)((n_chunks + 63) / 64)), dim3(64), 0, ctx->stream, g, (long)n_chunks, peak, csize,
                       cb, pos, stored, dst, reinterpret_cast<long long*>(out_len));
    if (!g.early_stored) {
        const long nmax = g.nsplits > 1 ? std::max(g.blocksize / g.nsplits, g.lastsize) : g.blocksize;
        hipLaunchKernelGGL(k_blosc_gather_streams, dim3((unsigned)ns, (unsigned)std::min<long>((nmax + 4095) / 4096, 1024)), dim3(256), 0, ctx->stream, g,
                           planes, work + w.scratch, cb, pos, stored, dst);
    }
    if (g.nbytes > 0)
        hipLaunchKernelGGL(k_blosc_gather_stored, dim3((unsigned)std::min<long>((g.nbytes + 4095) / 4096, 4096),
                           (unsigned)std::min<long>((long)n_chunks, 1024)), dim3(256), 0, ctx->stream, g, (long)n_chunks, src, stored, dst);
    HIP_TRY(ctx, hipGetLastError());
    return 0;
}
