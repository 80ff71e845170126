// marex_morphology.hip -- tracker pre-processing stage (first half): binary closing + opening of the
// extreme mask with a disk (marEx/track.py:1520-1676, gridded branch) and the temporal closing (track.py:1678-1726).
//
// The image of one timestep is padded by 2R cells on every side (wrap = global grid, edge = regional mode), bit-packed
// 64 cells per word, and the four morphological passes (dilate, erode | erode, dilate) run on the packed rows: one
// thread per output word ORs, for every row offset dy of the disk, the row's word dilated horizontally by the disk's
// half-width at dy (shifts across the word boundaries through the two neighbouring words).  Erosion is the dilation of
// the complement with the outside set to 1 -- scipy's border_value = 0 for both operations, which the reference
// inherits through dask_image, so the contamination that creeps 4R cells in from the padded border is reproduced too.
#include "marex_common.hip.h"

// padded packed layout: [T][Hp = ny + 4R][Wp = ceil((nx + 4R) / 64)] words; bit i of word w = cell x = 64 w + i of the
// padded row; bits past the row end are kept 0.
// one workgroup per padded row: the source row is resolved once (uniform), a wave packs 64 cells per ballot
__global__ void __launch_bounds__(256)
k_morph_pack(const unsigned char* __restrict__ data, long T, int ny, int nx, int R, int regional, int Hp, int Wp,
             u64* __restrict__ packed) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int nxp = nx + 4 * R;
    const long rows = T * Hp;
    for (long r = blockIdx.x; r < rows; r += gridDim.x) {
        const int yy = (int)(r % Hp);
        const long t = r / Hp;
        int y = yy - 2 * R;
        if (regional) {  // np.pad mode="edge"
            y = y < 0 ? 0 : (y >= ny ? ny - 1 : y);
        } else {  // np.pad mode="wrap" (both dimensions, as the reference does)
            y %= ny;
            if (y < 0) y += ny;
        }
        const unsigned char* src = data + ((size_t)t * ny + y) * nx;
        for (int w0 = wave; w0 < Wp; w0 += 4 * 8) {  // 8 byte loads in flight per lane before the ballots
            unsigned char v[8];
#pragma unroll
            for (int u = 0; u < 8; ++u) {
                const int xx = 64 * (w0 + 4 * u) + lane;
                v[u] = 0;
                if (w0 + 4 * u < Wp && xx < nxp) {
                    int x = xx - 2 * R;
                    if (regional) {
                        x = x < 0 ? 0 : (x >= nx ? nx - 1 : x);
                    } else {
                        x %= nx;  // np.pad "wrap" repeats as often as needed (grids narrower than 2 R)
                        if (x < 0) x += nx;
                    }
                    v[u] = src[x];
                }
            }
#pragma unroll
            for (int u = 0; u < 8; ++u) {
                const u64 word = __ballot(v[u] != 0);
                if (lane == 0 && w0 + 4 * u < Wp) packed[(size_t)r * Wp + w0 + 4 * u] = word;
            }
        }
    }
}

// out = dilate(in) with the disk of radius R (half-width hw[|dy|] at row offset dy), the outside of the image
// counting as `outside` (0 or ~0); invert: operate on the complement and complement the result (= erosion).
__global__ void __launch_bounds__(256)
k_morph_pass(const u64* __restrict__ in, u64* __restrict__ out, long T, int Hp, int Wp, int nxp, int R,
             const int* __restrict__ hw, int invert) {
    const long idx = (long)blockIdx.x * 256 + threadIdx.x;
    const long nwords = T * Hp * (long)Wp;
    if (idx >= nwords) return;
    const int w = (int)(idx % Wp);
    const long ty = idx / Wp;
    const int yy = (int)(ty % Hp);
    const long t = ty / Hp;
    const u64 flip = invert ? ~0ull : 0ull;      // complementing turns the stored 0 padding bits into the 1 outside
    const u64 outside = flip;
    const u64* img = in + (size_t)t * Hp * Wp;
    u64 acc = 0;
    for (int dy = -R; dy <= R; ++dy) {
        const int y = yy + dy;
        u64 L = outside, M = outside, Rw = outside;
        if (y >= 0 && y < Hp) {
            const u64* row = img + (size_t)y * Wp;
            M = row[w] ^ flip;
            if (w > 0) L = row[w - 1] ^ flip;
            if (w + 1 < Wp) Rw = row[w + 1] ^ flip;
        }
        const int wd = hw[dy < 0 ? -dy : dy];
        u64 d = M;
        for (int k = 1; k <= wd; ++k) d |= (M >> k) | (Rw << (64 - k)) | (M << k) | (L >> (64 - k));
        acc |= d;
    }
    acc ^= flip;
    // keep the bits past the row end at 0
    const int last_bits = nxp - 64 * (Wp - 1);
    if (w == Wp - 1 && last_bits < 64) acc &= (1ull << last_bits) - 1ull;
    out[idx] = acc;
}

// eight consecutive cells of a row per thread: 8 bits taken from one or two packed words, spread to bytes, ANDed with
// the ocean mask, one 8-byte store where `wide` says so (the host's decision: nx a multiple of 8 AND mask and out 8-byte
// aligned, so that every group of every row is), byte by byte otherwise
__global__ void __launch_bounds__(256)
k_morph_unpack(const u64* __restrict__ packed, const unsigned char* __restrict__ mask, long T, int ny, int nx, int R,
               int Hp, int Wp, int wide, unsigned char* __restrict__ out) {
    const int ng = (nx + 7) >> 3;  // groups of 8 cells per row
    const long idx = (long)blockIdx.x * 256 + threadIdx.x;
    if (idx >= T * ny * (long)ng) return;
    const int g = (int)(idx % ng);
    const long ty = idx / ng;
    const int y = (int)(ty % ny);
    const long t = ty / ny;
    const int x = g * 8, xx = x + 2 * R, yy = y + 2 * R;
    const u64* row = packed + ((size_t)t * Hp + yy) * Wp;
    const int w = xx >> 6, sh = xx & 63;
    u64 bits = row[w] >> sh;
    if (sh > 56 && w + 1 < Wp) bits |= row[w + 1] << (64 - sh);
    const unsigned char* mrow = mask + (size_t)y * nx + x;
    unsigned char* orow = out + ((size_t)t * ny + y) * nx + x;
    if (wide) {  // nx % 8 == 0: every group is whole
        u64 spread = 0;  // byte i = bit i
#pragma unroll
        for (int i = 0; i < 8; ++i) spread |= ((bits >> i) & 1ull) << (8 * i);
        const u64 m = *reinterpret_cast<const u64*>(mrow);
        // mask bytes are 0 / 1
        *reinterpret_cast<u64*>(orow) = spread & m;
    } else {
        for (int i = 0; i < 8 && x + i < nx; ++i) orow[i] = (((bits >> i) & 1ull) && mrow[i]) ? 1 : 0;
    }
}

__global__ void __launch_bounds__(256)
k_mask_and(const unsigned char* __restrict__ data, const unsigned char* __restrict__ mask, long T, long C,
           unsigned char* __restrict__ out) {
    const long idx = (long)blockIdx.x * 256 + threadIdx.x;
    if (idx >= T * C) return;
    out[idx] = (data[idx] && mask[idx % C]) ? 1 : 0;
}

// temporal closing with a centred window of 2c+1 steps, False outside the series (track.py:1694-1718: kernel of
// T_fill + 1 ones, T_fill even, padding of T_fill + 1 steps so that the border is never reached).
// One thread = 16 consecutive cells x a block of timesteps; bytes are 0 / 1, so OR / AND act on whole 16-byte vectors.
// The dilated rows of the block (+ c on either side) are kept in a small register ring.
#define TC_MAXC 8
#define TC_TBLOCK 32
__device__ __forceinline__ uint4 or4(uint4 a, uint4 b) { return make_uint4(a.x | b.x, a.y | b.y, a.z | b.z, a.w | b.w); }
__device__ __forceinline__ uint4 and4(uint4 a, uint4 b) { return make_uint4(a.x & b.x, a.y & b.y, a.z & b.z, a.w & b.w); }

__global__ void __launch_bounds__(256)
k_time_closing16(const unsigned char* __restrict__ data, long T, long C, int c, unsigned char* __restrict__ out) {
    const long c16 = ((long)blockIdx.x * 256 + threadIdx.x) * 16;
    if (c16 >= C) return;
    const long t0 = (long)blockIdx.y * TC_TBLOCK;
    const long t1 = t0 + TC_TBLOCK < T ? t0 + TC_TBLOCK : T;
    auto row = [&](long t) {
        return (t >= 0 && t < T) ? *reinterpret_cast<const uint4*>(data + (size_t)t * C + c16) : make_uint4(0, 0, 0, 0);
    };
    auto dil = [&](long t) {  // OR of rows t-c .. t+c; zero outside the series (the padded part of the reference's array)
        if (t < -(long)c - 1 || t > T + c) return make_uint4(0, 0, 0, 0);
        uint4 d = row(t - c);
        for (int i = -c + 1; i <= c; ++i) d = or4(d, row(t + i));
        return d;
    };
    for (long t = t0; t < t1; ++t) {
        uint4 e = dil(t - c);
        for (int j = -c + 1; j <= c; ++j) e = and4(e, dil(t + j));
        *reinterpret_cast<uint4*>(out + (size_t)t * C + c16) = e;
    }
}

__global__ void __launch_bounds__(256)
k_time_closing(const unsigned char* __restrict__ data, long T, long C, int c, unsigned char* __restrict__ out) {
    const long idx = (long)blockIdx.x * 256 + threadIdx.x;
    if (idx >= T * C) return;
    const long cell = idx % C, t = idx / C;
    bool all = true;
    for (int j = -c; j <= c && all; ++j) {  // erosion of ...
        bool any = false;
        for (int i = -c; i <= c; ++i) {      // ... the dilation
            const long tt = t + j + i;
            if (tt >= 0 && tt < T && data[(size_t)tt * C + cell]) any = true;
        }
        all = any;
    }
    out[idx] = all ? 1 : 0;
}

static int ensure_scratch(marex_ctx* ctx, size_t need) {
    HIP_TRY(ctx, grow_scratch(ctx->morph_scratch, ctx->morph_scratch_bytes, need));
    return 0;
}

extern "C" int marex_fill_holes_u8(marex_ctx* ctx, const uint8_t* data, const uint8_t* mask, int64_t T, int ny, int nx,
                                   int R, int regional_mode, uint8_t* out) {
    if (!ctx) return -1;
    if (!data || !mask || !out || T <= 0 || ny <= 0 || nx <= 0) return fail(ctx, -1, "marex_fill_holes_u8: null pointer or empty shape");
    if (R < 0 || R > 63) return fail(ctx, -4, "marex_fill_holes_u8: R_fill must be in 0..63");
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    LaunchTimer lt(ctx, MAREX_K_MORPH);
    const long C = (long)ny * nx;
    if (R == 0) {  // no morphology, only the land mask (track.py:1620-1621, 1674)
        hipLaunchKernelGGL(k_mask_and, dim3((unsigned)((T * C + 255) / 256)), dim3(256), 0, ctx->stream, data, mask, (long)T, C, out);
        HIP_TRY(ctx, hipGetLastError());
        return 0;
    }
    const int Hp = ny + 4 * R, nxp = nx + 4 * R, Wp = (nxp + 63) / 64;
    const size_t words = (size_t)T * Hp * Wp;
    const size_t need = 2 * words * sizeof(u64) + 64 * sizeof(int);
    if (int rc = ensure_scratch(ctx, need)) return rc;
    u64* a = reinterpret_cast<u64*>(ctx->morph_scratch);
    u64* b = a + words;
    int* hw_dev = reinterpret_cast<int*>(b + words);
    int hw[64];
    for (int dy = 0; dy <= R; ++dy) {  // se_kernel = x^2 + y^2 < R^2 + 1  (track.py:1613-1616)
        int w = 0;
        while ((w + 1) * (w + 1) + dy * dy < R * R + 1) ++w;
        hw[dy] = w;
    }
    HIP_TRY(ctx, hipMemcpyAsync(hw_dev, hw, (R + 1) * sizeof(int), hipMemcpyHostToDevice, ctx->stream));
    HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));  // hw lives on this stack frame
    const unsigned gw = (unsigned)((words + 255) / 256);
    hipLaunchKernelGGL(k_morph_pack, dim3((unsigned)((long)T * Hp < 1048576 ? (long)T * Hp : 1048576)), dim3(256), 0, ctx->stream, data, (long)T, ny, nx, R, regional_mode, Hp, Wp, a);
    hipLaunchKernelGGL(k_morph_pass, dim3(gw), dim3(256), 0, ctx->stream, a, b, (long)T, Hp, Wp, nxp, R, hw_dev, 0);  // closing:
    hipLaunchKernelGGL(k_morph_pass, dim3(gw), dim3(256), 0, ctx->stream, b, a, (long)T, Hp, Wp, nxp, R, hw_dev, 1);  //   dilate, erode
    hipLaunchKernelGGL(k_morph_pass, dim3(gw), dim3(256), 0, ctx->stream, a, b, (long)T, Hp, Wp, nxp, R, hw_dev, 1);  // opening:
    hipLaunchKernelGGL(k_morph_pass, dim3(gw), dim3(256), 0, ctx->stream, b, a, (long)T, Hp, Wp, nxp, R, hw_dev, 0);  //   erode, dilate
    // a view at an odd offset is a valid mask or output: the 8-byte accesses are taken on pointer alignment too
    const int wide = (nx & 7) == 0 && (((uintptr_t)mask | (uintptr_t)out) & 7) == 0;
    hipLaunchKernelGGL(k_morph_unpack, dim3((unsigned)((T * ny * (long)((nx + 7) / 8) + 255) / 256)), dim3(256), 0, ctx->stream, a,
                       mask, (long)T, ny, nx, R, Hp, Wp, wide, out);
    HIP_TRY(ctx, hipGetLastError());
    return 0;
}

extern "C" int marex_time_closing_u8(marex_ctx* ctx, const uint8_t* data, int64_t T, int64_t C, int T_fill, uint8_t* out) {
    if (!ctx) return -1;
    if (!data || !out || T <= 0 || C <= 0) return fail(ctx, -1, "marex_time_closing_u8: null pointer or empty shape");
    if (T_fill < 0 || (T_fill & 1)) return fail(ctx, -1, "marex_time_closing_u8: T_fill must be even and >= 0");
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    LaunchTimer lt(ctx, MAREX_K_MORPH);
    if ((C & 15) == 0 && (((uintptr_t)data | (uintptr_t)out) & 15) == 0) {
        dim3 grid((unsigned)((C / 16 + 255) / 256), (unsigned)((T + TC_TBLOCK - 1) / TC_TBLOCK));
        hipLaunchKernelGGL(k_time_closing16, grid, dim3(256), 0, ctx->stream, data, (long)T, (long)C, T_fill / 2, out);
    } else {
        hipLaunchKernelGGL(k_time_closing, dim3((unsigned)((T * C + 255) / 256)), dim3(256), 0, ctx->stream, data, (long)T, (long)C,
                           T_fill / 2, out);
    }
    HIP_TRY(ctx, hipGetLastError());
    return 0;
}

// ------------------------------------------------------------------------------------------------
// Connected components per timestep (track.py:1912-2049 structured branch with time_connectivity = False: 8-connected
// in (y, x), periodic in x unless regional) and the area filter of filter_small_objects (track.py:1755-1911).
//
// Label of a cell = 1 + the smallest linear index (over the whole [T, ny, nx] array) of its component, 0 = background:
// concurrent union-find, one merge pass over the four "backward" neighbours (W, NW, N, NE), a compression pass, and a
// flattening pass that also accumulates the areas at the roots.  Label VALUES differ from scipy's scan-order numbering; memberships and areas do not.
// ------------------------------------------------------------------------------------------------
// Union-find in the style of ECL-CC: a root is hooked under a smaller root with ONE compare-and-swap that only succeeds
// while it is still a root; finds shorten the paths they walk with plain stores (path halving) -- safe because only
// non-roots are rewritten (a non-root never becomes a root again, so it can never be the target of a hook) and the new
// parent is always one of its ancestors.  Parents only decrease, so every loop terminates.
__device__ __forceinline__ int uf_find(int* __restrict__ parent, int i) {
    int p = parent[i];
    while (p != i) {
        const int g = parent[p];
        if (g != p) parent[i] = g;
        i = p;
        p = g;
    }
    return i;
}

__device__ __forceinline__ void uf_union(int* __restrict__ parent, int a, int b) {
    a = uf_find(parent, a);
    b = uf_find(parent, b);
    while (a != b) {
        if (a < b) {
            const int s = a;
            a = b;
            b = s;
        }
        const int old = atomicCAS(&parent[a], a, b);  // a > b: hook a under b if a is still a root
        if (old == a) return;
        a = uf_find(parent, old);  // a was hooked elsewhere meanwhile: continue from its new root
        b = uf_find(parent, b);
    }
}

// Initial parents: every True cell points at the first cell of its horizontal run inside its wave's 64 consecutive
// cells (ballot + count-leading-zeros, no memory traffic) -- most "west" unions never have to happen.
__global__ void __launch_bounds__(256)
k_ccl_init(const unsigned char* __restrict__ data, long n, int nx, int* __restrict__ parent) {
    const long i = (long)blockIdx.x * 256 + threadIdx.x;
    const int lane = threadIdx.x & 63;
    const bool on = i < n && data[i];
    const bool row_start = i < n && (i % nx) == 0;
    const unsigned long long on_m = __ballot(on);
    // lane continues the run of lane-1: both set, same row
    const unsigned long long cont = on_m & (on_m << 1) & ~__ballot(row_start);
    if (i >= n) return;
    if (!on) {
        parent[i] = -1;
        return;
    }
    const unsigned long long upto = lane == 63 ? ~0ull : ((2ull << lane) - 1ull);
    const unsigned long long breaks = ~cont & upto;  // bit 0 is always a break (cont has bit 0 clear)
    const int start = 63 - __clzll((long long)breaks);
    parent[i] = (int)(i - lane + start);
}

__global__ void __launch_bounds__(256)
k_ccl_merge(const unsigned char* __restrict__ data, long T, int ny, int nx, int wrap_x, int* __restrict__ parent) {
    const long i = (long)blockIdx.x * 256 + threadIdx.x;
    const long n = T * ny * (long)nx;
    if (i >= n || !data[i]) return;
    const int x = (int)(i % nx);
    const int y = (int)((i / nx) % ny);
    const long base = i - x;  // start of this row
    // west: only where the in-wave run labelling could not see it (first lane of a wave) and across the periodic seam
    if (x > 0) {
        if ((threadIdx.x & 63) == 0 && data[i - 1]) uf_union(parent, (int)i, (int)(i - 1));
    } else if (wrap_x && nx > 1 && data[base + nx - 1]) {
        uf_union(parent, (int)i, (int)(base + nx - 1));
    }
    if (y > 0) {
        // One union per OVERLAP of a run with a run of the row above, not one per cell: a cell links to N only where
        // the overlap starts (its W neighbour is not part of the same overlap), to NW / NE only at run ends where the
        // diagonal is the sole contact.  In blobs that cover half the ocean this removes >90 % of the finds.
        const long up = base - nx;
        int xw = x - 1, xe = x + 1;
        bool okw = true, oke = true;
        if (xw < 0) {
            okw = wrap_x && nx > 1;
            xw += nx;
        }
        if (xe >= nx) {
            oke = wrap_x && nx > 1;
            xe -= nx;
        }
        const bool n_ = data[up + x] != 0;
        const bool nw = okw && data[up + xw] != 0, ne = oke && data[up + xe] != 0;
        const bool w_ = okw && data[base + xw] != 0, e_ = oke && data[base + xe] != 0;
        // x == 0 always links on its own account: on a periodic row an overlap may have no beginning otherwise
        const bool chain = x > 0;
        if (n_) {
            if (!(chain && w_ && nw)) uf_union(parent, (int)i, (int)(up + x));
        } else {
            if (nw && !(chain && w_)) uf_union(parent, (int)i, (int)(up + xw));
            if (ne && !e_) uf_union(parent, (int)i, (int)(up + xe));
        }
    }
}

// after all unions: point every cell straight at its root (plain stores are fine: nothing is merged any more)
__global__ void __launch_bounds__(256)
k_ccl_compress(long n, int* __restrict__ parent) {
    const long i = (long)blockIdx.x * 256 + threadIdx.x;
    if (i >= n || parent[i] < 0) return;
    int r = (int)i, p = parent[i];
    while (p != r) {
        r = p;
        p = parent[r];
    }
    parent[i] = r;
}

// labels + areas; the lanes of a wave that share a root add their count with ONE atomic (a blob covering half the
// ocean would otherwise serialise hundreds of thousands of atomics on one address)
__global__ void __launch_bounds__(256)
k_ccl_flatten(long n, const int* __restrict__ parent, int* __restrict__ labels, int* __restrict__ areas) {
    const long i = (long)blockIdx.x * 256 + threadIdx.x;
    int r = -1;
    if (i < n) {
        r = parent[i];
        labels[i] = r < 0 ? 0 : r + 1;
    }
    unsigned long long todo = __ballot(r >= 0);
    while (todo) {
        const int lead = __ffsll((long long)todo) - 1;
        const int rl = __shfl(r, lead, 64);
        const unsigned long long same = __ballot(r == rl) & todo;
        if ((int)(threadIdx.x & 63) == lead) atomicAdd(&areas[rl], __popcll(same));
        todo &= ~same;
    }
}

__global__ void __launch_bounds__(256)
k_ccl_filter(const int* __restrict__ labels, const int* __restrict__ areas, long n, double area_threshold, int drop_label,
             unsigned char* __restrict__ out) {
    const long i = (long)blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    const int l = labels[i];
    out[i] = (l > 0 && l != drop_label && (double)areas[l - 1] >= area_threshold) ? 1 : 0;
}

extern "C" int marex_label2d_i32(marex_ctx* ctx, const uint8_t* data, int64_t T, int ny, int nx, int wrap_x,
                                 int32_t* labels, int32_t* areas) {
    if (!ctx) return -1;
    if (!data || !labels || !areas || T <= 0 || ny <= 0 || nx <= 0) return fail(ctx, -1, "marex_label2d_i32: null pointer or empty shape");
    const long n = (long)T * ny * nx;
    if (n >= 2147483647L) return fail(ctx, -4, "marex_label2d_i32: more than 2^31 - 1 cells; label the series in time blocks");
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    LaunchTimer lt(ctx, MAREX_K_MORPH);
    const unsigned g = (unsigned)((n + 255) / 256);
    // `labels` doubles as the parent array during the merge; `areas` must start at zero
    HIP_TRY(ctx, hipMemsetAsync(areas, 0, (size_t)n * sizeof(int), ctx->stream));
    hipLaunchKernelGGL(k_ccl_init, dim3(g), dim3(256), 0, ctx->stream, data, n, nx, labels);
    hipLaunchKernelGGL(k_ccl_merge, dim3(g), dim3(256), 0, ctx->stream, data, (long)T, ny, nx, wrap_x, labels);
    // flatten in place is a race (a cell's parent may be overwritten by its label while another walks through it):
    // write the labels to `areas`' sibling buffer instead -- here: a scratch copy of the parents
    if (int rc = ensure_scratch(ctx, (size_t)n * sizeof(int))) return rc;
    int* parent = reinterpret_cast<int*>(ctx->morph_scratch);
    hipLaunchKernelGGL(k_ccl_compress, dim3(g), dim3(256), 0, ctx->stream, n, labels);
    HIP_TRY(ctx, hipMemcpyAsync(parent, labels, (size_t)n * sizeof(int), hipMemcpyDeviceToDevice, ctx->stream));
    hipLaunchKernelGGL(k_ccl_flatten, dim3(g), dim3(256), 0, ctx->stream, n, parent, labels, areas);
    HIP_TRY(ctx, hipGetLastError());
    return 0;
}

// ------------------------------------------------------------------------------------------------
// Connected components in (time, y, x) (track.py:2006-2048 structured branch with time_connectivity = True: the 3x3x3
// structure of ones, periodic in x unless regional) with compact IDs in the reference's order.
//
// Same union-find as above.  A cell's neighbourhood at t-1 is three more "rows above" -- (t-1, y-1), (t-1, y),
// (t-1, y+1) -- each seen through the same N / NW / NE window as the row (t, y-1), so the one-union-per-overlap rule
// carries over unchanged: the W / E cell of the current row sees the same row through a window shifted by one.
// ------------------------------------------------------------------------------------------------
__device__ __forceinline__ void ccl_link_row(const unsigned char* __restrict__ data, int* __restrict__ parent, long i,
                                             long up, int x, int xw, int xe, bool okw, bool oke, bool chain, bool w_,
                                             bool e_) {
    const bool n_ = data[up + x] != 0;
    const bool nw = okw && data[up + xw] != 0, ne = oke && data[up + xe] != 0;
    if (n_) {
        if (!(chain && w_ && nw)) uf_union(parent, (int)i, (int)(up + x));
    } else {
        if (nw && !(chain && w_)) uf_union(parent, (int)i, (int)(up + xw));
        if (ne && !e_) uf_union(parent, (int)i, (int)(up + xe));
    }
}

// connect_t = 0: the rows at t-1 are skipped (the per-timestep labelling of time_connectivity = False)
__global__ void __launch_bounds__(256)
k_ccl_merge3d(const unsigned char* __restrict__ data, long T, int ny, int nx, int wrap_x, int connect_t,
              int* __restrict__ parent) {
    const long i = (long)blockIdx.x * 256 + threadIdx.x;
    const long C = (long)ny * nx;
    if (i >= T * C || !data[i]) return;
    const int x = (int)(i % nx);
    const long ty = i / nx;
    const int y = (int)(ty % ny);
    const long t = ty / ny;
    const long base = i - x;
    const bool wrap = wrap_x && nx > 1;
    if (x > 0) {
        if ((threadIdx.x & 63) == 0 && data[i - 1]) uf_union(parent, (int)i, (int)(i - 1));
    } else if (wrap && data[base + nx - 1]) {
        uf_union(parent, (int)i, (int)(base + nx - 1));
    }
    const bool has_up = y > 0, has_prev = connect_t && t > 0;
    if (!has_up && !has_prev) return;
    int xw = x - 1, xe = x + 1;
    bool okw = true, oke = true;
    if (xw < 0) {
        okw = wrap;
        xw += nx;
    }
    if (xe >= nx) {
        oke = wrap;
        xe -= nx;
    }
    const bool w_ = okw && data[base + xw] != 0, e_ = oke && data[base + xe] != 0;
    const bool chain = x > 0;  // x == 0 always links on its own account (a periodic overlap may have no beginning)
    if (has_up) ccl_link_row(data, parent, i, base - nx, x, xw, xe, okw, oke, chain, w_, e_);
    if (has_prev) {
        const long prev = base - C;  // (t-1, y)
        if (y > 0) ccl_link_row(data, parent, i, prev - nx, x, xw, xe, okw, oke, chain, w_, e_);
        ccl_link_row(data, parent, i, prev, x, xw, xe, okw, oke, chain, w_, e_);
        if (y + 1 < ny) ccl_link_row(data, parent, i, prev + nx, x, xw, xe, okw, oke, chain, w_, e_);
    }
}

// Compact numbering: after compression a root is the component's smallest linear index (hooks always go to the
// smaller root), i.e. its first voxel in C order, and ID = 1 + rank of the root among all roots -- scipy.ndimage.label's
// scan order, which dask_image keeps by offsetting the block labels in time order and relabelling through
// connected_components (components numbered by their smallest provisional label).
// One workgroup counts (RANK = false) or ranks (RANK = true) the roots of CCL_TILE consecutive cells: a ballot and a
// popcount per wave and 256 cells, the four wave counts combined in LDS, in index order.
#define CCL_TILE 4096
template <bool RANK>
__global__ void __launch_bounds__(256)
k_ccl_roots(const int* __restrict__ parent, long n, const int* __restrict__ tile_off, int* __restrict__ tile_cnt,
            int* __restrict__ rank) {
    __shared__ int wcnt[4];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const long tile0 = (long)blockIdx.x * CCL_TILE;
    int run = RANK ? tile_off[blockIdx.x] : 0;
    for (int k = 0; k < CCL_TILE / 256; ++k) {
        const long i = tile0 + k * 256 + threadIdx.x;
        const bool root = i < n && parent[i] == (int)i;
        const unsigned long long b = __ballot(root);
        if (lane == 0) wcnt[wave] = __popcll(b);
        __syncthreads();
        if (RANK && root) {
            int before = run + __popcll(b & ((1ull << lane) - 1ull));
            for (int w = 0; w < wave; ++w) before += wcnt[w];
            rank[i] = before;
        }
        run += wcnt[0] + wcnt[1] + wcnt[2] + wcnt[3];
        __syncthreads();
    }
    if (!RANK && threadIdx.x == 0) tile_cnt[blockIdx.x] = run;
}

// exclusive scan of the tile counts by one workgroup (a few hundred thousand tiles at most); n_out = the total
__global__ void __launch_bounds__(1024)
k_ccl_scan_tiles(const int* __restrict__ cnt, long ntiles, int* __restrict__ off, int* __restrict__ n_out) {
    __shared__ int part[1024];
    const long per = (ntiles + 1023) / 1024;
    const long a = threadIdx.x * per, b = a + per < ntiles ? a + per : ntiles;
    int s = 0;
    for (long j = a; j < b; ++j) s += cnt[j];
    part[threadIdx.x] = s;
    __syncthreads();
    for (int d = 1; d < 1024; d <<= 1) {  // Hillis-Steele inclusive scan of the 1024 partial sums
        const int v = threadIdx.x >= (unsigned)d ? part[threadIdx.x - d] : 0;
        __syncthreads();
        part[threadIdx.x] += v;
        __syncthreads();
    }
    int run = part[threadIdx.x] - s;
    for (long j = a; j < b; ++j) {
        const int c = cnt[j];
        off[j] = run;
        run += c;
    }
    if (threadIdx.x == 1023) *n_out = part[1023];
}

// ids[i] = 1 + rank[root of i] in place (each thread reads and writes only its own element), areas[id - 1] += cells
// with one atomic per (wave, id)
__global__ void __launch_bounds__(256)
k_ccl_relabel(long n, const int* __restrict__ rank, int* __restrict__ ids, int* __restrict__ areas) {
    const long i = (long)blockIdx.x * 256 + threadIdx.x;
    int id = 0;
    if (i < n) {
        const int r = ids[i];
        id = r < 0 ? 0 : rank[r] + 1;
        ids[i] = id;
    }
    unsigned long long todo = __ballot(id > 0);
    while (todo) {
        const int lead = __ffsll((long long)todo) - 1;
        const int il = __shfl(id, lead, 64);
        const unsigned long long same = __ballot(id == il) & todo;
        if ((int)(threadIdx.x & 63) == lead) atomicAdd(&areas[il - 1], __popcll(same));
        todo &= ~same;
    }
}

extern "C" int marex_label3d_i32(marex_ctx* ctx, const uint8_t* data, int64_t T, int ny, int nx, int wrap_x, int connect_t,
                                 int32_t* ids, int32_t* areas, int32_t* n_out) {
    if (!ctx) return -1;
    if (!data || !ids || !areas || !n_out || T <= 0 || ny <= 0 || nx <= 0) return fail(ctx, -1, "marex_label3d_i32: null pointer or empty shape");
    const long n = (long)T * ny * nx;
    if (n >= 2147483647L) return fail(ctx, -4, "marex_label3d_i32: more than 2^31 - 1 cells; label the series in time blocks");
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    LaunchTimer lt(ctx, MAREX_K_MORPH);
    const unsigned g = (unsigned)((n + 255) / 256);
    const long ntiles = (n + CCL_TILE - 1) / CCL_TILE;
    // scratch: rank [n] (written at the roots only), tile counts and tile offsets [ntiles] each
    if (int rc = ensure_scratch(ctx, (size_t)(n + 2 * ntiles) * sizeof(int))) return rc;
    int* rank = reinterpret_cast<int*>(ctx->morph_scratch);
    int* tile_cnt = rank + n;
    int* tile_off = tile_cnt + ntiles;
    HIP_TRY(ctx, hipMemsetAsync(areas, 0, (size_t)n * sizeof(int), ctx->stream));
    // `ids` is the parent array until the relabelling
    hipLaunchKernelGGL(k_ccl_init, dim3(g), dim3(256), 0, ctx->stream, data, n, nx, ids);
    hipLaunchKernelGGL(k_ccl_merge3d, dim3(g), dim3(256), 0, ctx->stream, data, (long)T, ny, nx, wrap_x, connect_t, ids);
    hipLaunchKernelGGL(k_ccl_compress, dim3(g), dim3(256), 0, ctx->stream, n, ids);
    hipLaunchKernelGGL(k_ccl_roots<false>, dim3((unsigned)ntiles), dim3(256), 0, ctx->stream, ids, n, tile_off, tile_cnt, rank);
    hipLaunchKernelGGL(k_ccl_scan_tiles, dim3(1), dim3(1024), 0, ctx->stream, tile_cnt, ntiles, tile_off, n_out);
    hipLaunchKernelGGL(k_ccl_roots<true>, dim3((unsigned)ntiles), dim3(256), 0, ctx->stream, ids, n, tile_off, tile_cnt, rank);
    hipLaunchKernelGGL(k_ccl_relabel, dim3(g), dim3(256), 0, ctx->stream, n, rank, ids, areas);
    HIP_TRY(ctx, hipGetLastError());
    return 0;
}

// ------------------------------------------------------------------------------------------------
// Labelling in time blocks (fields of 2^31 - 1 cells and more): every block of timesteps is labelled on its own by
// marex_label3d_i32 (local IDs 1..n_k by first cell inside the block), block k's provisional global IDs are
// off_k + local with off_k = n_0 + ... + n_{k-1} -- already the global first-cell order, because every cell of block k
// precedes every cell of block k+1 -- and the seams are stitched at OBJECT level: a parent table over the provisional
// IDs (entry 0 = background, a root of its own), the same hook-to-the-smaller-root union-find as the cells', so that a
// root is the smallest provisional ID of its event = the one whose first cell comes first.  Ranking the roots of the
// table then is the single call's numbering (dask_image.ndmeasure.label does the same on the host: block labels offset
// in time order, joined through connected components of the seam pairs).
// ------------------------------------------------------------------------------------------------
// One thread per cell of the later slice (`next`, first step of block k+1): it looks at its up to nine neighbours in the
// earlier slice (`prev`, last step of block k), 3 x 3 in (y, x), x periodic with wrap_x.  Shared addresses: a lane
// skips a neighbour that repeats its previous one, and the lanes of a wave that hold the same (earlier, later) pair
// send ONE union (ballot, as in k_ccl_relabel); a pair that is already joined costs two finds and no atomic.  IDs
// outside 1..n_prev / 1..n_next count as background, so no table access can leave [0, off_next + n_next].
__global__ void __launch_bounds__(256)
k_seam_union(const int* __restrict__ prev, const int* __restrict__ next, int ny, int nx, int wrap_x, int off_prev,
             int n_prev, int off_next, int n_next, int* __restrict__ table) {
    const long C = (long)ny * nx;
    const long i = (long)blockIdx.x * 256 + threadIdx.x;
    const int lane = threadIdx.x & 63;
    const bool wrap = wrap_x && nx > 1;
    int b = 0, x = 0, y = 0;
    if (i < C) {
        const int v = next[i];
        if (v > 0 && v <= n_next) b = off_next + v;
        x = (int)(i % nx);
        y = (int)(i / nx);
    }
    int last = 0;
    for (int d = 0; d < 9; ++d) {  // uniform trip count: every lane takes part in the ballots
        int a = 0;
        if (b) {
            const int yy = y + d / 3 - 1;
            int xx = x + d % 3 - 1;
            bool ok = yy >= 0 && yy < ny;
            if (xx < 0) {
                ok = ok && wrap;
                xx += nx;
            } else if (xx >= nx) {
                ok = ok && wrap;
                xx -= nx;
            }
            if (ok) {
                const int p = prev[(long)yy * nx + xx];
                if (p > 0 && p <= n_prev) a = off_prev + p;
            }
            if (a == last) a = 0;
            else if (a) last = a;
        }
        unsigned long long todo = __ballot(a != 0);
        while (todo) {
            const int lead = __ffsll((long long)todo) - 1;
            const int al = __shfl(a, lead, 64), bl = __shfl(b, lead, 64);
            const unsigned long long same = __ballot(a == al && b == bl) & todo;
            if (lane == lead) uf_union(table, al, bl);
            todo &= ~same;
        }
    }
}

// table[g] = final ID of provisional ID g (rank[] holds, at the roots, the number of roots before them -- entry 0
// included, so that it IS the 1-based final ID and final[0] = 0); each thread rewrites only its own entry.  The block
// areas fold into the events' areas in int64: one event of such a field may exceed 2^31 cells.
__global__ void __launch_bounds__(256)
k_table_final(long len, const int* __restrict__ rank, const int* __restrict__ n_roots, int* __restrict__ table,
              const int* __restrict__ prov_areas, unsigned long long* __restrict__ areas, int* __restrict__ n_out) {
    const long g = (long)blockIdx.x * 256 + threadIdx.x;
    if (g >= len) return;
    if (g == 0) *n_out = *n_roots - 1;  // the background entry is a root too
    const int f = rank[table[g]];
    table[g] = f;
    if (g > 0 && f > 0) atomicAdd(&areas[f - 1], (unsigned long long)prov_areas[g - 1]);
}

// ids[i] = ids[i] > 0 ? table[off + ids[i]] : 0 in place: 16 bytes per thread where the slice allows it, the `head`
// elements before the first 16-byte boundary and the rest behind the last full vector one by one
__device__ __forceinline__ int table_map(const int* __restrict__ table, long table_len, int off, int v) {
    const long g = (long)off + v;
    return (v > 0 && g < table_len) ? table[g] : 0;
}

__global__ void __launch_bounds__(256)
k_label_apply(int* __restrict__ ids, long n, int head, const int* __restrict__ table, long table_len, int off) {
    const long idx = (long)blockIdx.x * 256 + threadIdx.x;
    const long nvec = (n - head) / 4;
    if (idx < nvec) {
        int4* p = reinterpret_cast<int4*>(ids + head) + idx;
        int4 v = *p;
        v.x = table_map(table, table_len, off, v.x);
        v.y = table_map(table, table_len, off, v.y);
        v.z = table_map(table, table_len, off, v.z);
        v.w = table_map(table, table_len, off, v.w);
        *p = v;
        return;
    }
    const long j = idx - nvec;
    const long e = j < head ? j : head + 4 * nvec + (j - head);
    if (e < n) ids[e] = table_map(table, table_len, off, ids[e]);
}

extern "C" int marex_label_seam_union_i32(marex_ctx* ctx, const int32_t* prev_ids, const int32_t* next_ids, int ny, int nx,
                                          int wrap_x, int off_prev, int n_prev, int off_next, int n_next, int32_t* table,
                                          int64_t table_len) {
    if (!ctx) return -1;
    if (!prev_ids || !next_ids || !table || ny <= 0 || nx <= 0) return fail(ctx, -1, "marex_label_seam_union_i32: null pointer or empty shape");
    if ((long)ny * nx >= 2147483647L) return fail(ctx, -4, "marex_label_seam_union_i32: a slice of 2^31 - 1 cells or more");
    if (off_prev < 0 || n_prev < 0 || off_next < 0 || n_next < 0 || (long)off_prev + n_prev >= table_len ||
        (long)off_next + n_next >= table_len || table_len > 2147483647L)
        return fail(ctx, -4, "marex_label_seam_union_i32: ID ranges outside the table (off + n must stay below table_len <= 2^31 - 1)");
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    LaunchTimer lt(ctx, MAREX_K_MORPH);
    const long C = (long)ny * nx;
    hipLaunchKernelGGL(k_seam_union, dim3((unsigned)((C + 255) / 256)), dim3(256), 0, ctx->stream, prev_ids, next_ids, ny, nx,
                       wrap_x, off_prev, n_prev, off_next, n_next, table);
    HIP_TRY(ctx, hipGetLastError());
    return 0;
}

extern "C" int marex_label_table_resolve_i32(marex_ctx* ctx, int32_t* table, int64_t n_prov, const int32_t* prov_areas,
                                             int64_t* areas, int32_t* n_out) {
    if (!ctx) return -1;
    if (!table || !prov_areas || !areas || !n_out || n_prov <= 0) return fail(ctx, -1, "marex_label_table_resolve_i32: null pointer or empty table");
    if (n_prov > 2147483646L) return fail(ctx, -4, "marex_label_table_resolve_i32: more than 2^31 - 2 provisional objects");
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    LaunchTimer lt(ctx, MAREX_K_MORPH);
    const long len = (long)n_prov + 1;  // entry 0 = background
    const unsigned g = (unsigned)((len + 255) / 256);
    const long ntiles = (len + CCL_TILE - 1) / CCL_TILE;
    // scratch: rank [len] (written at the roots only), tile counts and offsets [ntiles] each, the number of roots
    if (int rc = ensure_scratch(ctx, (size_t)(len + 2 * ntiles + 1) * sizeof(int))) return rc;
    int* rank = reinterpret_cast<int*>(ctx->morph_scratch);
    int* tile_cnt = rank + len;
    int* tile_off = tile_cnt + ntiles;
    int* n_roots = tile_off + ntiles;
    HIP_TRY(ctx, hipMemsetAsync(areas, 0, (size_t)n_prov * sizeof(int64_t), ctx->stream));
    hipLaunchKernelGGL(k_ccl_compress, dim3(g), dim3(256), 0, ctx->stream, len, table);
    hipLaunchKernelGGL(k_ccl_roots<false>, dim3((unsigned)ntiles), dim3(256), 0, ctx->stream, table, len, tile_off, tile_cnt, rank);
    hipLaunchKernelGGL(k_ccl_scan_tiles, dim3(1), dim3(1024), 0, ctx->stream, tile_cnt, ntiles, tile_off, n_roots);
    hipLaunchKernelGGL(k_ccl_roots<true>, dim3((unsigned)ntiles), dim3(256), 0, ctx->stream, table, len, tile_off, tile_cnt, rank);
    hipLaunchKernelGGL(k_table_final, dim3(g), dim3(256), 0, ctx->stream, len, rank, n_roots, table, prov_areas,
                       reinterpret_cast<unsigned long long*>(areas), n_out);
    HIP_TRY(ctx, hipGetLastError());
    return 0;
}

extern "C" int marex_label_apply_table_i32(marex_ctx* ctx, int32_t* ids, int64_t n, const int32_t* table, int64_t table_len,
                                           int off) {
    if (!ctx) return -1;
    if (!ids || !table || n <= 0 || table_len <= 0) return fail(ctx, -1, "marex_label_apply_table_i32: null pointer or empty shape");
    if (n >= 2147483647L) return fail(ctx, -4, "marex_label_apply_table_i32: a block of 2^31 - 1 cells or more");
    if (off < 0 || off >= table_len || table_len > 2147483647L) return fail(ctx, -4, "marex_label_apply_table_i32: offset outside the table");
    if ((uintptr_t)ids & 3) return fail(ctx, -4, "marex_label_apply_table_i32: ids must be 4-byte aligned");
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    LaunchTimer lt(ctx, MAREX_K_MORPH);
    long head = (long)(((16 - ((uintptr_t)ids & 15)) & 15) / 4);  // elements before the first 16-byte boundary
    if (head > n) head = n;
    const long nvec = (n - head) / 4;
    const long threads = nvec + head + (n - head - 4 * nvec);
    hipLaunchKernelGGL(k_label_apply, dim3((unsigned)((threads + 255) / 256)), dim3(256), 0, ctx->stream, ids, (long)n, (int)head,
                       table, (long)table_len, off);
    HIP_TRY(ctx, hipGetLastError());
    return 0;
}

extern "C" int marex_filter_by_area_u8(marex_ctx* ctx, const int32_t* labels, const int32_t* areas, int64_t n,
                                       double area_threshold, int drop_label, uint8_t* out) {
    if (!ctx) return -1;
    if (!labels || !areas || !out || n <= 0) return fail(ctx, -1, "marex_filter_by_area_u8: null pointer or empty shape");
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    LaunchTimer lt(ctx, MAREX_K_MORPH);
    hipLaunchKernelGGL(k_ccl_filter, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, ctx->stream, labels, areas, (long)n,
                       area_threshold, drop_label, out);
    HIP_TRY(ctx, hipGetLastError());
    return 0;
}

// ------------------------------------------------------------------------------------------------
// Unstructured meshes (track.py:1093-1117, 1543-1606, 1932-2004, 1776-1857): a cell's neighbourhood is itself plus up
// to three edge neighbours (nbr[3][C], 0-based, -1 = none); dilation by R = R sweeps of "OR over the neighbourhood".
// ------------------------------------------------------------------------------------------------
// pre-operation applied to every value read by the FIRST sweep of a group (fuses the reference's elementwise steps):
//   0: v                   1: !(v || land)      (b[:, ~mask] = True; ~b)
//   2: v && !land          (~(~v | land))       3: !v
__device__ __forceinline__ bool graph_pre(bool v, bool land, int pre) {
    return pre == 0 ? v : pre == 1 ? !(v || land) : pre == 2 ? (v && !land) : !v;
}

__global__ void __launch_bounds__(256)
k_graph_sweep(const unsigned char* __restrict__ in, const unsigned char* __restrict__ mask, const int* __restrict__ nbr,
              long T, long C, int pre, int dilate, unsigned char* __restrict__ out) {
    const long idx = (long)blockIdx.x * 256 + threadIdx.x;
    if (idx >= T * C) return;
    const long c = idx % C;
    const unsigned char* row = in + (idx - c);
    bool v = graph_pre(row[c] != 0, mask[c] == 0, pre);
    if (dilate) {
#pragma unroll
        for (int k = 0; k < 3; ++k) {
            const int n = nbr[(size_t)k * C + c];
            if (n >= 0) v = v || graph_pre(row[n] != 0, mask[n] == 0, pre);
        }
    }
    out[idx] = v ? 1 : 0;
}

extern "C" int marex_fill_holes_mesh_u8(marex_ctx* ctx, const uint8_t* data, const uint8_t* mask, const int32_t* nbr,
                                        int64_t T, int64_t C, int R, uint8_t* out) {
    if (!ctx) return -1;
    if (!data || !mask || !nbr || !out || T <= 0 || C <= 0) return fail(ctx, -1, "marex_fill_holes_mesh_u8: null pointer or empty shape");
    if (R < 0 || R > 1024) return fail(ctx, -4, "marex_fill_holes_mesh_u8: R_fill must be in 0..1024");
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    LaunchTimer lt(ctx, MAREX_K_MORPH);
    const size_t n = (size_t)T * C;
    if (int rc = ensure_scratch(ctx, 2 * n)) return rc;
    unsigned char* bufs[2] = {ctx->morph_scratch, ctx->morph_scratch + n};
    const unsigned g = (unsigned)((n + 255) / 256);
    const unsigned char* cur = data;
    int flip = 0;
    // dilation | (land := True, complement) dilation | (complement, land := True, complement) dilation | complement, dilation
    const int pres[4] = {0, 1, 2, 3};
    for (int grp = 0; grp < 4; ++grp) {
        const int sweeps = R > 0 ? R : 1;  // R = 0: only the elementwise step of the group
        for (int s = 0; s < sweeps; ++s) {
            const bool last = grp == 3 && s == sweeps - 1;
            unsigned char* dst = last ? out : bufs[flip];
            hipLaunchKernelGGL(k_graph_sweep, dim3(g), dim3(256), 0, ctx->stream, cur, mask, nbr, (long)T, (long)C,
                               s == 0 ? pres[grp] : 0, R > 0 ? 1 : 0, dst);
            cur = dst;
            flip ^= 1;
        }
    }
    HIP_TRY(ctx, hipGetLastError());
    return 0;
}

// connected components per timestep over the mesh edges, land excluded (track.py:1985, 1947-1981)
__global__ void __launch_bounds__(256)
k_mesh_ccl_init(const unsigned char* __restrict__ data, const unsigned char* __restrict__ mask, long T, long C,
                int* __restrict__ parent) {
    const long i = (long)blockIdx.x * 256 + threadIdx.x;
    if (i < T * C) parent[i] = (data[i] && mask[i % C]) ? (int)i : -1;
}

__global__ void __launch_bounds__(256)
k_mesh_ccl_merge(const int* __restrict__ nbr, long T, long C, int* __restrict__ parent) {
    const long i = (long)blockIdx.x * 256 + threadIdx.x;
    if (i >= T * C || parent[i] < 0) return;
    const long c = i % C, base = i - c;
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        const int n = nbr[(size_t)k * C + c];
        // an edge is an undirected link whichever end lists it (connected_components(directed=False), track.py:1979)
        if (n >= 0 && n != c && parent[base + n] >= 0) uf_union(parent, (int)i, (int)(base + n));
    }
}

extern "C" int marex_label_mesh_i32(marex_ctx* ctx, const uint8_t* data, const uint8_t* mask, const int32_t* nbr, int64_t T,
                                    int64_t C, int32_t* labels, int32_t* areas) {
    if (!ctx) return -1;
    if (!data || !mask || !nbr || !labels || !areas || T <= 0 || C <= 0) return fail(ctx, -1, "marex_label_mesh_i32: null pointer or empty shape");
    const long n = (long)T * C;
    if (n >= 2147483647L) return fail(ctx, -4, "marex_label_mesh_i32: more than 2^31 - 1 cells; label the series in time blocks");
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    LaunchTimer lt(ctx, MAREX_K_MORPH);
    const unsigned g = (unsigned)((n + 255) / 256);
    HIP_TRY(ctx, hipMemsetAsync(areas, 0, (size_t)n * sizeof(int), ctx->stream));
    hipLaunchKernelGGL(k_mesh_ccl_init, dim3(g), dim3(256), 0, ctx->stream, data, mask, (long)T, (long)C, labels);
    hipLaunchKernelGGL(k_mesh_ccl_merge, dim3(g), dim3(256), 0, ctx->stream, nbr, (long)T, (long)C, labels);
    hipLaunchKernelGGL(k_ccl_compress, dim3(g), dim3(256), 0, ctx->stream, n, labels);
    if (int rc = ensure_scratch(ctx, (size_t)n * sizeof(int))) return rc;
    int* parent = reinterpret_cast<int*>(ctx->morph_scratch);
    HIP_TRY(ctx, hipMemcpyAsync(parent, labels, (size_t)n * sizeof(int), hipMemcpyDeviceToDevice, ctx->stream));
    hipLaunchKernelGGL(k_ccl_flatten, dim3(g), dim3(256), 0, ctx->stream, n, parent, labels, areas);
    HIP_TRY(ctx, hipGetLastError());
    return 0;
}

// ------------------------------------------------------------------------------------------------
// Ordered stream compaction of the positive entries of an int32 array: the per-object areas that marex_label2d_i32 /
// marex_label_mesh_i32 leave at the root cells, as a list in index order (time, then first cell) -- what the blocked
// pre-processing appends to its per-object list instead of torch's `a[a > 0]` (4 bytes per cell of temporaries).
// Three launches and no workgroup waits on another: counts per tile of CCL_TILE consecutive entries (ballot + popcount
// per wave, the four wave counts through LDS), the exclusive scan of the tile counts by k_ccl_scan_tiles, and a scatter
// that ranks the entries of its tile the same way again.  v is read twice; the pass is bandwidth-bound.
// ------------------------------------------------------------------------------------------------
__global__ void __launch_bounds__(256)
k_compact_count(const int* __restrict__ v, long n, int* __restrict__ tile_cnt) {
    __shared__ int wcnt[4];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const long tile0 = (long)blockIdx.x * CCL_TILE;
    int mine = 0;
    for (int k = 0; k < CCL_TILE / 256; ++k) {
        const long i = tile0 + k * 256 + threadIdx.x;
        mine += (i < n && v[i] > 0) ? 1 : 0;
    }
    for (int d = 32; d > 0; d >>= 1) mine += __shfl_down(mine, d, 64);
    if (lane == 0) wcnt[wave] = mine;
    __syncthreads();
    if (threadIdx.x == 0) tile_cnt[blockIdx.x] = wcnt[0] + wcnt[1] + wcnt[2] + wcnt[3];
}

// out[rank] = v[i] for the positive entries with rank < cap; the entry of rank 0 reports its index, and the first
// thread of the grid the total (and -1 as the first index when there is none): every result has exactly one writer.
__global__ void __launch_bounds__(256)
k_compact_scatter(const int* __restrict__ v, long n, const int* __restrict__ tile_off, const int* __restrict__ total,
                  int* __restrict__ out, long cap, long long* __restrict__ n_out, long long* __restrict__ first_index) {
    __shared__ int wcnt[4];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const long tile0 = (long)blockIdx.x * CCL_TILE;
    if (blockIdx.x == 0 && threadIdx.x == 0) {
        const int tot = *total;
        *n_out = tot;
        if (tot == 0) *first_index = -1;
    }
    int run = tile_off[blockIdx.x];
    for (int k = 0; k < CCL_TILE / 256; ++k) {
        const long i = tile0 + k * 256 + threadIdx.x;
        const int val = i < n ? v[i] : 0;
        const bool keep = val > 0;
        const unsigned long long b = __ballot(keep);
        if (lane == 0) wcnt[wave] = __popcll(b);
        __syncthreads();
        if (keep) {
            long r = run + __popcll(b & ((1ull << lane) - 1ull));
            for (int w = 0; w < wave; ++w) r += wcnt[w];
            if (r < cap) out[r] = val;
            if (r == 0) *first_index = i;
        }
        run += wcnt[0] + wcnt[1] + wcnt[2] + wcnt[3];
        __syncthreads();
    }
}

extern "C" int marex_compact_positive_i32(marex_ctx* ctx, const int32_t* v, int64_t n, int32_t* out, int64_t cap,
                                          int64_t* n_out, int64_t* first_index) {
    if (!ctx) return -1;
    if (!v || !out || !n_out || !first_index || n <= 0 || cap < 0) return fail(ctx, -1, "marex_compact_positive_i32: null pointer, empty array or negative capacity");
    if (n > 2147483646L) return fail(ctx, -4, "marex_compact_positive_i32: more than 2^31 - 2 entries");
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    LaunchTimer lt(ctx, MAREX_K_MORPH);
    const long ntiles = (n + CCL_TILE - 1) / CCL_TILE;
    // scratch: tile counts and tile offsets [ntiles] each, the total
    if (int rc = ensure_scratch(ctx, (size_t)(2 * ntiles + 1) * sizeof(int))) return rc;
    int* tile_cnt = reinterpret_cast<int*>(ctx->morph_scratch);
    int* tile_off = tile_cnt + ntiles;
    int* total = tile_off + ntiles;
    hipLaunchKernelGGL(k_compact_count, dim3((unsigned)ntiles), dim3(256), 0, ctx->stream, v, (long)n, tile_cnt);
    hipLaunchKernelGGL(k_ccl_scan_tiles, dim3(1), dim3(1024), 0, ctx->stream, tile_cnt, ntiles, tile_off, total);
    hipLaunchKernelGGL(k_compact_scatter, dim3((unsigned)ntiles), dim3(256), 0, ctx->stream, v, (long)n, tile_off, total, out,
                       (long)cap, reinterpret_cast<long long*>(n_out), reinterpret_cast<long long*>(first_index));
    HIP_TRY(ctx, hipGetLastError());
    int count = 0;  // the caller sizes its list by the count: the one host read of this call
    HIP_TRY(ctx, hipMemcpyAsync(&count, total, sizeof(int), hipMemcpyDeviceToHost, ctx->stream));
    HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
    if ((int64_t)count > cap)
        return fail(ctx, -7, "marex_compact_positive_i32: %d positive entries, capacity %lld (the first %lld written)", count,
                    (long long)cap, (long long)cap);
    return 0;
}
