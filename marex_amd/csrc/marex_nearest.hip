// marex_nearest.hip -- nearest-cell resampling between any two geometries on the sphere: the exact nearest source cell of
// every target (once per pair of geometries) and the gather of a [time, cells] field through that index.
//
// Arithmetic contract.  The host hands over float64 unit vectors, [3][N] of the eligible source
// cells (with their original cell numbers ids [N]) and [3][M] of the targets; the device calls no transcendental.  The
// squared chord of source i and target j is q = (dx * dx + dy * dy) + dz * dz with dx = xs - xt etc., every operation
// rounded on its own (-ffp-contract=off), and the answer is the pair (q, id) that is smallest in the order "q first, then
// the cell number".  That is a total order, so neither the search structure, nor the order inside a voxel, nor the lane
// or wave that met a candidate can show in the result.  A target with a NaN coordinate compares false everywhere: it
// keeps index -1 and q = +inf.
//
// k_nearest_brute: a lane owns a target, the sources stream through LDS in tiles of NB_TILE; every lane of a wave reads
// the same LDS address (a broadcast), so the loop is float64 VALU work: 3 subtractions, 3 products, 2 sums, 2 compares.
// With a list sel [K] it runs over those K targets only (the fallback of the bucketed search).
//
// The bucketed search: the sources are binned into n^3 voxels of edge h = 2 / n over [-1, 1]^3 (k_voxel_count, a prefix
// sum by the caller, k_voxel_scatter, which writes vectors and cell numbers in voxel order; the order inside a voxel is
// whatever the atomics made it).  A voxel's number is (vz * n + vy) * n + vx, so a run of voxels along x is one contiguous
// range of the sorted table.  k_nearest_voxel: a lane owns a target and searches the Chebyshev rings r = 0, 1, 2 ... of
// voxels around its own, clamped to the grid: every (vz, vy) row of the ring's cube is either a whole x-run (a face) or
// its two end voxels.
//
// The stopping rule and its margin.  voxel_of(p) = clamp(int((p + 1) * (n / 2)), 0, n - 1).  p + 1 carries a relative
// rounding of 2^-53 on a value of at most 2, the product another one on a value of at most n: the computed voxel
// coordinate is off by at most n * 2^-52 voxels, that is by eps = 2^-51 in p.  So a point counted in voxel v lies, in
// exact arithmetic, in [v h - 1 - eps, (v + 1) h - 1 + eps] on every axis (|p| <= 1: the clamp moves p = 1 only).  When
// ring r is finished, every source not yet seen sits at least r + 1 voxels away on some axis, so its true difference on
// that axis is at least r h - 2 eps.  Its computed q is at least the computed square of that one difference (the sums
// add non-negative terms, and rounding is monotonic), which is at least (r h - 2 eps)^2 (1 - 2^-51).  With n <= 1024,
// h >= 2^-9 and 2 eps / (r h) <= 2^-41, so q_unseen >= (r h)^2 (1 - 2^-39).  The lane stops after ring r >= 1 when
//     best_q < bound(r) = fl(fl(fl(r * h)^2) * (1 - 2^-32)),
// three roundings of 2^-53 each below the exact (r h)^2 (1 - 2^-32) -- still below (r h)^2 (1 - 2^-39): every unseen
// source then has a strictly larger q than the best one and cannot win, not even a tie.  The lane also stops when the
// rings cover the grid.  qmax (the squared chord of max_distance_km, widened by the host; +inf: none) lets a lane give up
// once bound(r) > qmax: whatever is still unseen, and whatever it holds that is not below bound(r), the host would
// discard anyway.  A lane still open after ring max_rings writes flag 1; the caller runs the brute kernel over those.
//
// k_resample_nearest: a lane owns V consecutive targets (4 for bytes where a row is a multiple of 4, else 1), reads
// their indices once and walks the rows of its slice RS_U at a time: the stores are coalesced along the targets, the
// loads are gathers whose neighbours mostly share or neighbour a source cell.  64-bit offsets throughout.
#include "marex_common.hip.h"

#define NB_TILE 1024  // source cells per LDS tile of the brute kernel: 28 KiB of vectors and cell numbers
#define NV_MAX_N 1024  // the largest voxel grid: the margin above is derived for n <= 1024
#define RS_U 8  // rows a lane of the gather has in flight

// (q, id) < (bq, bi) in the total order; a NaN q is never smaller
__device__ __forceinline__ void nearest_take(double q, int id, double& bq, int& bi) {
    if (q < bq || (q == bq && id < bi)) {
        bq = q;
        bi = id;
    }
}

__device__ __forceinline__ double chord2(double xs, double ys, double zs, double xt, double yt, double zt) {
    const double dx = xs - xt, dy = ys - yt, dz = zs - zt;
    return (dx * dx + dy * dy) + dz * dz;
}

__global__ void __launch_bounds__(256)
k_nearest_brute(const double* __restrict__ src, const int* __restrict__ ids, long N, const double* __restrict__ dst, long M,
                const int* __restrict__ sel, long K, int* __restrict__ index, double* __restrict__ qout) {
    __shared__ double sx[NB_TILE], sy[NB_TILE], sz[NB_TILE];
    __shared__ int sid[NB_TILE];
    const long k = (long)blockIdx.x * 256 + threadIdx.x;
    long j = -1;
    if (k < K) j = sel ? (long)sel[k] : k;
    const bool active = j >= 0 && j < M;  // an entry of sel outside 0 .. M - 1 addresses nothing
    const double nan_ = __longlong_as_double(0x7FF8000000000000LL);
    const double xt = active ? dst[j] : nan_, yt = active ? dst[M + j] : nan_, zt = active ? dst[2 * M + j] : nan_;
    double bq = __longlong_as_double(0x7FF0000000000000LL);
    int bi = -1;
    for (long base = 0; base < N; base += NB_TILE) {
        const int cnt = (int)(N - base < NB_TILE ? N - base : NB_TILE);
        __syncthreads();  // the tile before is read out
        for (int s = threadIdx.x; s < cnt; s += 256) {
            sx[s] = src[base + s];
            sy[s] = src[N + base + s];
            sz[s] = src[2 * N + base + s];
            sid[s] = ids ? ids[base + s] : (int)(base + s);
        }
        __syncthreads();
#pragma unroll 4
        for (int s = 0; s < cnt; ++s) nearest_take(chord2(sx[s], sy[s], sz[s], xt, yt, zt), sid[s], bq, bi);
    }
    if (active) {
        index[j] = bi;
        qout[j] = bq;
    }
}

// the voxel coordinate of p on one axis; the comparisons also send a NaN to voxel 0
__device__ __forceinline__ int voxel_of(double p, int n, double half_n) {
    const double u = (p + 1.0) * half_n;
    int v = u >= 0.0 ? (u < (double)n ? (int)u : n - 1) : 0;
    return v < 0 ? 0 : (v > n - 1 ? n - 1 : v);
}

__device__ __forceinline__ long voxel_id(const double* __restrict__ p, long N, long i, int n, double half_n) {
    const int vx = voxel_of(p[i], n, half_n), vy = voxel_of(p[N + i], n, half_n), vz = voxel_of(p[2 * N + i], n, half_n);
    return ((long)vz * n + vy) * n + vx;
}

// count [n^3] += the sources of every voxel
__global__ void __launch_bounds__(256)
k_voxel_count(const double* __restrict__ src, long N, int n, double half_n, int* __restrict__ count) {
    for (long i = (long)blockIdx.x * 256 + threadIdx.x; i < N; i += (long)gridDim.x * 256)
        atomicAdd(&count[voxel_id(src, N, i, n, half_n)], 1);
}

// off [n^3 + 1]: the exclusive prefix sum of the counts; cursor [n^3] starts as zeros.  Writes the vectors and the cell
// numbers in voxel order.
__global__ void __launch_bounds__(256)
k_voxel_scatter(const double* __restrict__ src, const int* __restrict__ ids, long N, int n, double half_n,
                const int* __restrict__ off, int* __restrict__ cursor, double* __restrict__ sorted, int* __restrict__ sorted_ids) {
    for (long i = (long)blockIdx.x * 256 + threadIdx.x; i < N; i += (long)gridDim.x * 256) {
        const long v = voxel_id(src, N, i, n, half_n);
        const long p = (long)off[v] + atomicAdd(&cursor[v], 1);
        if (p < 0 || p >= N) continue;  // an offset table that does not belong to these sources writes nothing out of range
        sorted[p] = src[i];
        sorted[N + p] = src[N + i];
        sorted[2 * N + p] = src[2 * N + i];
        sorted_ids[p] = ids ? ids[i] : (int)i;
    }
}

__global__ void __launch_bounds__(256)
k_nearest_voxel(const double* __restrict__ sorted, const int* __restrict__ sorted_ids, long N, const int* __restrict__ off, int n,
                double half_n, double h, const double* __restrict__ dst, long M, int max_rings, double qmax,
                int* __restrict__ index, double* __restrict__ qout, unsigned char* __restrict__ flag) {
    const long j = (long)blockIdx.x * 256 + threadIdx.x;
    if (j >= M) return;
    const double xt = dst[j], yt = dst[M + j], zt = dst[2 * M + j];
    double bq = __longlong_as_double(0x7FF0000000000000LL);
    int bi = -1;
    unsigned char open = 0;
    if (xt == xt && yt == yt && zt == zt) {
        const int cx = voxel_of(xt, n, half_n), cy = voxel_of(yt, n, half_n), cz = voxel_of(zt, n, half_n);
        // the ring that reaches the last voxel of the grid on every axis
        int rfull = cx > n - 1 - cx ? cx : n - 1 - cx;
        rfull = cy > rfull ? cy : rfull;
        rfull = n - 1 - cy > rfull ? n - 1 - cy : rfull;
        rfull = cz > rfull ? cz : rfull;
        rfull = n - 1 - cz > rfull ? n - 1 - cz : rfull;
        auto scan = [&](long a, long b) {
            a = a < 0 ? 0 : a;
            b = b > N ? N : b;  // a table that does not belong to these sources reads nothing out of range
            for (long s = a; s < b; ++s) nearest_take(chord2(sorted[s], sorted[N + s], sorted[2 * N + s], xt, yt, zt), sorted_ids[s], bq, bi);
        };
        open = 1;
        for (int r = 0; r <= max_rings; ++r) {
            const int z0 = cz - r < 0 ? 0 : cz - r, z1 = cz + r > n - 1 ? n - 1 : cz + r;
            const int y0 = cy - r < 0 ? 0 : cy - r, y1 = cy + r > n - 1 ? n - 1 : cy + r;
            const int x0 = cx - r < 0 ? 0 : cx - r, x1 = cx + r > n - 1 ? n - 1 : cx + r;
            for (int vz = z0; vz <= z1; ++vz) {
                const bool zface = vz == cz - r || vz == cz + r;
                for (int vy = y0; vy <= y1; ++vy) {
                    const long row = ((long)vz * n + vy) * n;
                    if (zface || vy == cy - r || vy == cy + r) {
                        scan(off[row + x0], off[row + x1 + 1]);
                    } else {
                        if (cx - r >= 0) scan(off[row + cx - r], off[row + cx - r + 1]);
                        if (cx + r <= n - 1) scan(off[row + cx + r], off[row + cx + r + 1]);  // r >= 1 here: another voxel
                    }
                }
            }
            if (r >= rfull) {  // every voxel is searched
                open = 0;
                break;
            }
            if (r >= 1) {
                const double rh = (double)r * h;
                const double bound = (rh * rh) * (1.0 - 0x1p-32);
                if (bq < bound || bound > qmax) {
                    open = 0;
                    break;
                }
            }
        }
    }
    index[j] = bi;
    qout[j] = bq;
    flag[j] = open;
}

template <typename T, int V>
struct gather_word;
template <typename T>
struct gather_word<T, 1> { typedef T type; };
template <>
struct gather_word<unsigned char, 4> { typedef unsigned type; };

// out [Tb][M] = x [Tb][C] gathered through index [M]; fill where index < 0.  An index of C or more reads nothing either.
template <typename T, int V>
__global__ void __launch_bounds__(256)
k_resample_nearest(const T* __restrict__ x, long Tb, long C, const int* __restrict__ index, long M, T fill, T* __restrict__ out) {
    typedef typename gather_word<T, V>::type W;
    const long lane = (long)blockIdx.x * 256 + threadIdx.x;
    const long j = lane * V;
    if (j >= M) return;  // V == 4 only where M is a multiple of 4: a lane's targets are all there
    int idx[V];
#pragma unroll
    for (int v = 0; v < V; ++v) {
        const int i = index[j + v];
        idx[v] = (i >= 0 && (long)i < C) ? i : -1;
    }
    for (long r = (long)blockIdx.y * RS_U; r < Tb; r += (long)gridDim.y * RS_U) {
        T val[RS_U][V];
#pragma unroll
        for (int k = 0; k < RS_U; ++k)
#pragma unroll
            for (int v = 0; v < V; ++v) val[k][v] = (r + k < Tb && idx[v] >= 0) ? x[(size_t)(r + k) * (size_t)C + idx[v]] : fill;
#pragma unroll
        for (int k = 0; k < RS_U; ++k) {
            if (r + k < Tb) {
                W w;
                if constexpr (V == 4)
                    w = (unsigned)val[k][0] | ((unsigned)val[k][1] << 8) | ((unsigned)val[k][2] << 16) | ((unsigned)val[k][3] << 24);
                else
                    w = val[k][0];
                *reinterpret_cast<W*>(out + (size_t)(r + k) * (size_t)M + j) = w;
            }
        }
    }
}

static int nearest_args(marex_ctx* ctx, const char* name, const void* src, int64_t N, const void* dst, int64_t M, const void* index,
                        const void* q) {
    if (!src || !dst || !index || !q || N <= 0 || M <= 0) return fail(ctx, -1, "%s: null pointer or empty shape", name);
    if (N >= 2147483647L || M >= 2147483647L) return fail(ctx, -4, "%s: 2^31 - 1 or more source or target cells", name);
    return 0;
}

static int voxel_args(marex_ctx* ctx, const char* name, int n) {
    if (n < 1 || n > NV_MAX_N) return fail(ctx, -1, "%s: the voxel grid must have 1 .. %d voxels per axis", name, NV_MAX_N);
    return 0;
}

extern "C" int marex_nearest_brute_f64(marex_ctx* ctx, const double* src, const int32_t* ids, int64_t N, const double* dst, int64_t M,
                                       const int32_t* sel, int64_t K, int32_t* index, double* q) {
    const char* name = "marex_nearest_brute_f64";
    if (!ctx) return -1;
    if (const int rc = nearest_args(ctx, name, src, N, dst, M, index, q)) return rc;
    if (sel ? (K <= 0 || K > M) : K != M) return fail(ctx, -1, "%s: K must be M without a list, 1 .. M with one", name);
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    LaunchTimer lt(ctx, MAREX_K_MORPH);
    hipLaunchKernelGGL(k_nearest_brute, dim3((unsigned)((K + 255) / 256)), dim3(256), 0, ctx->stream, src, (const int*)ids, (long)N, dst,
                       (long)M, (const int*)sel, (long)K, (int*)index, q);
    HIP_TRY(ctx, hipGetLastError());
    return 0;
}

extern "C" int marex_voxel_count_f64(marex_ctx* ctx, const double* src, int64_t N, int n, int32_t* count) {
    const char* name = "marex_voxel_count_f64";
    if (!ctx) return -1;
    if (!src || !count || N <= 0) return fail(ctx, -1, "%s: null pointer or empty shape", name);
    if (N >= 2147483647L) return fail(ctx, -4, "%s: 2^31 - 1 or more source cells", name);
    if (const int rc = voxel_args(ctx, name, n)) return rc;
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    LaunchTimer lt(ctx, MAREX_K_MORPH);
    hipLaunchKernelGGL(k_voxel_count, dim3(stride_grid(N)), dim3(256), 0, ctx->stream, src, (long)N, n, 0.5 * (double)n, (int*)count);
    HIP_TRY(ctx, hipGetLastError());
    return 0;
}

extern "C" int marex_voxel_scatter_f64(marex_ctx* ctx, const double* src, const int32_t* ids, int64_t N, int n, const int32_t* off,
                                       int32_t* cursor, double* sorted, int32_t* sorted_ids) {
    const char* name = "marex_voxel_scatter_f64";
    if (!ctx) return -1;
    if (!src || !off || !cursor || !sorted || !sorted_ids || N <= 0) return fail(ctx, -1, "%s: null pointer or empty shape", name);
    if (N >= 2147483647L) return fail(ctx, -4, "%s: 2^31 - 1 or more source cells", name);
    if (const int rc = voxel_args(ctx, name, n)) return rc;
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    LaunchTimer lt(ctx, MAREX_K_MORPH);
    hipLaunchKernelGGL(k_voxel_scatter, dim3(stride_grid(N)), dim3(256), 0, ctx->stream, src, (const int*)ids, (long)N, n,
                       0.5 * (double)n, (const int*)off, (int*)cursor, sorted, (int*)sorted_ids);
    HIP_TRY(ctx, hipGetLastError());
    return 0;
}

extern "C" int marex_nearest_voxel_f64(marex_ctx* ctx, const double* sorted, const int32_t* sorted_ids, int64_t N, const int32_t* off,
                                       int n, const double* dst, int64_t M, int max_rings, double qmax, int32_t* index, double* q,
                                       uint8_t* flag) {
    const char* name = "marex_nearest_voxel_f64";
    if (!ctx) return -1;
    if (const int rc = nearest_args(ctx, name, sorted, N, dst, M, index, q)) return rc;
    if (!sorted_ids || !off || !flag || max_rings < 0 || !(qmax >= 0.0))
        return fail(ctx, -1, "%s: null pointer, negative max_rings, or qmax negative or NaN", name);
    if (const int rc = voxel_args(ctx, name, n)) return rc;
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    LaunchTimer lt(ctx, MAREX_K_MORPH);
    hipLaunchKernelGGL(k_nearest_voxel, dim3((unsigned)((M + 255) / 256)), dim3(256), 0, ctx->stream, sorted, (const int*)sorted_ids,
                       (long)N, (const int*)off, n, 0.5 * (double)n, 2.0 / (double)n, dst, (long)M, max_rings, qmax, (int*)index, q,
                       (unsigned char*)flag);
    HIP_TRY(ctx, hipGetLastError());
    return 0;
}

template <typename T>
static int resample_launch(marex_ctx* ctx, const char* name, const T* x, int64_t Tb, int64_t C, const int32_t* index, int64_t M, T fill,
                           T* out) {
    if (!ctx) return -1;
    if (!x || !index || !out || Tb <= 0 || C <= 0 || M <= 0) return fail(ctx, -1, "%s: null pointer or empty shape", name);
    if (const int rc = cell_stream_limits(ctx, name, 0, Tb, C > M ? C : M)) return rc;
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    LaunchTimer lt(ctx, MAREX_K_MORPH);
    const long slices = (Tb + RS_U - 1) / RS_U;
    const unsigned gy = (unsigned)(slices < 64 ? slices : 64);
    if (sizeof(T) == 1 && M % 4 == 0 && ((uintptr_t)out & 3) == 0) {
        if constexpr (sizeof(T) == 1)
            hipLaunchKernelGGL((k_resample_nearest<T, 4>), dim3((unsigned)((M / 4 + 255) / 256), gy), dim3(256), 0, ctx->stream, x, (long)Tb,
                               (long)C, (const int*)index, (long)M, fill, out);
    } else {
        hipLaunchKernelGGL((k_resample_nearest<T, 1>), dim3((unsigned)((M + 255) / 256), gy), dim3(256), 0, ctx->stream, x, (long)Tb, (long)C,
                           (const int*)index, (long)M, fill, out);
    }
    HIP_TRY(ctx, hipGetLastError());
    return 0;
}

extern "C" int marex_resample_nearest_u8(marex_ctx* ctx, const uint8_t* x, int64_t Tb, int64_t C, const int32_t* index, int64_t M,
                                         int fill, uint8_t* out) {
    if (ctx && (fill < 0 || fill > 255)) return fail(ctx, -1, "marex_resample_nearest_u8: fill must be 0 .. 255");
    return resample_launch<unsigned char>(ctx, "marex_resample_nearest_u8", x, Tb, C, index, M, (unsigned char)fill, out);
}

extern "C" int marex_resample_nearest_i32(marex_ctx* ctx, const int32_t* x, int64_t Tb, int64_t C, const int32_t* index, int64_t M,
                                          int fill, int32_t* out) {
    return resample_launch<int>(ctx, "marex_resample_nearest_i32", x, Tb, C, index, M, fill, out);
}

extern "C" int marex_resample_nearest_f32(marex_ctx* ctx, const float* x, int64_t Tb, int64_t C, const int32_t* index, int64_t M,
                                          float fill, float* out) {
    return resample_launch<float>(ctx, "marex_resample_nearest_f32", x, Tb, C, index, M, fill, out);
}
