// marex_objects.hip -- object properties and time overlaps of an int32 ID field (the data stages under the reference's
// merge tracker, marEx/track.py:2109-2504, gridded branch): per (timestep, ID) the cell count and the integer moments
// behind regionprops' centroid plus the seam correction of calculate_centroid, and the cell counts of every
// (ID at t, ID at t + 1) pair.
//
// Every sum is an integer, accumulated with 64-bit integer atomics, so the results do not depend on the order in which
// waves arrive.  A wave walks OBJ_ITERS consecutive 64-cell pieces of every OBJ_TSTRIDE-th slice and keeps a running
// group (equal IDs, or equal pairs) in uniform registers: it reaches memory only when the ID changes, so the interior
// of a large object costs one atomic set per wave chunk instead of one per cell (per wave, across slices, where the
// destination does not depend on the slice).
#include "marex_common.hip.h"

#define OBJ_ITERS 16                     // 64-cell pieces per wave
#define OBJ_CHUNK (256 * OBJ_ITERS)      // cells of a slice per workgroup (4 waves)
#define OBJ_TILE 4096                    // IDs per tile of the span scan (16 per thread)
#define OBJ_MOM 5                        // u64 per slot: count, sum y, sum x, cells with x > nx / 2, near-edge flags

__device__ __forceinline__ int obj_wave_max_i32(int m) { return ~wave_min_i32(~m); }  // ~ reverses the order, never overflows

__global__ void __launch_bounds__(256) k_obj_fill_i32(int* __restrict__ p, long n, int v) {
    for (long i = (long)blockIdx.x * 256 + threadIdx.x; i < n; i += (long)gridDim.x * 256) p[i] = v;
}

// mm[0] = min, mm[1] = max over the field (mm initialised to INT_MAX, INT_MIN)
__global__ void __launch_bounds__(256) k_obj_minmax(const int* __restrict__ ids, long n, int* __restrict__ mm) {
    int lo = 2147483647, hi = -2147483647 - 1;
    for (long i = (long)blockIdx.x * 256 + threadIdx.x; i < n; i += (long)gridDim.x * 256) {
        const int v = ids[i];
        lo = v < lo ? v : lo;
        hi = v > hi ? v : hi;
    }
    lo = wave_min_i32(lo);
    hi = obj_wave_max_i32(hi);
    if ((threadIdx.x & 63) == 0) {
        atomicMin(&mm[0], lo);
        atomicMax(&mm[1], hi);
    }
}

// The cells of wave `wave` of workgroup (bx, .) in a slice of C cells: r = bx * OBJ_CHUNK + wave * 64 * OBJ_ITERS + 64 k
// + lane, k < OBJ_ITERS; cells at r >= C read as background.
__device__ __forceinline__ long obj_piece0(int wave) { return (long)blockIdx.x * OBJ_CHUNK + (long)wave * (64 * OBJ_ITERS); }

// tmin[id] / tmax[id]: first and last timestep ID id occurs in (initialised to INT_MAX / -1)
__global__ void __launch_bounds__(256)
k_obj_spans(const int* __restrict__ ids, long T, long C, int* __restrict__ tmin, int* __restrict__ tmax) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const long r0 = obj_piece0(wave);
    // the run (cur, first, last) lives across the slices the wave visits (t only grows), so an ID that fills the wave's
    // cells in slice after slice is sent once; min / max are idempotent, so an ID met again later is simply sent again
    int cur = 0, first = 0, last = 0;
    auto flush = [&]() {
        if (cur > 0 && lane == 0) {
            atomicMin(&tmin[cur], first);
            atomicMax(&tmax[cur], last);
        }
    };
    for (long t = blockIdx.y; t < T; t += gridDim.y) {
        const int* row = ids + t * C;
        int v[OBJ_ITERS];
#pragma unroll
        for (int k = 0; k < OBJ_ITERS; ++k) {
            const long r = r0 + 64 * k + lane;
            v[k] = r < C ? row[r] : 0;
        }
#pragma unroll
        for (int k = 0; k < OBJ_ITERS; ++k) {
            const int id = v[k] > 0 ? v[k] : 0;
            u64 todo = __ballot(id > 0);
            while (todo) {
                const int lead = __ffsll((long long)todo) - 1;
                const int il = __shfl(id, lead, 64);
                todo &= ~__ballot(id == il);
                if (il != cur) {
                    flush();
                    cur = il;
                    first = (int)t;
                }
                last = (int)t;
            }
        }
    }
    flush();
}

__device__ __forceinline__ long long obj_span(const int* tmin, const int* tmax, long id) {
    const int a = tmin[id], b = tmax[id];
    return b >= a ? (long long)b - a + 1 : 0;
}

// block sum of a per-thread int64 (256 threads), returned to every thread
__device__ __forceinline__ long long obj_block_sum_i64(long long s) {
    __shared__ long long part[4];
    s = wave_sum(s);
    if ((threadIdx.x & 63) == 0) part[threadIdx.x >> 6] = s;
    __syncthreads();
    const long long tot = part[0] + part[1] + part[2] + part[3];
    __syncthreads();
    return tot;
}

// tile_sum[b] = sum of the spans of IDs b * OBJ_TILE .. + OBJ_TILE
__global__ void __launch_bounds__(256)
k_obj_span_tiles(const int* __restrict__ tmin, const int* __restrict__ tmax, long nid, long long* __restrict__ tile_sum) {
    long long s = 0;
    for (int j = threadIdx.x; j < OBJ_TILE; j += 256) {
        const long id = (long)blockIdx.x * OBJ_TILE + j;
        if (id < nid) s += obj_span(tmin, tmax, id);
    }
    s = obj_block_sum_i64(s);
    if (threadIdx.x == 0) tile_sum[blockIdx.x] = s;
}

// exclusive scan of the tile sums by one workgroup (at most 2^31 / OBJ_TILE = 524288 tiles); *total = the sum
__global__ void __launch_bounds__(1024)
k_obj_scan_tiles(const long long* __restrict__ cnt, long ntiles, long long* __restrict__ off, long long* __restrict__ total) {
    __shared__ long long part[1024];
    const long per = (ntiles + 1023) / 1024;
    const long a = threadIdx.x * per, b = a + per < ntiles ? a + per : ntiles;
    long long s = 0;
    for (long j = a; j < b; ++j) s += cnt[j];
    part[threadIdx.x] = s;
    __syncthreads();
    for (int d = 1; d < 1024; d <<= 1) {
        const long long v = threadIdx.x >= (unsigned)d ? part[threadIdx.x - d] : 0;
        __syncthreads();
        part[threadIdx.x] += v;
        __syncthreads();
    }
    long long run = part[threadIdx.x] - s;
    for (long j = a; j < b; ++j) {
        const long long c = cnt[j];
        off[j] = run;
        run += c;
    }
    if (threadIdx.x == 1023) *total = part[1023];
}

// off[id] = exclusive prefix sum of the spans in ID order: thread j of tile b owns IDs b * OBJ_TILE + 16 j .. + 16
__global__ void __launch_bounds__(256)
k_obj_span_offsets(const int* __restrict__ tmin, const int* __restrict__ tmax, long nid, const long long* __restrict__ tile_off,
                   long long* __restrict__ off) {
    __shared__ long long part[256];
    const long id0 = (long)blockIdx.x * OBJ_TILE + 16L * threadIdx.x;
    long long s = 0;
    for (int j = 0; j < 16; ++j)
        if (id0 + j < nid) s += obj_span(tmin, tmax, id0 + j);
    part[threadIdx.x] = s;
    __syncthreads();
    for (int d = 1; d < 256; d <<= 1) {
        const long long v = threadIdx.x >= (unsigned)d ? part[threadIdx.x - d] : 0;
        __syncthreads();
        part[threadIdx.x] += v;
        __syncthreads();
    }
    long long run = tile_off[blockIdx.x] + part[threadIdx.x] - s;
    for (int j = 0; j < 16; ++j) {
        if (id0 + j >= nid) break;
        off[id0 + j] = run;
        run += obj_span(tmin, tmax, id0 + j);
    }
}

// Moments of every (t, id) slot, slot = off[id] + t - tmin[id]: acc[slot][0..4] += count, sum y, sum x, cells with
// x > nx / 2, flags (1: a cell with x < 100, 2: a cell with x >= nx - 100).  Inside one 64-cell piece lane l is cell
// r0 + l, so for a group of equal IDs  sum y = n y0 + sum dy  and  sum x = n x0 + sum l - nx sum dy  (y0, x0: the
// coordinates of r0, dy = y - y0 <= 64): one packed 32-bit wave sum of (l | dy << 16) per group.
__global__ void __launch_bounds__(256)
k_obj_moments(const int* __restrict__ ids, long T, int ny, int nx, const int* __restrict__ tmin, const long long* __restrict__ off,
              u64* __restrict__ acc) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const long C = (long)ny * nx;
    const long rw = obj_piece0(wave);
    const int half = nx / 2, right0 = nx - 100;
    for (long t = blockIdx.y; t < T; t += gridDim.y) {
        const int* row = ids + t * C;
        int v[OBJ_ITERS];
#pragma unroll
        for (int k = 0; k < OBJ_ITERS; ++k) {
            const long r = rw + 64 * k + lane;
            v[k] = r < C ? row[r] : 0;
        }
        int cur = 0;
        long long n = 0, sy = 0, sx = 0, nr = 0;
        unsigned fl = 0;
        auto flush = [&]() {
            if (cur > 0 && lane == 0) {
                u64* p = acc + (size_t)(off[cur] + (t - tmin[cur])) * OBJ_MOM;
                atomicAdd(p + 0, (u64)n);
                atomicAdd(p + 1, (u64)sy);
                atomicAdd(p + 2, (u64)sx);
                atomicAdd(p + 3, (u64)nr);
                atomicOr(p + 4, (u64)fl);
            }
        };
#pragma unroll  // v[k] must stay in registers: no dynamic indexing
        for (int k = 0; k < OBJ_ITERS; ++k) {
            const long r0 = rw + 64 * k;
            if (r0 >= C) break;  // wave-uniform
            const int id = v[k] > 0 ? v[k] : 0;
            u64 todo = __ballot(id > 0);
            if (!todo) continue;
            const unsigned ur0 = (unsigned)r0, ur = ur0 + lane, unx = (unsigned)nx;  // r0 + 63 < C + 64 < 2^32
            const long y0 = ur0 / unx, x0 = ur0 - (unsigned)y0 * unx;
            const unsigned y = ur / unx;
            const int x = (int)(ur - y * unx);
            const unsigned packed = (unsigned)lane | ((y - (unsigned)y0) << 16);
            const u64 b_right = __ballot(id > 0 && x > half);
            const u64 b_left_band = __ballot(id > 0 && x < 100);
            const u64 b_right_band = __ballot(id > 0 && x >= right0);
            while (todo) {
                const int lead = __ffsll((long long)todo) - 1;
                const int il = __shfl(id, lead, 64);
                const u64 same = __ballot(id == il) & todo;
                todo &= ~same;
                const unsigned s = wave_sum(((same >> lane) & 1ull) ? packed : 0u);
                const long long c = __popcll(same), sl = s & 0xFFFFu, sdy = s >> 16;
                if (il != cur) {
                    flush();
                    cur = il;
                    n = sy = sx = nr = 0;
                    fl = 0;
                }
                n += c;
                sy += c * y0 + sdy;
                sx += c * x0 + sl - (long long)nx * sdy;
                nr += __popcll(same & b_right);
                fl |= ((same & b_left_band) ? 1u : 0u) | ((same & b_right_band) ? 2u : 0u);
            }
        }
        flush();
    }
}

// Compaction of the non-empty slots (count > 0), in no particular order (the host sorts them): out_tid[2 p] = t,
// out_tid[2 p + 1] = id, out_mom[5 p ..] = the slot's moments.  The slot's ID is the last one whose offset is <= the
// slot (IDs with empty spans repeat the offset of the next ID, so the last one is the owner).
__global__ void __launch_bounds__(256)
k_obj_compact(long n_slots, long nid, const int* __restrict__ tmin, const long long* __restrict__ off, const u64* __restrict__ acc,
              u64* __restrict__ n_out, int* __restrict__ out_tid, u64* __restrict__ out_mom) {
    for (long j = (long)blockIdx.x * 256 + threadIdx.x; j < n_slots; j += (long)gridDim.x * 256) {
        const u64* a = acc + (size_t)j * OBJ_MOM;
        if (a[0] == 0) continue;
        long lo = 0, hi = nid - 1;  // largest id with off[id] <= j
        while (lo < hi) {
            const long mid = lo + (hi - lo + 1) / 2;
            if (off[mid] <= j) lo = mid; else hi = mid - 1;
        }
        const u64 p = atomicAdd(n_out, 1ull);
        out_tid[2 * p] = (int)(tmin[lo] + (j - off[lo]));
        out_tid[2 * p + 1] = (int)lo;
        for (int q = 0; q < OBJ_MOM; ++q) out_mom[OBJ_MOM * p + q] = a[q];
    }
}

// Overlap pairs of slices t and t + 1 (t < T - 1): key = a << 32 | b for every cell with a = ids[t] > 0 and
// b = ids[t + 1] > 0.  A wave folds equal keys of consecutive cells into one run; each run is one insert.
// INSERT = false: stats[0] += overlapping cells, stats[1] += runs (an upper bound of the distinct keys: the table size).
// INSERT = true: each run adds its cells to the key's entry of an open-addressing table (linear probing, CAS on the
// key, 0 = empty); stats[2] is set when a probe sequence found no free entry.
template <bool INSERT>
__global__ void __launch_bounds__(256)
k_ovl_pass(const int* __restrict__ ids, long T, long C, long cap, u64* __restrict__ keys, u64* __restrict__ cnts,
           u64* __restrict__ stats) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const long rw = obj_piece0(wave);
    u64 cells = 0, runs = 0;
    u64 cur = 0, cc = 0;  // the run lives across the slices the wave visits: a pair that persists is inserted once
    auto flush = [&]() {
        if (!cur) return;
        ++runs;
        if (INSERT && lane == 0) {
            const u64 mask = (u64)cap - 1;
            u64 h = splitmix64(cur) & mask;
            for (long p = 0; p < cap; ++p) {
                const u64 prev = atomicCAS(&keys[h], 0ull, cur);
                if (prev == 0ull || prev == cur) {
                    atomicAdd(&cnts[h], cc);
                    return;
                }
                h = (h + 1) & mask;
            }
            atomicOr(&stats[2], 1ull);
        }
    };
    for (long t = blockIdx.y; t + 1 < T; t += gridDim.y) {
        const int* ra = ids + t * C;
        const int* rb = ra + C;
        int va[OBJ_ITERS], vb[OBJ_ITERS];
#pragma unroll
        for (int k = 0; k < OBJ_ITERS; ++k) {
            const long r = rw + 64 * k + lane;
            va[k] = r < C ? ra[r] : 0;
            vb[k] = r < C ? rb[r] : 0;
        }
#pragma unroll  // v[k] must stay in registers: no dynamic indexing
        for (int k = 0; k < OBJ_ITERS; ++k) {
            const u64 key = (va[k] > 0 && vb[k] > 0) ? ((u64)(unsigned)va[k] << 32) | (unsigned)vb[k] : 0ull;
            u64 todo = __ballot(key != 0);
            cells += __popcll(todo);
            while (todo) {
                const int lead = __ffsll((long long)todo) - 1;
                const u64 kl = wave_shfl_u64(key, lead);
                const u64 same = __ballot(key == kl) & todo;
                todo &= ~same;
                if (kl != cur) {
                    flush();
                    cur = kl;
                    cc = 0;
                }
                cc += __popcll(same);
            }
        }
    }
    flush();
    if (!INSERT) {  // one pair of atomics per workgroup on the two shared counters
        __shared__ u64 part[2][4];
        if (lane == 0) {
            part[0][wave] = cells;
            part[1][wave] = runs;
        }
        __syncthreads();
        if (threadIdx.x == 0) {
            const u64 c = part[0][0] + part[0][1] + part[0][2] + part[0][3], n = part[1][0] + part[1][1] + part[1][2] + part[1][3];
            if (c) atomicAdd(&stats[0], c);
            if (n) atomicAdd(&stats[1], n);
        }
    }
}

// occupied table entries -> out_keys / out_counts (no particular order; the host sorts by key); stats[3] = how many
__global__ void __launch_bounds__(256)
k_ovl_compact(long cap, const u64* __restrict__ keys, const u64* __restrict__ cnts, long out_cap, u64* __restrict__ stats,
              u64* __restrict__ out_keys, u64* __restrict__ out_counts) {
    for (long h = (long)blockIdx.x * 256 + threadIdx.x; h < cap; h += (long)gridDim.x * 256) {
        const u64 k = keys[h];
        if (!k) continue;
        const u64 p = atomicAdd(&stats[3], 1ull);
        if (p < (u64)out_cap) {
            out_keys[p] = k;
            out_counts[p] = cnts[h];
        }
    }
}

// (pieces of a slice) x (up to OBJ_TSTRIDE slices; a workgroup walks every OBJ_TSTRIDE-th slice): few enough
// workgroups that the runs carried across slices and the per-workgroup counters keep same-address atomics rare, and
// OBJ_TSTRIDE slices in flight at once spread what remains over as many addresses
#define OBJ_TSTRIDE 64
static inline dim3 obj_slice_grid(long T, long C) {
    return slice_grid(T, C, OBJ_CHUNK, OBJ_TSTRIDE);
}

extern "C" int marex_ids_minmax_i32(marex_ctx* ctx, const int32_t* ids, int64_t n, int32_t* minmax) {
    if (!ctx) return -1;
    if (!ids || !minmax || n <= 0) return fail(ctx, -1, "marex_ids_minmax_i32: null pointer or empty field");
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    LaunchTimer lt(ctx, MAREX_K_MORPH);
    hipLaunchKernelGGL(k_obj_fill_i32, dim3(1), dim3(256), 0, ctx->stream, minmax, 1L, 2147483647);
    hipLaunchKernelGGL(k_obj_fill_i32, dim3(1), dim3(256), 0, ctx->stream, minmax + 1, 1L, -2147483647 - 1);
    hipLaunchKernelGGL(k_obj_minmax, dim3(stride_grid(n)), dim3(256), 0, ctx->stream, ids, (long)n, minmax);
    HIP_TRY(ctx, hipGetLastError());
    return 0;
}

extern "C" int marex_object_spans_i32(marex_ctx* ctx, const int32_t* ids, int64_t T, int64_t C, int max_id, int32_t* tmin,
                                      int32_t* tmax, int64_t* off, int64_t* work, int64_t* total) {
    if (!ctx) return -1;
    if (!ids || !tmin || !tmax || !off || !work || !total || T <= 0 || C <= 0 || max_id < 0)
        return fail(ctx, -1, "marex_object_spans_i32: null pointer, empty shape or negative max_id");
    if (C >= 2147483647L || T >= 2147483647L) return fail(ctx, -4, "marex_object_spans_i32: a slice or the time axis has 2^31 - 1 or more entries");
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    LaunchTimer lt(ctx, MAREX_K_MORPH);
    const long nid = (long)max_id + 1, ntiles = (nid + OBJ_TILE - 1) / OBJ_TILE;
    long long* tile_sum = reinterpret_cast<long long*>(work);
    long long* tile_off = tile_sum + ntiles;
    hipLaunchKernelGGL(k_obj_fill_i32, dim3(stride_grid(nid)), dim3(256), 0, ctx->stream, tmin, nid, 2147483647);
    hipLaunchKernelGGL(k_obj_fill_i32, dim3(stride_grid(nid)), dim3(256), 0, ctx->stream, tmax, nid, -1);
    hipLaunchKernelGGL(k_obj_spans, obj_slice_grid(T, C), dim3(256), 0, ctx->stream, ids, (long)T, (long)C, tmin, tmax);
    hipLaunchKernelGGL(k_obj_span_tiles, dim3((unsigned)ntiles), dim3(256), 0, ctx->stream, tmin, tmax, nid, tile_sum);
    hipLaunchKernelGGL(k_obj_scan_tiles, dim3(1), dim3(1024), 0, ctx->stream, tile_sum, ntiles, tile_off, (long long*)total);
    hipLaunchKernelGGL(k_obj_span_offsets, dim3((unsigned)ntiles), dim3(256), 0, ctx->stream, tmin, tmax, nid, tile_off,
                       (long long*)off);
    HIP_TRY(ctx, hipGetLastError());
    return 0;
}

extern "C" int marex_object_moments_i32(marex_ctx* ctx, const int32_t* ids, int64_t T, int ny, int nx, const int32_t* tmin,
                                        const int64_t* off, int64_t n_slots, uint64_t* acc) {
    if (!ctx) return -1;
    if (!ids || !tmin || !off || !acc || T <= 0 || ny <= 0 || nx <= 0 || n_slots <= 0)
        return fail(ctx, -1, "marex_object_moments_i32: null pointer or empty shape");
    const long C = (long)ny * nx;
    if (C >= 2147483647L || T >= 2147483647L) return fail(ctx, -4, "marex_object_moments_i32: a slice or the time axis has 2^31 - 1 or more entries");
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    LaunchTimer lt(ctx, MAREX_K_MORPH);
    HIP_TRY(ctx, hipMemsetAsync(acc, 0, (size_t)n_slots * OBJ_MOM * sizeof(u64), ctx->stream));
    hipLaunchKernelGGL(k_obj_moments, obj_slice_grid(T, C), dim3(256), 0, ctx->stream, ids, (long)T, ny, nx, tmin,
                       (const long long*)off, (u64*)acc);
    HIP_TRY(ctx, hipGetLastError());
    return 0;
}

extern "C" int marex_object_compact(marex_ctx* ctx, int64_t n_slots, int max_id, const int32_t* tmin, const int64_t* off,
                                    const uint64_t* acc, uint64_t* n_out, int32_t* out_tid, uint64_t* out_mom) {
    if (!ctx) return -1;
    if (!tmin || !off || !acc || !n_out || !out_tid || !out_mom || n_slots <= 0 || max_id < 0)
        return fail(ctx, -1, "marex_object_compact: null pointer or empty slot list");
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    LaunchTimer lt(ctx, MAREX_K_MORPH);
    HIP_TRY(ctx, hipMemsetAsync(n_out, 0, sizeof(u64), ctx->stream));
    hipLaunchKernelGGL(k_obj_compact, dim3(stride_grid(n_slots)), dim3(256), 0, ctx->stream, (long)n_slots, (long)max_id + 1,
                       tmin, (const long long*)off, (const u64*)acc, (u64*)n_out, out_tid, (u64*)out_mom);
    HIP_TRY(ctx, hipGetLastError());
    return 0;
}

extern "C" int marex_overlap_count_i32(marex_ctx* ctx, const int32_t* ids, int64_t T, int64_t C, uint64_t* stats) {
    if (!ctx) return -1;
    if (!ids || !stats || T <= 0 || C <= 0) return fail(ctx, -1, "marex_overlap_count_i32: null pointer or empty shape");
    if (C >= 2147483647L || T >= 2147483647L) return fail(ctx, -4, "marex_overlap_count_i32: a slice or the time axis has 2^31 - 1 or more entries");
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    LaunchTimer lt(ctx, MAREX_K_MORPH);
    HIP_TRY(ctx, hipMemsetAsync(stats, 0, 4 * sizeof(u64), ctx->stream));
    if (T > 1)
        hipLaunchKernelGGL(k_ovl_pass<false>, obj_slice_grid(T - 1, C), dim3(256), 0, ctx->stream, ids, (long)T, (long)C, 0L,
                           (u64*)nullptr, (u64*)nullptr, (u64*)stats);
    HIP_TRY(ctx, hipGetLastError());
    return 0;
}

extern "C" int marex_overlap_pairs_i32(marex_ctx* ctx, const int32_t* ids, int64_t T, int64_t C, int64_t cap, uint64_t* keys,
                                       uint64_t* counts, uint64_t* stats, int64_t out_cap, uint64_t* out_keys,
                                       uint64_t* out_counts) {
    if (!ctx) return -1;
    if (!ids || !keys || !counts || !stats || !out_keys || !out_counts || T < 2 || C <= 0 || out_cap <= 0)
        return fail(ctx, -1, "marex_overlap_pairs_i32: null pointer, fewer than two slices or no room for pairs");
    if (cap < 64 || (cap & (cap - 1))) return fail(ctx, -1, "marex_overlap_pairs_i32: cap=%lld is not a power of two >= 64", (long long)cap);
    if (C >= 2147483647L || T >= 2147483647L) return fail(ctx, -4, "marex_overlap_pairs_i32: a slice or the time axis has 2^31 - 1 or more entries");
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    LaunchTimer lt(ctx, MAREX_K_MORPH);
    HIP_TRY(ctx, hipMemsetAsync(keys, 0, (size_t)cap * sizeof(u64), ctx->stream));
    HIP_TRY(ctx, hipMemsetAsync(counts, 0, (size_t)cap * sizeof(u64), ctx->stream));
    HIP_TRY(ctx, hipMemsetAsync(stats + 2, 0, 2 * sizeof(u64), ctx->stream));
    hipLaunchKernelGGL(k_ovl_pass<true>, obj_slice_grid(T - 1, C), dim3(256), 0, ctx->stream, ids, (long)T, (long)C, (long)cap,
                       (u64*)keys, (u64*)counts, (u64*)stats);
    hipLaunchKernelGGL(k_ovl_compact, dim3(stride_grid(cap)), dim3(256), 0, ctx->stream, (long)cap, (const u64*)keys,
                       (const u64*)counts, (long)out_cap, (u64*)stats, (u64*)out_keys, (u64*)out_counts);
    HIP_TRY(ctx, hipGetLastError());
    return 0;
}
