// marex_mesh_objects.hip -- the object stages of the tracker on an unstructured mesh (marEx/track.py:1947-2005,
// 2135-2323, 2431-2439, 1513-1514, 2762-2764): per-timestep IDs in the reference's order, and area-weighted object
// moments, time overlaps and total areas of a [T][C] field.
//
// The weights are fixed point: q int64 [4][C] holds the cell area and the area times the cell's unit vector (x, y, z),
// scaled by 2^e on the host so that the sum of any row over all cells stays below 2^62 (marex_amd/track_mesh.py,
// mesh_weight_tables).  The device only adds integers, with 64-bit integer atomics, so a result does not depend on the order
// in which waves arrive and is the same from run to run; the host turns the sums into float32 areas and centroids.
//
// The accumulating kernels keep the shape of marex_objects.hip: a wave walks MOBJ_ITERS consecutive 64-cell pieces of a
// slice, groups the lanes of a piece by equal ID (or pair) with __ballot, reduces each group over the wave and carries the
// group's sums in uniform registers until the ID changes -- the interior of a large object costs one set of atomics per
// wave chunk, not one per cell.  q is read only by lanes that hold an ID.
#include "marex_common.hip.h"

#define MOBJ_ITERS 16                     // 64-cell pieces per wave
#define MOBJ_CHUNK (256 * MOBJ_ITERS)     // cells of a slice per workgroup (4 waves)
#define MOBJ_MOM 5                        // u64 per slot: cells, sum q0 (area), sum q1, q2, q3 (area * x, y, z)
#define MOBJ_TSTRIDE 64                   // slices in flight: a workgroup walks every MOBJ_TSTRIDE-th slice
#define RANK_THREADS 1024
#define RANK_PIECES 8                     // 64-cell pieces per wave and iteration of the rank scan
#define RANK_CHUNK (RANK_THREADS * RANK_PIECES)

__device__ __forceinline__ long long mobj_wave_sum_i64(long long v) {
    for (int o = 32; o; o >>= 1) {
        const unsigned lo = __shfl_xor((unsigned)v, o, 64), hi = __shfl_xor((unsigned)((u64)v >> 32), o, 64);
        v += (long long)(((u64)hi << 32) | lo);
    }
    return v;
}

__device__ __forceinline__ long mobj_piece0(int wave) { return (long)blockIdx.x * MOBJ_CHUNK + (long)wave * (64 * MOBJ_ITERS); }

static inline dim3 mobj_slice_grid(long T, long C) {
    return slice_grid(T, C, MOBJ_CHUNK, MOBJ_TSTRIDE);
}

// ------------------------------------------------------------------------------------------------ per-timestep IDs
// One workgroup per slice: rank[t C + c] = 1 + the number of root cells of slice t below c, for every root cell c
// (labels[t C + c] == t C + c + 1); n_t[t] = the roots of the slice.  Wave w of the 16 owns cells base + 512 w .. + 512 of
// every RANK_CHUNK cells: 8 ballots, one exchange of the wave totals through LDS (double buffered: one barrier).
__global__ void __launch_bounds__(RANK_THREADS)
k_mesh_rank_roots(const int* labels, long C, int* __restrict__ rank, int* __restrict__ n_t) {
    __shared__ int wtot[2][RANK_THREADS / 64];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const long t = blockIdx.x, row = t * C;
    const u64 below = lane ? (~0ull >> (64 - lane)) : 0ull;
    int run = 0, par = 0;
    for (long base = 0; base < C; base += RANK_CHUNK, par ^= 1) {
        const long c0 = base + (long)wave * (64 * RANK_PIECES);
        u64 b[RANK_PIECES];
        int tot = 0;
#pragma unroll
        for (int j = 0; j < RANK_PIECES; ++j) {
            const long c = c0 + 64 * j + lane;
            const bool root = c < C && labels[row + c] == (int)(row + c + 1);
            b[j] = __ballot(root);
            tot += __popcll(b[j]);
        }
        if (lane == 0) wtot[par][wave] = tot;
        __syncthreads();
        int before = 0, all = 0;
#pragma unroll
        for (int w = 0; w < RANK_THREADS / 64; ++w) {
            const int v = wtot[par][w];
            before += w < wave ? v : 0;
            all += v;
        }
        int r = run + before;
#pragma unroll
        for (int j = 0; j < RANK_PIECES; ++j) {
            if ((b[j] >> lane) & 1ull) rank[row + c0 + 64 * j + lane] = r + __popcll(b[j] & below) + 1;
            r += __popcll(b[j]);
        }
        run += all;
    }
    if (threadIdx.x == 0) n_t[t] = run;
}

// ids[i] = the rank of the root of cell i (0 for background); labels and ids may be the same array
__global__ void __launch_bounds__(256) k_mesh_rank_gather(const int* labels, long n, const int* __restrict__ rank, int* ids) {
    for (long i = (long)blockIdx.x * 256 + threadIdx.x; i < n; i += (long)gridDim.x * 256) {
        const int l = labels[i];
        ids[i] = (l > 0 && (long)l <= n) ? rank[l - 1] : 0;
    }
}

extern "C" int marex_label_mesh_rank_i32(marex_ctx* ctx, const int32_t* labels, int64_t T, int64_t C, int32_t* rank,
                                         int32_t* ids, int32_t* n_t) {
    if (!ctx) return -1;
    if (!labels || !rank || !ids || !n_t || T <= 0 || C <= 0) return fail(ctx, -1, "marex_label_mesh_rank_i32: null pointer or empty shape");
    const long n = (long)T * C;
    if (n >= 2147483647L) return fail(ctx, -4, "marex_label_mesh_rank_i32: more than 2^31 - 1 cells; label the series in time blocks");
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    LaunchTimer lt(ctx, MAREX_K_MORPH);
    hipLaunchKernelGGL(k_mesh_rank_roots, dim3((unsigned)T), dim3(RANK_THREADS), 0, ctx->stream, labels, (long)C, rank, n_t);
    hipLaunchKernelGGL(k_mesh_rank_gather, dim3(stride_grid(n)), dim3(256), 0, ctx->stream, labels, n, (const int*)rank, ids);
    HIP_TRY(ctx, hipGetLastError());
    return 0;
}

// ------------------------------------------------------------------------------------------------ IDs unique in time
// rowmax[t] = max(0, max over c of ids[t][c])  (rowmax zeroed first)
__global__ void __launch_bounds__(256) k_mesh_row_max(const int* __restrict__ ids, long T, long C, int* __restrict__ rowmax) {
    for (long t = blockIdx.y; t < T; t += gridDim.y) {
        const int* row = ids + t * C;
        int m = 0;
        for (long c = (long)blockIdx.x * 256 + threadIdx.x; c < C; c += (long)gridDim.x * 256) {
            const int v = row[c];
            m = v > m ? v : m;
        }
        m = ~wave_min_i32(~m);  // ~ reverses the order, never overflows
        if ((threadIdx.x & 63) == 0 && m > 0) atomicMax(&rowmax[t], m);
    }
}

// out[t][c] = ids[t][c] > 0 ? ids[t][c] + off[t] : 0; ids and out may be the same array
__global__ void __launch_bounds__(256) k_mesh_add_row_offset(const int* ids, long T, long C, const int* __restrict__ off, int* out) {
    for (long t = blockIdx.y; t < T; t += gridDim.y) {
        const int o = off[t];
        for (long c = (long)blockIdx.x * 256 + threadIdx.x; c < C; c += (long)gridDim.x * 256) {
            const int v = ids[t * C + c];
            out[t * C + c] = v > 0 ? v + o : 0;
        }
    }
}

static inline dim3 mobj_row_grid(long T, long C) {
    const long per = (C + 255) / 256;
    return dim3((unsigned)(per < 1024 ? per : 1024), (unsigned)(T < 65535 ? T : 65535));
}

extern "C" int marex_ids_row_max_i32(marex_ctx* ctx, const int32_t* ids, int64_t T, int64_t C, int32_t* rowmax) {
    if (!ctx) return -1;
    if (!ids || !rowmax || T <= 0 || C <= 0) return fail(ctx, -1, "marex_ids_row_max_i32: null pointer or empty shape");
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    LaunchTimer lt(ctx, MAREX_K_MORPH);
    HIP_TRY(ctx, hipMemsetAsync(rowmax, 0, (size_t)T * sizeof(int), ctx->stream));
    hipLaunchKernelGGL(k_mesh_row_max, mobj_row_grid(T, C), dim3(256), 0, ctx->stream, ids, (long)T, (long)C, rowmax);
    HIP_TRY(ctx, hipGetLastError());
    return 0;
}

extern "C" int marex_ids_add_row_offset_i32(marex_ctx* ctx, const int32_t* ids, int64_t T, int64_t C, const int32_t* off,
                                            int32_t* out) {
    if (!ctx) return -1;
    if (!ids || !off || !out || T <= 0 || C <= 0) return fail(ctx, -1, "marex_ids_add_row_offset_i32: null pointer or empty shape");
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    LaunchTimer lt(ctx, MAREX_K_MORPH);
    hipLaunchKernelGGL(k_mesh_add_row_offset, mobj_row_grid(T, C), dim3(256), 0, ctx->stream, ids, (long)T, (long)C, off, out);
    HIP_TRY(ctx, hipGetLastError());
    return 0;
}

// ------------------------------------------------------------------------------------------------ object moments
// acc[slot][0..4] += cells, q0, q1, q2, q3 for every cell with ids[t][c] > 0, slot = off[id] + t - tmin[id]
// (marex_object_spans_i32).  The four rows of q are read by the lanes that hold an ID only.
__global__ void __launch_bounds__(256)
k_mesh_moments(const int* __restrict__ ids, long T, long C, const long long* __restrict__ q, const int* __restrict__ tmin,
               const long long* __restrict__ off, u64* __restrict__ acc) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const long rw = mobj_piece0(wave);
    for (long t = blockIdx.y; t < T; t += gridDim.y) {
        const int* row = ids + t * C;
        int v[MOBJ_ITERS];
#pragma unroll
        for (int k = 0; k < MOBJ_ITERS; ++k) {
            const long r = rw + 64 * k + lane;
            v[k] = r < C ? row[r] : 0;
        }
        int cur = 0;
        long long n = 0, s0 = 0, s1 = 0, s2 = 0, s3 = 0;
        auto flush = [&]() {
            if (cur > 0 && lane == 0) {
                u64* p = acc + (size_t)(off[cur] + (t - tmin[cur])) * MOBJ_MOM;
                atomicAdd(p + 0, (u64)n);
                atomicAdd(p + 1, (u64)s0);
                atomicAdd(p + 2, (u64)s1);
                atomicAdd(p + 3, (u64)s2);
                atomicAdd(p + 4, (u64)s3);
            }
        };
#pragma unroll  // v[k] must stay in registers: no dynamic indexing
        for (int k = 0; k < MOBJ_ITERS; ++k) {
            const long r0 = rw + 64 * k;
            if (r0 >= C) break;  // wave-uniform
            const int id = v[k] > 0 ? v[k] : 0;
            u64 todo = __ballot(id > 0);
            if (!todo) continue;
            long long q0 = 0, q1 = 0, q2 = 0, q3 = 0;
            if (id > 0) {  // id > 0 implies r0 + lane < C
                const long c = r0 + lane;
                q0 = q[c];
                q1 = q[C + c];
                q2 = q[2 * C + c];
                q3 = q[3 * C + c];
            }
            while (todo) {
                const int lead = __ffsll((long long)todo) - 1;
                const int il = __shfl(id, lead, 64);
                const u64 same = __ballot(id == il) & todo;
                todo &= ~same;
                const bool in = (same >> lane) & 1ull;
                const long long g0 = mobj_wave_sum_i64(in ? q0 : 0), g1 = mobj_wave_sum_i64(in ? q1 : 0),
                                g2 = mobj_wave_sum_i64(in ? q2 : 0), g3 = mobj_wave_sum_i64(in ? q3 : 0);
                if (il != cur) {
                    flush();
                    cur = il;
                    n = s0 = s1 = s2 = s3 = 0;
                }
                n += __popcll(same);
                s0 += g0;
                s1 += g1;
                s2 += g2;
                s3 += g3;
            }
        }
        flush();
    }
}

extern "C" int marex_mesh_object_moments_i64(marex_ctx* ctx, const int32_t* ids, int64_t T, int64_t C, const int64_t* q,
                                             const int32_t* tmin, const int64_t* off, int64_t n_slots, uint64_t* acc) {
    if (!ctx) return -1;
    if (!ids || !q || !tmin || !off || !acc || T <= 0 || C <= 0 || n_slots <= 0)
        return fail(ctx, -1, "marex_mesh_object_moments_i64: null pointer or empty shape");
    if (C >= 2147483647L || T >= 2147483647L) return fail(ctx, -4, "marex_mesh_object_moments_i64: a slice or the time axis has 2^31 - 1 or more entries");
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    LaunchTimer lt(ctx, MAREX_K_MORPH);
    HIP_TRY(ctx, hipMemsetAsync(acc, 0, (size_t)n_slots * MOBJ_MOM * sizeof(u64), ctx->stream));
    hipLaunchKernelGGL(k_mesh_moments, mobj_slice_grid(T, C), dim3(256), 0, ctx->stream, ids, (long)T, (long)C, (const long long*)q,
                       tmin, (const long long*)off, (u64*)acc);
    HIP_TRY(ctx, hipGetLastError());
    return 0;
}

// ------------------------------------------------------------------------------------------------ events: rename and accumulate
// One pass over the field, in place: ids[t][c] = ev = lut[v] for 0 < v = ids[t][c] < lut_len (anything else, and an ev
// outside 1..n_ev: 0), and for ev > 0 the dense slot s = t n_ev + ev - 1 takes acc[s][0..4] += 1, q0..q3[c] and
// gid[s] = max(gid[s], v).  k_mesh_moments with the event as the group key: a cell is read and written by one lane only,
// the run of an event is carried across the pieces of the wave and flushed once.
__global__ void __launch_bounds__(256)
k_mesh_event_rename(int* ids, long T, long C, const int* __restrict__ lut, long lut_len, int n_ev,
                    const long long* __restrict__ q, u64* __restrict__ acc, int* __restrict__ gid) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const long rw = mobj_piece0(wave);
    for (long t = blockIdx.y; t < T; t += gridDim.y) {
        int* row = ids + t * C;
        int v[MOBJ_ITERS], ev[MOBJ_ITERS];
#pragma unroll
        for (int k = 0; k < MOBJ_ITERS; ++k) {
            const long r = rw + 64 * k + lane;
            v[k] = r < C ? row[r] : 0;
        }
#pragma unroll
        for (int k = 0; k < MOBJ_ITERS; ++k) {
            const long r = rw + 64 * k + lane;
            int e = (v[k] > 0 && (long)v[k] < lut_len) ? lut[v[k]] : 0;
            e = (e > 0 && e <= n_ev) ? e : 0;  // the slot index below never comes from an unchecked value
            ev[k] = e;
            if (r < C && e != v[k]) row[r] = e;
        }
        int cur = 0, big = 0;
        long long n = 0, s0 = 0, s1 = 0, s2 = 0, s3 = 0;
        auto flush = [&]() {
            if (cur > 0 && lane == 0) {
                const size_t s = (size_t)t * (size_t)n_ev + (size_t)(cur - 1);
                u64* p = acc + s * MOBJ_MOM;
                atomicAdd(p + 0, (u64)n);
                atomicAdd(p + 1, (u64)s0);
                atomicAdd(p + 2, (u64)s1);
                atomicAdd(p + 3, (u64)s2);
                atomicAdd(p + 4, (u64)s3);
                atomicMax(gid + s, big);
            }
        };
#pragma unroll  // v[k], ev[k] must stay in registers: no dynamic indexing
        for (int k = 0; k < MOBJ_ITERS; ++k) {
            const long r0 = rw + 64 * k;
            if (r0 >= C) break;  // wave-uniform
            const int id = ev[k];
            u64 todo = __ballot(id > 0);
            if (!todo) continue;
            long long q0 = 0, q1 = 0, q2 = 0, q3 = 0;
            if (id > 0) {  // id > 0 implies r0 + lane < C
                const long c = r0 + lane;
                q0 = q[c];
                q1 = q[C + c];
                q2 = q[2 * C + c];
                q3 = q[3 * C + c];
            }
            while (todo) {
                const int lead = __ffsll((long long)todo) - 1;
                const int il = __shfl(id, lead, 64);
                const u64 same = __ballot(id == il) & todo;
                todo &= ~same;
                const bool in = (same >> lane) & 1ull;
                const long long g0 = mobj_wave_sum_i64(in ? q0 : 0), g1 = mobj_wave_sum_i64(in ? q1 : 0),
                                g2 = mobj_wave_sum_i64(in ? q2 : 0), g3 = mobj_wave_sum_i64(in ? q3 : 0);
                const int gm = wave_max_i32(in ? v[k] : 0);  // v > 0 wherever ev > 0
                if (il != cur) {
                    flush();
                    cur = il;
                    n = s0 = s1 = s2 = s3 = 0;
                    big = 0;
                }
                n += __popcll(same);
                s0 += g0;
                s1 += g1;
                s2 += g2;
                s3 += g3;
                big = gm > big ? gm : big;
            }
        }
        flush();
    }
}

extern "C" int marex_mesh_event_rename_i64(marex_ctx* ctx, int32_t* ids, int64_t T, int64_t C, const int32_t* lut,
                                           int64_t lut_len, int n_ev, const int64_t* q, uint64_t* acc, int32_t* gid) {
    if (!ctx) return -1;
    if (!ids || !lut || !q || !acc || !gid || T <= 0 || C <= 0 || lut_len <= 0 || n_ev <= 0)
        return fail(ctx, -1, "marex_mesh_event_rename_i64: null pointer or empty shape");
    if (C >= 2147483647L || T >= 2147483647L) return fail(ctx, -4, "marex_mesh_event_rename_i64: a slice or the time axis has 2^31 - 1 or more entries");
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    LaunchTimer lt(ctx, MAREX_K_MORPH);
    const size_t slots = (size_t)T * (size_t)n_ev;
    HIP_TRY(ctx, hipMemsetAsync(acc, 0, slots * MOBJ_MOM * sizeof(u64), ctx->stream));
    HIP_TRY(ctx, hipMemsetAsync(gid, 0, slots * sizeof(int), ctx->stream));
    hipLaunchKernelGGL(k_mesh_event_rename, mobj_slice_grid(T, C), dim3(256), 0, ctx->stream, ids, (long)T, (long)C, lut,
                       (long)lut_len, n_ev, (const long long*)q, (u64*)acc, gid);
    HIP_TRY(ctx, hipGetLastError());
    return 0;
}

// ------------------------------------------------------------------------------------------------ weighted overlaps
// key = a << 32 | b for every cell with a = ids[t] > 0 and b = ids[t + 1] > 0; each run of equal keys adds the sum of
// q0 over its cells to the key's entry of an open-addressing table (linear probing, CAS on the key, 0 = empty);
// stats[2] is set when a probe sequence found no free entry.  A pair that persists through many timesteps can add up to
// more than 64 bits hold (one slice stays below 2^62, T slices do not), so an entry is two words: every group sum g of one
// 64-cell piece goes in as g mod 2^32 and g >> 32, and the pair's sum is sums[h][1] * 2^32 + sums[h][0], exact for up to
// 2^32 groups per pair.
__global__ void __launch_bounds__(256)
k_mesh_ovl_insert(const int* __restrict__ ids, long T, long C, const long long* __restrict__ q0, long cap, u64* __restrict__ keys,
                  u64* __restrict__ sums, u64* __restrict__ stats) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const long rw = mobj_piece0(wave);
    u64 cur = 0, cs_lo = 0, cs_hi = 0;  // the run lives across the slices the wave visits: a pair that persists is inserted once
    auto flush = [&]() {
        if (!cur || lane != 0) return;
        const u64 mask = (u64)cap - 1;
        u64 h = splitmix64(cur) & mask;
        for (long p = 0; p < cap; ++p) {
            const u64 prev = atomicCAS(&keys[h], 0ull, cur);
            if (prev == 0ull || prev == cur) {
                atomicAdd(&sums[2 * h], cs_lo);
                atomicAdd(&sums[2 * h + 1], cs_hi);
                return;
            }
            h = (h + 1) & mask;
        }
        atomicOr(&stats[2], 1ull);
    };
    for (long t = blockIdx.y; t + 1 < T; t += gridDim.y) {
        const int* ra = ids + t * C;
        const int* rb = ra + C;
        int va[MOBJ_ITERS], vb[MOBJ_ITERS];
#pragma unroll
        for (int k = 0; k < MOBJ_ITERS; ++k) {
            const long r = rw + 64 * k + lane;
            va[k] = r < C ? ra[r] : 0;
            vb[k] = r < C ? rb[r] : 0;
        }
#pragma unroll  // v[k] must stay in registers: no dynamic indexing
        for (int k = 0; k < MOBJ_ITERS; ++k) {
            const u64 key = (va[k] > 0 && vb[k] > 0) ? ((u64)(unsigned)va[k] << 32) | (unsigned)vb[k] : 0ull;
            u64 todo = __ballot(key != 0);
            if (!todo) continue;
            const long long w = key ? q0[rw + 64 * k + lane] : 0;  // key != 0 implies the cell is inside the slice
            while (todo) {
                const int lead = __ffsll((long long)todo) - 1;
                const u64 kl = wave_shfl_u64(key, lead);
                const u64 same = __ballot(key == kl) & todo;
                todo &= ~same;
                const u64 g = (u64)mobj_wave_sum_i64(((same >> lane) & 1ull) ? w : 0);  // one slice: below 2^62
                if (kl != cur) {
                    flush();
                    cur = kl;
                    cs_lo = cs_hi = 0;
                }
                cs_lo += g & 0xFFFFFFFFull;
                cs_hi += g >> 32;
            }
        }
    }
    flush();
}

// occupied table entries -> out_keys / out_sums (no particular order; the host sorts by key); stats[3] = how many
__global__ void __launch_bounds__(256)
k_mesh_ovl_compact(long cap, const u64* __restrict__ keys, const u64* __restrict__ sums, long out_cap, u64* __restrict__ stats,
                   u64* __restrict__ out_keys, u64* __restrict__ out_sums) {
    for (long h = (long)blockIdx.x * 256 + threadIdx.x; h < cap; h += (long)gridDim.x * 256) {
        const u64 k = keys[h];
        if (!k) continue;
        const u64 p = atomicAdd(&stats[3], 1ull);
        if (p < (u64)out_cap) {
            out_keys[p] = k;
            out_sums[2 * p] = sums[2 * h];
            out_sums[2 * p + 1] = sums[2 * h + 1];
        }
    }
}

extern "C" int marex_mesh_overlap_pairs_i64(marex_ctx* ctx, const int32_t* ids, int64_t T, int64_t C, const int64_t* q0,
                                            int64_t cap, uint64_t* keys, uint64_t* sums, uint64_t* stats, int64_t out_cap,
                                            uint64_t* out_keys, uint64_t* out_sums) {
    if (!ctx) return -1;
    if (!ids || !q0 || !keys || !sums || !stats || !out_keys || !out_sums || T < 2 || C <= 0 || out_cap <= 0)
        return fail(ctx, -1, "marex_mesh_overlap_pairs_i64: null pointer, fewer than two slices or no room for pairs");
    if (cap < 64 || (cap & (cap - 1))) return fail(ctx, -1, "marex_mesh_overlap_pairs_i64: cap=%lld is not a power of two >= 64", (long long)cap);
    if (C >= 2147483647L || T >= 2147483647L) return fail(ctx, -4, "marex_mesh_overlap_pairs_i64: a slice or the time axis has 2^31 - 1 or more entries");
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    LaunchTimer lt(ctx, MAREX_K_MORPH);
    HIP_TRY(ctx, hipMemsetAsync(keys, 0, (size_t)cap * sizeof(u64), ctx->stream));
    HIP_TRY(ctx, hipMemsetAsync(sums, 0, (size_t)cap * 2 * sizeof(u64), ctx->stream));
    HIP_TRY(ctx, hipMemsetAsync(stats + 2, 0, 2 * sizeof(u64), ctx->stream));
    hipLaunchKernelGGL(k_mesh_ovl_insert, mobj_slice_grid(T - 1, C), dim3(256), 0, ctx->stream, ids, (long)T, (long)C,
                       (const long long*)q0, (long)cap, (u64*)keys, (u64*)sums, (u64*)stats);
    hipLaunchKernelGGL(k_mesh_ovl_compact, dim3(stride_grid(cap)), dim3(256), 0, ctx->stream, (long)cap, (const u64*)keys,
                       (const u64*)sums, (long)out_cap, (u64*)stats, (u64*)out_keys, (u64*)out_sums);
    HIP_TRY(ctx, hipGetLastError());
    return 0;
}

// ------------------------------------------------------------------------------------------------ area per timestep
// out[t] += sum of q0[c] over the cells of the workgroup's piece with data[t][c] != 0: registers, wave, LDS, one atomic
__global__ void __launch_bounds__(256)
k_mesh_area(const unsigned char* __restrict__ data, long T, long C, const long long* __restrict__ q0, u64* __restrict__ out) {
    __shared__ long long part[4];
    const long c0 = (long)blockIdx.x * MOBJ_CHUNK;
    for (long t = blockIdx.y; t < T; t += gridDim.y) {  // uniform over the workgroup
        const unsigned char* row = data + t * C;
        long long s = 0;
#pragma unroll
        for (int k = 0; k < MOBJ_ITERS; ++k) {
            const long c = c0 + 256 * k + threadIdx.x;
            if (c < C && row[c]) s += q0[c];
        }
        s = mobj_wave_sum_i64(s);
        if ((threadIdx.x & 63) == 0) part[threadIdx.x >> 6] = s;
        __syncthreads();
        if (threadIdx.x == 0) {
            const long long tot = part[0] + part[1] + part[2] + part[3];
            if (tot) atomicAdd(&out[t], (u64)tot);
        }
        __syncthreads();
    }
}

extern "C" int marex_mesh_area_i64(marex_ctx* ctx, const uint8_t* data, int64_t T, int64_t C, const int64_t* q0, uint64_t* out) {
    if (!ctx) return -1;
    if (!data || !q0 || !out || T <= 0 || C <= 0) return fail(ctx, -1, "marex_mesh_area_i64: null pointer or empty shape");
    if (C >= 2147483647L || T >= 2147483647L) return fail(ctx, -4, "marex_mesh_area_i64: a slice or the time axis has 2^31 - 1 or more entries");
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    LaunchTimer lt(ctx, MAREX_K_MORPH);
    HIP_TRY(ctx, hipMemsetAsync(out, 0, (size_t)T * sizeof(u64), ctx->stream));
    hipLaunchKernelGGL(k_mesh_area, slice_grid(T, C, MOBJ_CHUNK, 65535), dim3(256), 0, ctx->stream, data, (long)T, (long)C,
                       (const long long*)q0, (u64*)out);
    HIP_TRY(ctx, hipGetLastError());
    return 0;
}
