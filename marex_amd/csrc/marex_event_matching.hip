// marex_event_matching.hip -- the join of two tracked fields: per (timestep, event of A, event of B) the cells the two share
// and their area.  The scheme is that of marex_event_exposure.hip with a second streamed field where it has a region map:
//
//   count pass   the runs of equal (a, b) pairs, an upper bound of the distinct keys, and the largest ID of either field: the
//                caller plans the widths of the key and sizes the table from them
//   insert pass  every run adds its record to the key's entry of an open-addressing table (table_claim, marex_common.hip.h:
//                at most cap probes); a full table sets a status word, nothing spins, nothing is written outside the table
//   compaction   the occupied entries, in no particular order (k_table_compact; the host sorts them by key)
//
// Presence: a lane is present where a > 0 || b > 0 (a negative cell is counted and then background).  The pairs (a, 0) and
// (0, b) are kept: the cells of an event that the other field leaves uncovered, so that every total and share is exact.
//
// Key (u64): a << (bits_b + bits_step) | b << bits_step | step, with the three widths given by the caller at run time.  Two
// 31-bit IDs and a 17-bit step are 79 bits, and there is no 128-bit compare-and-swap on global memory: a two-word key would
// need a lock or a spin on a half-written entry.  The IDs of one window seldom need 31 bits, so the caller measures them (the
// count pass) and gives the step what is left of 64 bits, at least 2; a window of more steps than that is run in pieces.  No
// key is 0, since (0, 0) is not present.  An ID that does not fit its width is counted (status[6]) and dropped before a key
// is formed: never mis-keyed.  Sorted as integers the keys are in (a, b, step) order.
//
// Shape: as k_exp_pass -- a workgroup of four waves takes MAT_WG_CELLS consecutive cells and every gridDim.y-th row (at most
// MAT_TSTRIDE rows in flight), a wave MAT_ITERS consecutive 64-cell pieces of both fields (2 MAT_ITERS loads in flight per
// lane); q is read under present lanes only.  A wave folds the equal pairs of a piece with the ballot loop, keeps the run of
// the current pair in wave-uniform registers -- the pair, not the key: the key is formed once per run, at the flush -- and
// lane 0 issues the atomics of a run.
//
// Arithmetic contract: cells and areas are integers, exact and independent of order, windows, widths and layout.
#include "marex_common.hip.h"

#define MAT_ITERS 8                      // 64-cell pieces per wave, of each field
#define MAT_WAVE_CELLS (64 * MAT_ITERS)  // cells of a wave per row
#define MAT_WG_CELLS (4 * MAT_WAVE_CELLS)
#define MAT_TSTRIDE 32                   // rows in flight: a workgroup walks every MAT_TSTRIDE-th row
#define MAT_ID_BITS 31                   // the most an ID takes
#define MAT_MIN_STEP_BITS (64 - 2 * MAT_ID_BITS)

// status words (uint64 [8]); the count pass writes 0 .. 4, the insert pass and the compaction 5 .. 7
#define MAT_ST_NEG_A 0
#define MAT_ST_NEG_B 1
#define MAT_ST_RUNS 2
#define MAT_ST_MAX_A 3
#define MAT_ST_MAX_B 4
#define MAT_ST_FULL 5
#define MAT_ST_OVER 6
#define MAT_ST_OUT 7

// Rows 0 .. Tb - 1 of ia and ib [Tb][C].  INSERT false: the count pass (q, the widths and the table are not touched).  The
// entry point has checked the widths (each >= 1, their sum <= 64), Tb <= 2^bits_step and cap.
template <bool INSERT>
__global__ void __launch_bounds__(256)
k_mat_pass(const int* __restrict__ ia, const int* __restrict__ ib, long Tb, long C, const long long* __restrict__ q, int bits_a,
           int bits_b, int bits_step, long cap, u64* __restrict__ keys, u64* __restrict__ cnt, u64* __restrict__ area,
           u64* __restrict__ status) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const long rw = ((long)blockIdx.x * 4 + wave) * MAT_WAVE_CELLS;
    u64 runs = 0, over = 0;
    unsigned neg_a = 0, neg_b = 0;
    int max_a = 0, max_b = 0;
    bool full = false;
    // the run of the current pair (a << 32 | b): wave-uniform
    u64 cur = 0;
    unsigned rc = 0;
    long long ra = 0;
    auto flush = [&](long row) {
        if (!cur) return;
        ++runs;
        if (INSERT && lane == 0) {
            const u64 a = cur >> 32, b = cur & 0xFFFFFFFFull;
            if ((a >> bits_a) | (b >> bits_b)) {
                over += rc;  // an ID wider than the caller said: dropped, never mis-keyed
            } else {
                const u64 key = (a << (bits_b + bits_step)) | (b << bits_step) | (u64)row;
                const long h = table_claim(keys, cap, key);  // bounded: a full table is a status, not a spin
                if (h >= 0) {
                    atomicAdd(&cnt[h], (u64)rc);
                    if (area) atomicAdd(&area[h], (u64)ra);
                } else {
                    full = true;
                }
            }
        }
        cur = 0;
        rc = 0;
        ra = 0;
    };
    for (long row = blockIdx.y; row < Tb; row += gridDim.y) {
        const int* arow = ia + (size_t)row * (size_t)C;
        const int* brow = ib + (size_t)row * (size_t)C;
        int va[MAT_ITERS], vb[MAT_ITERS];
#pragma unroll
        for (int k = 0; k < MAT_ITERS; ++k) {
            const long c = rw + 64L * k + lane;
            va[k] = c < C ? arow[c] : 0;
            vb[k] = c < C ? brow[c] : 0;
        }
#pragma unroll  // va[k], vb[k] must stay in registers: no dynamic indexing
        for (int k = 0; k < MAT_ITERS; ++k) {
            const long c = rw + 64L * k + lane;  // present implies c < C
            if (!INSERT) {
                neg_a += va[k] < 0;
                neg_b += vb[k] < 0;
                max_a = va[k] > max_a ? va[k] : max_a;
                max_b = vb[k] > max_b ? vb[k] : max_b;
            }
            const unsigned a = va[k] > 0 ? (unsigned)va[k] : 0u, b = vb[k] > 0 ? (unsigned)vb[k] : 0u;
            const u64 pair = ((u64)a << 32) | (u64)b;  // 0: not present
            u64 todo = __ballot(pair != 0);
            if (!todo) continue;  // wave-uniform
            long long qa = 1;
            if (INSERT && q && pair) qa = q[c];
            while (todo) {  // at most 64 rounds: each takes at least the leading lane
                const int lead = __ffsll((long long)todo) - 1;
                const u64 pl = wave_shfl_u64(pair, lead);
                const bool mine = pair == pl;  // pl != 0: only present lanes
                const u64 same = __ballot(mine);
                todo &= ~same;
                if (pl != cur) {
                    flush(row);
                    cur = pl;
                }
                if (INSERT) {
                    rc += (unsigned)__popcll(same);
                    if (q) ra += dpp_wave_sum(mine ? qa : 0LL);
                }
            }
        }
        flush(row);  // the step is part of the key
    }
    if (INSERT) {
        if (lane == 0 && full) atomicOr(&status[MAT_ST_FULL], 1ull);
        if (lane == 0 && over) atomicAdd(&status[MAT_ST_OVER], over);
        return;
    }
    __shared__ u64 part[5][4];  // one set of atomics per workgroup on the shared counters
    const u64 na = dpp_wave_sum((u64)neg_a), nb = dpp_wave_sum((u64)neg_b);
    const int ma = wave_max_i32(max_a), mb = wave_max_i32(max_b);
    if (lane == 0) {
        part[0][wave] = na;
        part[1][wave] = nb;
        part[2][wave] = runs;
        part[3][wave] = (u64)ma;
        part[4][wave] = (u64)mb;
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        const u64 ga = part[0][0] + part[0][1] + part[0][2] + part[0][3], gb = part[1][0] + part[1][1] + part[1][2] + part[1][3],
                  n = part[2][0] + part[2][1] + part[2][2] + part[2][3];
        u64 xa = 0, xb = 0;
        for (int w = 0; w < 4; ++w) {
            xa = part[3][w] > xa ? part[3][w] : xa;
            xb = part[4][w] > xb ? part[4][w] : xb;
        }
        if (ga) atomicAdd(&status[MAT_ST_NEG_A], ga);
        if (gb) atomicAdd(&status[MAT_ST_NEG_B], gb);
        if (n) atomicAdd(&status[MAT_ST_RUNS], n);
        if (xa) atomicMax(&status[MAT_ST_MAX_A], xa);
        if (xb) atomicMax(&status[MAT_ST_MAX_B], xb);
    }
}

static inline dim3 mat_grid(long Tb, long C) {
    return slice_grid(Tb, C, MAT_WG_CELLS, MAT_TSTRIDE);
}

// the constants the kernels above are compiled with, for callers and tests that place cases at their edges
extern "C" int marex_event_matching_layout(int32_t* out) {
    if (!out) return -1;
    out[0] = 64;              // cells of a piece
    out[1] = MAT_WAVE_CELLS;  // cells of a wave per row
    out[2] = MAT_WG_CELLS;    // cells of a workgroup per row
    out[3] = MAT_TSTRIDE;     // rows between two of a workgroup's
    out[4] = MAT_ID_BITS;
    out[5] = MAT_MIN_STEP_BITS;
    return 0;
}

extern "C" int marex_event_matching_count_i32(marex_ctx* ctx, const int32_t* ids_a, const int32_t* ids_b, int64_t Tb, int64_t C,
                                              uint64_t* status) {
    const char* name = "marex_event_matching_count_i32";
    if (!ctx) return -1;
    if (!ids_a || !ids_b || !status || Tb <= 0 || C <= 0) return fail(ctx, -1, "%s: null pointer or empty shape", name);
    if (const int rc = cell_stream_limits(ctx, name, 0, Tb, C)) return rc;
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    LaunchTimer lt(ctx, MAREX_K_MORPH);
    HIP_TRY(ctx, hipMemsetAsync(status, 0, 8 * sizeof(u64), ctx->stream));
    hipLaunchKernelGGL((k_mat_pass<false>), mat_grid(Tb, C), dim3(256), 0, ctx->stream, ids_a, ids_b, (long)Tb, (long)C,
                       (const long long*)nullptr, 0, 0, 0, 0L, (u64*)nullptr, (u64*)nullptr, (u64*)nullptr, (u64*)status);
    HIP_TRY(ctx, hipGetLastError());
    return 0;
}

extern "C" int marex_event_matching_i32(marex_ctx* ctx, const int32_t* ids_a, const int32_t* ids_b, int64_t Tb, int64_t C,
                                        const int64_t* q, int bits_a, int bits_b, int bits_step, int64_t cap, uint64_t* keys,
                                        uint64_t* cnt, int64_t* area, uint64_t* status, int64_t out_cap, uint64_t* out_keys,
                                        uint64_t* out_cnt, int64_t* out_area) {
    const char* name = "marex_event_matching_i32";
    if (!ctx) return -1;
    const int nar = (q != nullptr) + (area != nullptr) + (out_area != nullptr);
    if (!ids_a || !ids_b || !keys || !cnt || !status || !out_keys || !out_cnt || Tb <= 0 || C <= 0 || out_cap <= 0 ||
        (nar != 0 && nar != 3))
        return fail(ctx, -1, "%s: null pointer, empty shape, no room for entries, or area arguments given in part", name);
    if (cap < 64 || (cap & (cap - 1))) return fail(ctx, -1, "%s: cap=%lld is not a power of two >= 64", name, (long long)cap);
    if (bits_a < 1 || bits_b < 1 || bits_step < 1 || (long)bits_a + bits_b + bits_step > 64)
        return fail(ctx, -1, "%s: the widths %d + %d + %d of the key: each takes at least 1 bit, together at most 64", name, bits_a,
                    bits_b, bits_step);
    if (Tb > (1L << bits_step))
        return fail(ctx, -4, "%s: a window of %lld steps, the key takes %ld", name, (long long)Tb, 1L << bits_step);
    if (const int rc = cell_stream_limits(ctx, name, 0, Tb, C)) return rc;
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    {
        LaunchTimer lt(ctx, MAREX_K_MORPH);
        HIP_TRY(ctx, hipMemsetAsync(keys, 0, (size_t)cap * sizeof(u64), ctx->stream));
        HIP_TRY(ctx, hipMemsetAsync(cnt, 0, (size_t)cap * sizeof(u64), ctx->stream));
        if (area) HIP_TRY(ctx, hipMemsetAsync(area, 0, (size_t)cap * sizeof(u64), ctx->stream));
        HIP_TRY(ctx, hipMemsetAsync(status + MAT_ST_FULL, 0, 3 * sizeof(u64), ctx->stream));
        hipLaunchKernelGGL((k_mat_pass<true>), mat_grid(Tb, C), dim3(256), 0, ctx->stream, ids_a, ids_b, (long)Tb, (long)C,
                           (const long long*)q, bits_a, bits_b, bits_step, (long)cap, (u64*)keys, (u64*)cnt, (u64*)area, (u64*)status);
    }
    {
        LaunchTimer lt(ctx, MAREX_K_MORPH);
        hipLaunchKernelGGL(k_table_compact<MAT_ST_OUT>, dim3(stride_grid(cap)), dim3(256), 0, ctx->stream, (long)cap,
                           (const u64*)keys, (const u64*)cnt, (const u64*)area, (const double*)nullptr, (const unsigned*)nullptr,
                           (long)out_cap, (u64*)status, (u64*)out_keys, (u64*)out_cnt, (u64*)out_area, (double*)nullptr,
                           (unsigned*)nullptr);
    }
    HIP_TRY(ctx, hipGetLastError());
    return 0;
}
