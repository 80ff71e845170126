// marex_event_exposure.hip -- the join of tracked events with regions: per (timestep, region, event) the cells of the event in
// the region, their area, the weighted anomaly sums and the largest anomaly.  The result is sparse -- an event touches one or
// two regions, a region sees a small share of the events -- so this is no dense slot array like the other statistics but a
// keyed accumulation, the scheme of k_ovl_pass (marex_objects.hip) with a record per key and the step in the key:
//
//   count pass   the runs of equal keys, an upper bound of the distinct keys: the caller sizes the table from it
//   insert pass  every run adds its record to the key's entry of an open-addressing table (linear probing, CAS on the key,
//                0 = empty, at most cap probes); a full table sets status[1], nothing spins, nothing is written outside it
//   compaction   the occupied entries, in no particular order (the host sorts them by key)
//
// Key (u64): id << 33 | rank << 17 | step -- 31 bits of ID (1 .. 2^31 - 1, so no key is 0), 16 of region rank (R, the rank of
// "no region", included), 17 of the step within the window.  Sorted as integers the keys are in (ID, region, time) order.
//
// Shape: a workgroup of four waves takes EXP_WG_CELLS consecutive cells and every gridDim.y-th row (at most EXP_TSTRIDE rows
// in flight, the strided-row grid of obj_slice_grid / REG_TSTRIDE: few enough workgroups that same-address atomics stay
// rare); a wave takes EXP_ITERS consecutive 64-cell pieces.  The ID rows are read once per pass; the region, the anomaly and
// the area are read under event cells only, the weight under event cells with a finite anomaly.  A wave folds the equal keys
// of a piece with the ballot loop of k_ovl_pass, reduces each group over the wave (dpp_wave_sum) and keeps the run of the
// current key in wave-uniform registers for as long as consecutive groups share the key; lane 0 issues the atomics of a run.
//
// Arithmetic contract: cells, finite cells, areas, maxima and steps are integers, exact and independent of order, windows
// and layout.  The two float64 sums follow marex_event_intensity_f32: sums of exact products ((double)w * (double)a of two
// float32 values; -ffp-contract=off), added in an order that depends on the layout and on the arrival of the atomics: bit
// for bit reproducible whenever the partial sums are exactly representable, otherwise within 2 n u sum|w a| of the exact sum.
#include "marex_common.hip.h"

#define EXP_ITERS 8                      // 64-cell pieces per wave
#define EXP_WAVE_CELLS (64 * EXP_ITERS)  // cells of a wave per row
#define EXP_WG_CELLS (4 * EXP_WAVE_CELLS)
#define EXP_TSTRIDE 32                   // rows in flight: a workgroup walks every EXP_TSTRIDE-th row
#define EXP_STEP_BITS 17
#define EXP_RANK_BITS 16
#define EXP_ID_BITS 31
static_assert(EXP_STEP_BITS + EXP_RANK_BITS + EXP_ID_BITS == 64, "the key is one u64");

// status words (uint64 [8]): 0 negative cells (count pass), 1 table full, 2 runs, 3 compacted entries, 4 event cells
#define EXP_ST_NEG 0
#define EXP_ST_FULL 1
#define EXP_ST_RUNS 2
#define EXP_ST_OUT 3
#define EXP_ST_CELLS 4

// Rows 0 .. Tb - 1: ids (and anom) [Tb][C].  INSERT false: the count pass (q, wf, anom and the table are not touched).
// A region outside 0 .. R - 1 is rank R, "no region", before it enters a key; the entry point has checked R, Tb and cap.
template <bool INSERT, bool ANOM>
__global__ void __launch_bounds__(256)
k_exp_pass(const int* __restrict__ ids, long Tb, long C, const int* __restrict__ reg, int R, const long long* __restrict__ q,
           const float* __restrict__ wf, const float* __restrict__ anom, long cap, u64* __restrict__ keys, u64* __restrict__ cnt,
           u64* __restrict__ area, double* __restrict__ sums, unsigned* __restrict__ vmax, u64* __restrict__ status) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const long rw = ((long)blockIdx.x * 4 + wave) * EXP_WAVE_CELLS;
    u64 cells = 0, runs = 0;
    unsigned neg = 0;
    bool full = false;
    // the run of the current key: wave-uniform
    u64 cur = 0;
    unsigned rc = 0, rf = 0, rkey = 0;
    long long ra = 0;
    double rsw = 0, rswa = 0;
    auto flush = [&]() {
        if (!cur) return;
        ++runs;
        if (INSERT && lane == 0) {
            const long h = table_claim(keys, cap, cur);  // bounded: a full table is a status, not a spin
            if (h >= 0) {
                atomicAdd(&cnt[h], ((u64)rf << 32) | (u64)rc);  // a step holds fewer than 2^31 cells: no carry between the halves
                if (area) atomicAdd(&area[h], (u64)ra);
                if (ANOM && rf) {
                    atomicAdd(&sums[2 * h], rsw);
                    atomicAdd(&sums[2 * h + 1], rswa);
                    atomicMax(&vmax[h], rkey);
                }
            } else {
                full = true;
            }
        }
        cur = 0;
        rc = rf = rkey = 0;
        ra = 0;
        rsw = rswa = 0;
    };
    for (long row = blockIdx.y; row < Tb; row += gridDim.y) {
        const int* xrow = ids + (size_t)row * (size_t)C;
        int v[EXP_ITERS];
#pragma unroll
        for (int k = 0; k < EXP_ITERS; ++k) {
            const long c = rw + 64L * k + lane;
            v[k] = c < C ? xrow[c] : 0;
        }
#pragma unroll  // v[k] must stay in registers: no dynamic indexing
        for (int k = 0; k < EXP_ITERS; ++k) {
            const long c = rw + 64L * k + lane;  // present implies c < C
            const bool present = v[k] > 0;
            neg += v[k] < 0;
            u64 todo = __ballot(present);
            if (!todo) continue;  // wave-uniform
            cells += __popcll(todo);
            u64 key = 0;
            bool fin = false;
            float a = 0.f, w = 1.f;
            long long qa = 1;
            if (present) {
                const int rv = reg[c];
                const int r = (rv >= 0 && rv < R) ? rv : R;
                key = ((u64)(unsigned)v[k] << (EXP_RANK_BITS + EXP_STEP_BITS)) | ((u64)(unsigned)r << EXP_STEP_BITS) | (u64)row;
                if (INSERT) {
                    fin = true;
                    if (ANOM) {
                        a = anom[(size_t)row * (size_t)C + c];
                        fin = finite_bits(a);
                    }
                    if (q) qa = q[c];
                    if (ANOM && wf && fin) w = wf[c];
                }
            }
            const double dw = fin ? (double)w : 0.0;
            const double dwa = fin ? dw * (double)a : 0.0;  // a select, not a product with 0: a may be NaN
            const unsigned ky = (ANOM && fin) ? ordered_key(a) : 0u;
            while (todo) {  // at most 64 rounds: each takes at least the leading lane
                const int lead = __ffsll((long long)todo) - 1;
                const u64 kl = wave_shfl_u64(key, lead);
                const bool mine = key == kl;  // kl != 0: only present lanes
                const u64 same = __ballot(mine);
                todo &= ~same;
                if (kl != cur) {
                    flush();
                    cur = kl;
                }
                if (INSERT) {
                    const unsigned n = (unsigned)__popcll(same);
                    const unsigned nf = ANOM ? (unsigned)__popcll(__ballot(mine && fin)) : n;
                    rc += n;
                    rf += nf;
                    if (q) ra += dpp_wave_sum(mine ? qa : 0LL);
                    if (ANOM && nf) {  // wave-uniform
                        rsw += wf ? dpp_wave_sum(mine ? dw : 0.0) : (double)nf;
                        rswa += dpp_wave_sum(mine ? dwa : 0.0);
                        const unsigned m = dpp_wave_max_u32(mine ? ky : 0u);
                        rkey = m > rkey ? m : rkey;
                    }
                }
            }
        }
        flush();  // the step is part of the key
    }
    if (INSERT) {
        if (lane == 0 && full) atomicOr(&status[EXP_ST_FULL], 1ull);
        return;
    }
    __shared__ u64 part[3][4];  // one set of atomics per workgroup on the shared counters
    const u64 negs = dpp_wave_sum((u64)neg);
    if (lane == 0) {
        part[0][wave] = cells;
        part[1][wave] = runs;
        part[2][wave] = negs;
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        const u64 c = part[0][0] + part[0][1] + part[0][2] + part[0][3], n = part[1][0] + part[1][1] + part[1][2] + part[1][3],
                  g = part[2][0] + part[2][1] + part[2][2] + part[2][3];
        if (c) atomicAdd(&status[EXP_ST_CELLS], c);
        if (n) atomicAdd(&status[EXP_ST_RUNS], n);
        if (g) atomicAdd(&status[EXP_ST_NEG], g);
    }
}

static inline dim3 exp_grid(long Tb, long C) {
    return slice_grid(Tb, C, EXP_WG_CELLS, EXP_TSTRIDE);
}

static int exp_limits(marex_ctx* ctx, const char* name, int64_t Tb, int64_t C, int R) {
    if (R <= 0 || R >= (1 << (EXP_RANK_BITS - 1)))
        return fail(ctx, -1, "%s: R=%d regions, the key takes 1 .. %d", name, R, (1 << (EXP_RANK_BITS - 1)) - 1);
    if (Tb > (1L << EXP_STEP_BITS)) return fail(ctx, -4, "%s: a window of %lld steps, the key takes %ld", name, (long long)Tb, 1L << EXP_STEP_BITS);
    return cell_stream_limits(ctx, name, 0, Tb, C);
}

// the constants the kernels above are compiled with, for callers and tests that place cases at their edges
extern "C" int marex_event_exposure_layout(int32_t* out) {
    if (!out) return -1;
    out[0] = 64;              // cells of a piece
    out[1] = EXP_WAVE_CELLS;  // cells of a wave per row
    out[2] = EXP_WG_CELLS;    // cells of a workgroup per row
    out[3] = EXP_TSTRIDE;     // rows between two of a workgroup's
    out[4] = EXP_ID_BITS;
    out[5] = EXP_RANK_BITS;
    out[6] = EXP_STEP_BITS;
    return 0;
}

extern "C" int marex_event_exposure_count_i32(marex_ctx* ctx, const int32_t* ids, int64_t Tb, int64_t C, const int32_t* reg, int R,
                                              uint64_t* status) {
    if (!ctx) return -1;
    if (!ids || !reg || !status || Tb <= 0 || C <= 0) return fail(ctx, -1, "marex_event_exposure_count_i32: null pointer or empty shape");
    if (const int rc = exp_limits(ctx, "marex_event_exposure_count_i32", Tb, C, R)) return rc;
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    LaunchTimer lt(ctx, MAREX_K_MORPH);
    HIP_TRY(ctx, hipMemsetAsync(status, 0, 8 * sizeof(u64), ctx->stream));
    hipLaunchKernelGGL((k_exp_pass<false, false>), exp_grid(Tb, C), dim3(256), 0, ctx->stream, ids, (long)Tb, (long)C, reg, R,
                       (const long long*)nullptr, (const float*)nullptr, (const float*)nullptr, 0L, (u64*)nullptr, (u64*)nullptr,
                       (u64*)nullptr, (double*)nullptr, (unsigned*)nullptr, (u64*)status);
    HIP_TRY(ctx, hipGetLastError());
    return 0;
}

extern "C" int marex_event_exposure_i32(marex_ctx* ctx, const int32_t* ids, int64_t Tb, int64_t C, const int32_t* reg, int R,
                                        const int64_t* q, const float* wf, const float* anom, int64_t cap, uint64_t* keys,
                                        uint64_t* cnt, int64_t* area, double* sums, uint32_t* vmax, uint64_t* status,
                                        int64_t out_cap, uint64_t* out_keys, uint64_t* out_cnt, int64_t* out_area,
                                        double* out_sums, uint32_t* out_vmax) {
    const char* name = "marex_event_exposure_i32";
    if (!ctx) return -1;
    const int nan = (anom != nullptr) + (sums != nullptr) + (vmax != nullptr) + (out_sums != nullptr) + (out_vmax != nullptr);
    const int nar = (q != nullptr) + (area != nullptr) + (out_area != nullptr);
    if (!ids || !reg || !keys || !cnt || !status || !out_keys || !out_cnt || Tb <= 0 || C <= 0 || out_cap <= 0 ||
        (nan != 0 && nan != 5) || (nar != 0 && nar != 3) || (wf && !anom))
        return fail(ctx, -1, "%s: null pointer, empty shape, no room for entries, anomaly or area arguments given in part, or "
                             "weights without anomalies", name);
    if (cap < 64 || (cap & (cap - 1))) return fail(ctx, -1, "%s: cap=%lld is not a power of two >= 64", name, (long long)cap);
    if (const int rc = exp_limits(ctx, name, Tb, C, R)) return rc;
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    {
        LaunchTimer lt(ctx, MAREX_K_MORPH);
        HIP_TRY(ctx, hipMemsetAsync(keys, 0, (size_t)cap * sizeof(u64), ctx->stream));
        HIP_TRY(ctx, hipMemsetAsync(cnt, 0, (size_t)cap * sizeof(u64), ctx->stream));
        if (area) HIP_TRY(ctx, hipMemsetAsync(area, 0, (size_t)cap * sizeof(u64), ctx->stream));
        if (anom) {
            HIP_TRY(ctx, hipMemsetAsync(sums, 0, (size_t)cap * 2 * sizeof(double), ctx->stream));
            HIP_TRY(ctx, hipMemsetAsync(vmax, 0, (size_t)cap * sizeof(unsigned), ctx->stream));
        }
        HIP_TRY(ctx, hipMemsetAsync(status + EXP_ST_FULL, 0, sizeof(u64), ctx->stream));
        HIP_TRY(ctx, hipMemsetAsync(status + EXP_ST_OUT, 0, sizeof(u64), ctx->stream));
#define EXP_GO(ANOM)                                                                                                          \
    hipLaunchKernelGGL((k_exp_pass<true, ANOM>), exp_grid(Tb, C), dim3(256), 0, ctx->stream, ids, (long)Tb, (long)C, reg, R,   \
                       (const long long*)q, wf, anom, (long)cap, (u64*)keys, (u64*)cnt, (u64*)area, sums, (unsigned*)vmax,     \
                       (u64*)status)
        if (anom)
            EXP_GO(true);
        else
            EXP_GO(false);
#undef EXP_GO
    }
    {
        LaunchTimer lt(ctx, MAREX_K_MORPH);
        hipLaunchKernelGGL(k_table_compact<EXP_ST_OUT>, dim3(stride_grid(cap)), dim3(256), 0, ctx->stream, (long)cap, (const u64*)keys,
                           (const u64*)cnt, (const u64*)area, (const double*)sums, (const unsigned*)vmax, (long)out_cap,
                           (u64*)status, (u64*)out_keys, (u64*)out_cnt, (u64*)out_area, out_sums, (unsigned*)out_vmax);
    }
    HIP_TRY(ctx, hipGetLastError());
    return 0;
}
