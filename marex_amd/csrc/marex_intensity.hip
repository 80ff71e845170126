// marex_intensity.hip -- per-(timestep, event) intensity sums: the tracked ID field joined with the anomaly field it was
// detected in (the reference leaves this to notebook code: groupby / where over ID_field and dat_anomaly).  One streaming
// pass of the shape of k_mrg_event_rename (marex_merge.hip) over two read-only inputs: the int32 event IDs, and the float32
// anomalies, which are fetched only under the cells that belong to an event.
//
// Arithmetic contract: the two counts and the maximum are exact and independent of any order.  The two float64 sums are
// atomic adds of exact terms ((double)w * (double)a of two float32 values is exact; compiled with -ffp-contract=off): bit
// for bit reproducible whenever the partial sums are exactly representable, otherwise within 2 n u sum|w a| (n finite
// cells of the slot, u = 2^-53) of the exact sum -- the precedent of the weighted grid moments (wacc of
// marex_event_rename_i32), not the integer contract of the mesh areas.
#include "marex_common.hip.h"

#define INT_ITERS 16                  // 64-cell pieces per wave
#define INT_BATCH 4                   // pieces loaded together (loads in flight per lane); INT_ITERS is a multiple
#define INT_CHUNK (256 * INT_ITERS)   // cells of a row per workgroup (4 waves)
#define INT_TSTRIDE 64                // rows in flight: a workgroup walks every INT_TSTRIDE-th row

__device__ __forceinline__ unsigned int_wave_max_u32(unsigned v) {
    for (int o = 32; o; o >>= 1) {
        const unsigned w = (unsigned)__shfl_xor((int)v, o, 64);
        v = w > v ? w : v;
    }
    return v;
}

// Rows t0 .. t0 + Tb - 1 of the field: ids / anom [Tb][C].  A cell of event e = ids[row][c] in 1 .. n_ev at the global
// timestep t = t0 + row belongs to the slot s = ev_off[e] + t - ev_tmin[e] (the compact slots of k_mrg_event_rename).  A wave
// walks INT_ITERS consecutive 64-cell pieces of a row, INT_BATCH at a time: the IDs of the batch are loaded first, the
// anomalies (and weights) only by the lanes whose ID is an event, so a piece without an event costs no anomaly cache line.
// The lanes of a piece are grouped by event (ballot); the run of an event is carried across its pieces in uniform
// registers and flushed once, when the event changes: lanes 0 and 1 add the two counts and the two float64 sums of the slot
// (16 contiguous bytes each), lane 2 raises the maximum -- the interior of a large event costs one set of atomics per 1024
// cells.  The slot index is checked against the event's own span and against n_slots before it addresses anything; a run
// outside it adds its cells to status[0] instead.  Nothing is zeroed here: the accumulators continue over time blocks.
template <bool WEIGHTED>
__global__ void __launch_bounds__(256)
k_evt_intensity(const int* __restrict__ ids, const float* __restrict__ anom, long t0, long Tb, long C, int n_ev,
                const int* __restrict__ ev_tmin, const long long* __restrict__ ev_off, long long n_slots,
                const float* __restrict__ w, u64* __restrict__ cnt, double* __restrict__ sums, unsigned* __restrict__ vmax,
                u64* __restrict__ status) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const long rw = (long)blockIdx.x * INT_CHUNK + (long)wave * (64 * INT_ITERS);
    for (long row = blockIdx.y; row < Tb; row += gridDim.y) {
        const int* irow = ids + row * C;
        const float* arow = anom + row * C;
        const long long t = t0 + row;
        int cur = 0;
        unsigned big = 0;
        long long nf = 0, nb = 0;
        double sw = 0, swa = 0;
        auto flush = [&]() {
            if (cur <= 0) return;  // wave-uniform
            const int tm = ev_tmin[cur];
            const long long o0 = ev_off[cur], o1 = ev_off[cur + 1];
            const long long s = o0 + (t - tm);
            if (t < tm || o0 < 0 || s >= o1 || s >= n_slots) {  // outside the declared span: counted, not accumulated
                if (lane == 0) atomicAdd(status, (u64)(nf + nb));
                return;
            }
            if (lane < 2) {
                if (lane == 0 ? nf != 0 : nb != 0) atomicAdd(cnt + (size_t)s * 2 + lane, (u64)(lane == 0 ? nf : nb));
                if (nf) atomicAdd(sums + (size_t)s * 2 + lane, lane == 0 ? sw : swa);
            } else if (lane == 2) {
                if (big) atomicMax(vmax + s, big);
            }
        };
#pragma unroll 1
        for (int b = 0; b < INT_ITERS; b += INT_BATCH) {
            if (rw + 64 * b >= C) break;  // wave-uniform
            int ev[INT_BATCH];
            float av[INT_BATCH], wv[INT_BATCH];
#pragma unroll
            for (int k = 0; k < INT_BATCH; ++k) {
                const long r = rw + 64 * (b + k) + lane;
                const int v = r < C ? irow[r] : 0;
                ev[k] = (v > 0 && v <= n_ev) ? v : 0;  // ev_tmin / ev_off are never indexed by an unchecked value
            }
#pragma unroll
            for (int k = 0; k < INT_BATCH; ++k) {
                const long r = rw + 64 * (b + k) + lane;  // ev[k] > 0 implies r < C
                av[k] = ev[k] > 0 ? arow[r] : 0.f;
                wv[k] = (WEIGHTED && ev[k] > 0) ? w[r] : 1.f;
            }
#pragma unroll  // ev[k], av[k], wv[k] must stay in registers: no dynamic indexing
            for (int k = 0; k < INT_BATCH; ++k) {
                const int e = ev[k];
                u64 todo = __ballot(e > 0);
                if (!todo) continue;
                const float a = av[k];
                // finite_bits(a), written out: behind the function the compiler picks a class test here, other instructions
                const bool fin = (__float_as_uint(a) & 0x7F800000u) != 0x7F800000u;  // neither NaN nor +-inf
                while (todo) {
                    const int lead = __ffsll((long long)todo) - 1;
                    const int el = __shfl(e, lead, 64);
                    const u64 same = __ballot(e == el) & todo;
                    todo &= ~same;
                    const bool me = ((same >> lane) & 1ull) && fin;
                    const u64 good = __ballot(me);
                    const int gf = __popcll(good), gb = __popcll(same) - gf;
                    double gw = (double)gf, gwa = 0;
                    unsigned gk = 0;
                    if (good) {  // wave-uniform
                        const double x = me ? (double)wv[k] : 0.0;
                        if (WEIGHTED) gw = wave_sum(x);
                        gwa = wave_sum(me ? x * (double)a : 0.0);
                        gk = int_wave_max_u32(me ? ordered_key(a) : 0u);
                    }
                    if (el != cur) {
                        flush();
                        cur = el;
                        nf = nb = 0;
                        sw = swa = 0;
                        big = 0;
                    }
                    nf += gf;
                    nb += gb;
                    sw += gw;
                    swa += gwa;
                    big = gk > big ? gk : big;
                }
            }
        }
        flush();
    }
}

extern "C" int marex_event_intensity_f32(marex_ctx* ctx, const int32_t* ids, const float* anom, int64_t t0, int64_t Tb,
                                         int64_t C, int n_ev, const int32_t* ev_tmin, const int64_t* ev_off, int64_t n_slots,
                                         const float* w, uint64_t* cnt, double* sums, uint32_t* vmax, uint64_t* status) {
    if (!ctx) return -1;
    if (const int rc = evt_slot_args(ctx, "marex_event_intensity_f32", ids && anom && cnt && sums && vmax && status, ev_tmin, ev_off,
                                     t0, Tb, C, n_ev, n_slots))
        return rc;
    if (const int rc = cell_stream_limits(ctx, "marex_event_intensity_f32", t0, Tb, C)) return rc;
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    LaunchTimer lt(ctx, MAREX_K_MORPH);
    const dim3 grid = slice_grid(Tb, C, INT_CHUNK, INT_TSTRIDE);
    if (w)
        hipLaunchKernelGGL(k_evt_intensity<true>, grid, dim3(256), 0, ctx->stream, ids, anom, (long)t0, (long)Tb, (long)C, n_ev,
                           ev_tmin, (const long long*)ev_off, (long long)n_slots, w, (u64*)cnt, sums, (unsigned*)vmax,
                           (u64*)status);
    else
        hipLaunchKernelGGL(k_evt_intensity<false>, grid, dim3(256), 0, ctx->stream, ids, anom, (long)t0, (long)Tb, (long)C, n_ev,
                           ev_tmin, (const long long*)ev_off, (long long)n_slots, w, (u64*)cnt, sums, (unsigned*)vmax,
                           (u64*)status);
    HIP_TRY(ctx, hipGetLastError());
    return 0;
}
