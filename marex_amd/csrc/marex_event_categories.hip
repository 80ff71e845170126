// marex_event_categories.hip -- severity categories of tracked events (Hobday et al. 2018): the tracked ID field joined with
// the anomaly field and the day-of-year thresholds, per (timestep, event) the cells of every class and their area, and the
// category map of every step.  One streaming pass of the shape of k_evt_intensity (marex_intensity.hip) over three read-only
// inputs: the int32 event IDs, the float32 anomalies, fetched only under the cells of an event, and the float32 thresholds
// (and weights), fetched only under the cells of an event whose anomaly is finite.
//
// Arithmetic contract: the counts and the field are exact and independent of any order.  The float64 areas are atomic adds
// of exact terms ((double)w of a float32): bit for bit reproducible whenever the partial sums are exactly representable,
// otherwise within 2 n u sum w (n cells of the slot and class, u = 2^-53) of the exact sum -- the contract of sums of
// marex_event_intensity_f32.  The class of a cell is the rule of marex_local_intensity_*: float32 products, one rounding
// each (compiled with -ffp-contract=off).
#include "marex_common.hip.h"

#define CAT_ITERS 16                  // 64-cell pieces per wave
#define CAT_BATCH 4                   // pieces loaded together (loads in flight per lane); CAT_ITERS is a multiple
#define CAT_CHUNK (256 * CAT_ITERS)   // cells of a row per workgroup (4 waves)
#define CAT_TSTRIDE 64                // rows in flight: a workgroup walks every CAT_TSTRIDE-th row
#define CAT_NCNT 7                    // below, moderate, strong, severe, extreme, undefined, non-finite anomaly
#define CAT_NAREA 6                   // the classified ones

// Rows t0 .. t0 + Tb - 1 of the field: ids / anom [Tb][C]; a cell of event e = ids[row][c] in 1 .. n_ev at the global step
// t = t0 + row belongs to the slot s = ev_off[e] + t - ev_tmin[e].  A wave walks CAT_ITERS consecutive 64-cell pieces of a
// row, CAT_BATCH at a time: the IDs of the batch are loaded first, the anomalies only by the lanes whose ID is an event, the
// thresholds of the row's day of the year (and the weights) only by those of them whose anomaly is finite.  The lanes of a
// piece are grouped by event (ballot); the cells of a group per class are the popcounts of its class ballots, the weighted
// sums wave reductions that run only for a class with a lane.  The run of an event is carried across its pieces in uniform
// registers -- its slot is resolved and range-checked once, where the run begins -- and flushed when the event changes:
// lane q adds the count (and the area) of class q, where it is not zero.  A run outside the event's declared span adds its
// cells to status[0] instead; under a row whose doy label is outside 0 .. n_doy - 1 the event cells add to status[1] and to
// nothing else.  field (the whole [T][C] output, addressed by t) gets one plain byte store per cell of the rows walked.
// Nothing is zeroed here: the accumulators continue over time blocks.
template <bool WEIGHTED, bool FIELD>
__global__ void __launch_bounds__(256)
k_evt_categories(const int* __restrict__ ids, const float* __restrict__ anom, long t0, long Tb, long C, int n_ev,
                 const int* __restrict__ ev_tmin, const long long* __restrict__ ev_off, long long n_slots,
                 const float* __restrict__ thr, const int* __restrict__ doy, int n_doy, const float* __restrict__ w,
                 u64* __restrict__ cnt, double* __restrict__ area, unsigned char* __restrict__ field,
                 u64* __restrict__ status) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const long rw = (long)blockIdx.x * CAT_CHUNK + (long)wave * (64 * CAT_ITERS);
    for (long row = blockIdx.y; row < Tb; row += gridDim.y) {
        const int* irow = ids + row * C;
        const float* arow = anom + row * C;
        const long long t = t0 + row;
        unsigned char* frow = FIELD ? field + (size_t)t * (size_t)C : nullptr;
        const int d = doy[t];
        if (d < 0 || d >= n_doy) {  // wave-uniform: no row of thr belongs to this step
            long long lost = 0;
#pragma unroll 1
            for (int b = 0; b < CAT_ITERS; ++b) {
                if (rw + 64 * b >= C) break;
                const long r = rw + 64 * b + lane;
                const int v = r < C ? irow[r] : 0;
                lost += __popcll(__ballot(v > 0 && v <= n_ev));
                if (FIELD && r < C) frow[r] = 0;
            }
            if (lost && lane == 0) atomicAdd(status + 1, (u64)lost);
            continue;
        }
        const float* hrow = thr + (size_t)d * (size_t)C;
        int cur = 0;
        long long slot = -1;
        unsigned n[CAT_NCNT];
        double ar[CAT_NAREA];
#pragma unroll
        for (int q = 0; q < CAT_NCNT; ++q) n[q] = 0;
#pragma unroll
        for (int q = 0; q < CAT_NAREA; ++q) ar[q] = 0;
        auto flush = [&]() {
            if (cur <= 0) return;  // wave-uniform
            unsigned mine = 0, all = 0;
            double am = 0;
#pragma unroll
            for (int q = 0; q < CAT_NCNT; ++q) {
                all += n[q];
                if (lane == q) mine = n[q];
            }
            if (slot < 0) {  // outside the declared span: counted, not accumulated
                if (lane == 0 && all) atomicAdd(status, (u64)all);
                return;
            }
            if (WEIGHTED) {
#pragma unroll
                for (int q = 0; q < CAT_NAREA; ++q)
                    if (lane == q) am = ar[q];
            }
            if (lane < CAT_NCNT && mine) {
                atomicAdd(cnt + (size_t)slot * CAT_NCNT + lane, (u64)mine);
                if (WEIGHTED && lane < CAT_NAREA) atomicAdd(area + (size_t)slot * CAT_NAREA + lane, am);
            }
        };
#pragma unroll 1
        for (int b = 0; b < CAT_ITERS; b += CAT_BATCH) {
            if (rw + 64 * b >= C) break;  // wave-uniform
            int ev[CAT_BATCH], cl[CAT_BATCH];
            float av[CAT_BATCH], hv[CAT_BATCH], wv[CAT_BATCH];
#pragma unroll
            for (int k = 0; k < CAT_BATCH; ++k) {
                const long r = rw + 64 * (b + k) + lane;
                const int v = r < C ? irow[r] : 0;
                ev[k] = (v > 0 && v <= n_ev) ? v : 0;  // ev_tmin / ev_off are never indexed by an unchecked value
            }
#pragma unroll
            for (int k = 0; k < CAT_BATCH; ++k) {
                const long r = rw + 64 * (b + k) + lane;  // ev[k] > 0 implies r < C
                av[k] = ev[k] > 0 ? arow[r] : 0.f;
            }
#pragma unroll
            for (int k = 0; k < CAT_BATCH; ++k) {
                const long r = rw + 64 * (b + k) + lane;
                const bool fin = ev[k] > 0 && finite_bits(av[k]);
                hv[k] = fin ? hrow[r] : 0.f;
                wv[k] = (WEIGHTED && fin) ? w[r] : 0.f;
                cl[k] = fin ? 0 : 6;
            }
#pragma unroll  // ev[k], av[k], hv[k], wv[k] must stay in registers: no dynamic indexing
            for (int k = 0; k < CAT_BATCH; ++k) {
                const int e = ev[k];
                u64 todo = __ballot(e > 0);
                unsigned char fv = 0;
                if (todo) {
                    const int c = cl[k] ? 6 : severity_class(av[k], hv[k]);
                    while (todo) {
                        const int lead = __ffsll((long long)todo) - 1;
                        const int el = __shfl(e, lead, 64);
                        const u64 same = __ballot(e == el) & todo;
                        todo &= ~same;
                        if (el != cur) {
                            flush();
                            cur = el;
#pragma unroll
                            for (int q = 0; q < CAT_NCNT; ++q) n[q] = 0;
#pragma unroll
                            for (int q = 0; q < CAT_NAREA; ++q) ar[q] = 0;
                            const int tm = ev_tmin[el];
                            const long long o0 = ev_off[el], o1 = ev_off[el + 1];
                            const long long s = o0 + (t - tm);
                            slot = (t < tm || o0 < 0 || s >= o1 || s >= n_slots) ? -1 : s;
                        }
                        const bool me = (same >> lane) & 1ull;
#pragma unroll
                        for (int q = 0; q < CAT_NCNT; ++q) {
                            const u64 bq = __ballot(me && c == q);
                            if (!bq) continue;  // wave-uniform
                            n[q] += (unsigned)__popcll(bq);
                            if (WEIGHTED && q < CAT_NAREA) ar[q] += wave_sum((me && c == q) ? (double)wv[k] : 0.0);
                        }
                        if (FIELD && me) fv = slot >= 0 ? (unsigned char)(c + 1) : (unsigned char)0;
                    }
                }
                if (FIELD) {
                    const long r = rw + 64 * (b + k) + lane;
                    if (r < C) frow[r] = fv;
                }
            }
        }
        flush();
    }
}

extern "C" int marex_event_categories_f32(marex_ctx* ctx, const int32_t* ids, const float* anom, int64_t t0, int64_t Tb,
                                          int64_t C, int n_ev, const int32_t* ev_tmin, const int64_t* ev_off, int64_t n_slots,
                                          const float* thr, const int32_t* doy, int n_doy, const float* w, uint64_t* cat_cnt,
                                          double* cat_area, uint8_t* field, uint64_t* status) {
    if (!ctx) return -1;
    if (const int rc = evt_slot_args(ctx, "marex_event_categories_f32", ids && anom && cat_cnt && status, ev_tmin, ev_off, t0, Tb, C,
                                     n_ev, n_slots))
        return rc;
    if (!thr || !doy || n_doy <= 0 || (w == nullptr) != (cat_area == nullptr))
        return fail(ctx, -1, "marex_event_categories_f32: thr or doy missing, n_doy <= 0, or w and cat_area given in part");
    if (const int rc = cell_stream_limits(ctx, "marex_event_categories_f32", t0, Tb, C)) return rc;
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    LaunchTimer lt(ctx, MAREX_K_MORPH);
    const dim3 grid = slice_grid(Tb, C, CAT_CHUNK, CAT_TSTRIDE);
#define CAT_LAUNCH(WT, FD)                                                                                                  \
    hipLaunchKernelGGL((k_evt_categories<WT, FD>), grid, dim3(256), 0, ctx->stream, ids, anom, (long)t0, (long)Tb, (long)C,  \
                       n_ev, ev_tmin, (const long long*)ev_off, (long long)n_slots, thr, doy, n_doy, w, (u64*)cat_cnt,       \
                       cat_area, (unsigned char*)field, (u64*)status)
    if (w && field)
        CAT_LAUNCH(true, true);
    else if (w)
        CAT_LAUNCH(true, false);
    else if (field)
        CAT_LAUNCH(false, true);
    else
        CAT_LAUNCH(false, false);
#undef CAT_LAUNCH
    HIP_TRY(ctx, hipGetLastError());
    return 0;
}
