// marex_composites.hip -- lagged composites (superposed-epoch analysis) of a float field around the onsets or the ends of
// the events of a presence field: per cell, time group and lag l = -L .. L the number, the sum and the sum of squares of the
// finite values v[t + l] over the anchors t of the cell (include/marex_hip.h: marex_event_composites_u8).
//
// The work is sparse and anchor-driven, unlike the dense per-cell streams of the sibling units: the presence bytes are
// streamed once, the values are touched only around anchors.
//   Detection: a wave owns 64 consecutive cells, a lane one of them.  The wave walks the rows a .. b - 1, CPS_U at a time
//   with CPS_U + 1 coalesced 64-byte loads in flight (every row is also the neighbour of the next one), and a ballot gives
//   the wave's anchors of a row.
//   Accumulation: wave-cooperative.  For every set bit, in ascending lane order, the wave takes that cell's anchor and its
//   lanes become the lags: lane j < 2 L + 1 reads v[t + j - L][c] where that row lies in the record, tests it with
//   finite_bits and does a plain read-modify-write on sum, sumsq and cnt at [g][c][j] -- contiguous across the lanes, which
//   is why the accumulators are cell-major.  The value and the three accumulators are loaded together: one round trip per
//   anchor.  Lane 0 bumps anchors[g][c].  An anchor costs one wave step instead of 2 L + 1 steps at one active lane.
// Only the owning wave ever touches a cell's accumulators, always lane j for lag j, and it takes its anchors in time order:
// program order alone makes every (group, cell, lag) sum a sequence of float64 additions in ascending anchor step, whatever
// the windows.  No atomic on a per-cell output, no LDS, no barrier; the only atomic is the add to status.
// Arithmetic: sum += (double)v, sumsq += (double)v * (double)v.  The product of two float32 values has at most 48
// significant bits and is exact in float64, so a contracted FMA and a separate multiply and add give the same bits (the
// unit is built without contraction anyway).
#include "marex_cellwalk.hip.h"

// rows whose anchors are found together: CPS_U + 1 byte loads of a lane in flight
#ifndef CPS_U
#define CPS_U 4
#endif
#define CPS_MAX_LAG 30
static_assert(2 * CPS_MAX_LAG + 1 <= 64, "the lags of an anchor are the lanes of one wave");

// x, v [Tr][C]: the rows r0 .. r0 + Tr - 1 of the record of T steps; anchors at the steps a .. b - 1.  END: an anchor is the
// last step of a run (x[t] and not x[t + 1], t < T - 1), else its first (x[t] and not x[t - 1], t > 0).  A neighbour row
// outside the record counts as present, which censors the run that touches the record's edge.  Lanes past the last cell
// stay in the loop (they take part in the ballots and are the lags of other cells' anchors) with nothing present.
template <bool END>
__global__ void __launch_bounds__(256)
k_event_composites(const unsigned char* __restrict__ x, const float* __restrict__ v, long r0, long Tr, long a, long b, long T,
                   long C, int L, const int* __restrict__ grp, int G, unsigned* anchors, double* sum, double* sumsq,
                   unsigned* cnt, u64* status) {
    const int lane = threadIdx.x & 63;
    const long cbase = ((long)blockIdx.x * 4 + (threadIdx.x >> 6)) * 64;  // wave-uniform
    if (cbase >= C) return;                                               // the whole wave
    const long c = cbase + lane;
    const bool active = c < C;
    const int W = 2 * L + 1;
    const long rend = r0 + Tr;
    for (long t = a; t < b; t += CPS_U) {
        // w[k]: row t - 1 + k (onset) or t + k (end)
        const long first = END ? t : t - 1;
        unsigned char w[CPS_U + 1];
#pragma unroll
        for (int k = 0; k <= CPS_U; ++k) {
            const long row = first + k;
            const bool in = row >= r0 && row < rend && row < b + 1;  // wave-uniform; never past the rows given
            w[k] = in ? (active ? x[(size_t)(row - r0) * (size_t)C + c] : (unsigned char)0) : (unsigned char)1;
        }
#pragma unroll  // w[k] must stay in registers: no dynamic indexing
        for (int k = 0; k < CPS_U; ++k) {
            const long tk = t + k;
            if (tk >= b) break;  // wave-uniform
            const bool here = (END ? w[k] : w[k + 1]) != 0, beside = (END ? w[k + 1] : w[k]) != 0;
            u64 m = __ballot(active && here && !beside);
            if (!m) continue;
            const int g = grp ? grp[tk] : 0;
            if (g < 0 || g >= G) {  // a label outside 0 .. G - 1 addresses nothing
                if (lane == 0) atomicAdd(status, (u64)__popcll(m));
                continue;
            }
            const long lo = tk - L;  // the step of lag -L
            while (m) {              // wave-uniform: the anchors of this row in ascending cell order
                const int src = __ffsll((long long)m) - 1;
                m &= m - 1;
                const long cc = cbase + src;
                const size_t cell = (size_t)g * (size_t)C + (size_t)cc;
                const size_t at = cell * (size_t)W + (size_t)lane;
                const long tt = lo + lane;
                if (lane < W && tt >= 0 && tt < T) {  // rows inside the record are rows given: the entry point checks
                    const float val = v[(size_t)(tt - r0) * (size_t)C + (size_t)cc];
                    const double s = sum[at], q = sumsq[at];
                    const unsigned n = cnt[at];
                    if (finite_bits(val)) {
                        const double d = (double)val;
                        sum[at] = s + d;
                        sumsq[at] = q + d * d;  // exact product: see the head of the file
                        cnt[at] = n + 1u;
                    }
                }
                if (lane == 0) anchors[cell] += 1u;
            }
        }
    }
}

extern "C" int marex_event_composites_u8(marex_ctx* ctx, const uint8_t* x, const float* v, int64_t r0, int64_t Tr, int64_t a,
                                         int64_t b, int64_t T, int64_t C, int max_lag, int anchor, const int32_t* grp, int G,
                                         uint32_t* anchors, double* sum, double* sumsq, uint32_t* cnt, uint64_t* status) {
    const char* name = "marex_event_composites_u8";
    if (!ctx) return -1;
    if (!x || !v || !anchors || !sum || !sumsq || !cnt || !status || C <= 0 || G <= 0 || (!grp && G != 1))
        return fail(ctx, -1, "%s: null pointer, empty row, no group, or labels missing with G != 1", name);
    if (max_lag < 0 || max_lag > CPS_MAX_LAG || anchor < 0 || anchor > 1)
        return fail(ctx, -1, "%s: max_lag must lie in 0 .. %d and anchor in 0 .. 1", name, CPS_MAX_LAG);
    if (r0 < 0 || Tr < 0 || r0 > T || Tr > T - r0 || a < 0 || a > b || b > T)
        return fail(ctx, -1, "%s: needs 0 <= r0, r0 + Tr <= T and 0 <= a <= b <= T", name);
    if ((((uintptr_t)v | (uintptr_t)grp | (uintptr_t)anchors | (uintptr_t)cnt) & 3) != 0 ||
        (((uintptr_t)sum | (uintptr_t)sumsq | (uintptr_t)status) & 7) != 0)
        return fail(ctx, -1, "%s: a pointer is not aligned to its element", name);
    if (const int rc = cell_stream_limits(ctx, name, 0, T, C)) return rc;
    if (a == b) return 0;
    const int64_t H = max_lag > 1 ? max_lag : 1;
    const int64_t need_lo = a - H > 0 ? a - H : 0, need_hi = b + H < T ? b + H : T;
    if (r0 > need_lo || r0 + Tr < need_hi)
        return fail(ctx, -1, "%s: the rows %lld .. %lld do not cover the halo %lld .. %lld of the steps %lld .. %lld", name,
                    (long long)r0, (long long)(r0 + Tr - 1), (long long)need_lo, (long long)(need_hi - 1), (long long)a,
                    (long long)(b - 1));
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    LaunchTimer lt(ctx, MAREX_K_MORPH);
    const dim3 grid((unsigned)((C + 255) / 256)), block(256);
    if (anchor)
        hipLaunchKernelGGL((k_event_composites<true>), grid, block, 0, ctx->stream, x, v, (long)r0, (long)Tr, (long)a, (long)b,
                           (long)T, (long)C, max_lag, grp, G, (unsigned*)anchors, sum, sumsq, (unsigned*)cnt, (u64*)status);
    else
        hipLaunchKernelGGL((k_event_composites<false>), grid, block, 0, ctx->stream, x, v, (long)r0, (long)Tr, (long)a, (long)b,
                           (long)T, (long)C, max_lag, grp, G, (unsigned*)anchors, sum, sumsq, (unsigned*)cnt, (u64*)status);
    HIP_TRY(ctx, hipGetLastError());
    return 0;
}
