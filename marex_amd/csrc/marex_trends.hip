// marex_trends.hip -- per-cell trends of a short series of maps y [G][C] over abscissae x [G] (the annual maps of
// local_intensity / cell_events / event_occurrence / compound_events with by="year"): the integers of the Mann-Kendall
// test, the medians and the ordinary-least-squares sums in one launch (k_trend_stats), and exact order statistics of the
// P = n (n - 1) / 2 pairwise slopes of a cell -- the Theil-Sen slope and its confidence bounds -- in another
// (k_trend_select).  The first compute-bound unit of the analysis layer: O(G^2) float64 work per cell on a small input.
//
// Layout: a lane owns one cell, a workgroup is one wave over 64 consecutive cells, so a row of y is read as 512 contiguous
// bytes.  For a short series the wave copies its samples once into an LDS tile [G][64] of doubles (a lane reads back only
// what it wrote itself: no barrier; consecutive lanes, consecutive 8-byte words: no bank conflict), a sample that is not
// finite as NaN; for a long one, where the tiles would leave a compute unit with too few waves to keep its four SIMDs busy
// with divisions, the samples are re-read from y, which the caches hold (G x 512 bytes per wave).  The selection changes
// over above G = 64 (five waves per compute unit), the statistics above G = 128; both were measured.
// The samples are NOT compacted: with every lane at the same pair (i, j), x[j] - x[i] is the same in all lanes, the pair
// loop has no divergence, and a missing sample needs no branch -- a NaN gives a NaN difference and a NaN slope, which no
// comparison counts.  Rows that are missing in the whole wave are skipped, and a wave without a cell of two samples does
// no selection at all.
//
// Selection: the P slopes are never stored.  key(v) = the bits of v with the sign flipped (v >= 0) or all bits flipped
// (v < 0) orders the doubles as unsigned integers; the keys from key(-inf) to key(+inf) are exactly the non-NaN doubles.
// For a rank r the answer is the smallest key m in that range with #{slopes <= value(m)} > r: a bisection of at most 64
// steps, each of which recomputes every quotient once and compares it with the pivots of up to TREND_PIVOTS ranks of the
// cell.  The comparison is the float64 one, under which -0.0 and +0.0 are one value as they are in the slopes (+ 0.0), so
// the count is monotone in the key; the result is normalised the same way.  The loop ends when every interval of the wave
// has closed.
// Arithmetic: every slope is two float64 subtractions, one correctly rounded IEEE division and + 0.0; the sums are
// sequential additions of separately rounded products (-ffp-contract=off).  No reciprocal of x[j] - x[i] is ever used.
#include "marex_common.hip.h"

#define TREND_MAX_STEPS 256
// the largest G whose samples a wave keeps in LDS: k_trend_stats (64 KiB), k_trend_select (32 KiB)
#ifndef TREND_STATS_LDS_STEPS
#define TREND_STATS_LDS_STEPS 128
#endif
#ifndef TREND_SELECT_LDS_STEPS
#define TREND_SELECT_LDS_STEPS 64
#endif
// ranks of a cell that share the quotients of a bisection step
#define TREND_PIVOTS 4
static_assert(TREND_STATS_LDS_STEPS * 512 <= 65536 && TREND_SELECT_LDS_STEPS * 512 <= 65536,
              "the tile is dynamic LDS without an attribute: at most 64 KiB");

__device__ __forceinline__ double nan_d() { return __builtin_nan(""); }
__device__ __forceinline__ double trend_sample(double v) { return fabs(v) <= 1.7976931348623157e308 ? v : nan_d(); }

__device__ __forceinline__ double key_to_double(u64 k) {
    return __longlong_as_double((long long)((k >> 63) ? (k & 0x7FFFFFFFFFFFFFFFull) : ~k));
}
static constexpr u64 KEY_NEG_INF = 0x000FFFFFFFFFFFFFull, KEY_POS_INF = 0xFFF0000000000000ull;

// The samples of the lane's cell: its column of the wave's LDS tile, or y itself.
template <bool LDS>
struct Samples {
    const double* col;  // LDS: tile + lane (stride 64); else y + c (stride C)
    size_t stride;
    bool active;
    __device__ __forceinline__ double operator()(int j) const {
        if constexpr (LDS) return col[(size_t)j * 64];
        return active ? trend_sample(col[(size_t)j * stride]) : nan_d();
    }
};

// Sets up the lane's samples (copies them into the tile for LDS) and returns the number of valid ones.
template <bool LDS>
__device__ __forceinline__ int trend_stage(const double* __restrict__ y, int G, size_t C, size_t c, bool active, double* tile,
                                           Samples<LDS>& sm) {
    const int lane = threadIdx.x;
    int n = 0;
    if constexpr (LDS) {
        for (int j = 0; j < G; ++j) {
            const double v = active ? trend_sample(y[(size_t)j * C + c]) : nan_d();
            tile[(size_t)j * 64 + lane] = v;
            n += v == v;
        }
        sm.col = tile + lane;
        sm.stride = 64;
    } else {
        sm.col = y + (active ? c : 0);
        sm.stride = C;
        for (int j = 0; j < G; ++j) {
            const double v = active ? trend_sample(y[(size_t)j * C + c]) : nan_d();
            n += v == v;
        }
    }
    sm.active = active;
    return n;
}

template <bool LDS>
__global__ void __launch_bounds__(64)
k_trend_stats(const double* __restrict__ y, const double* __restrict__ x, int G, long C, int* __restrict__ n_out,
              int* __restrict__ s_out, int* __restrict__ ties_out, double* __restrict__ med, double* __restrict__ sums) {
    extern __shared__ double tile[];
    const size_t c = (size_t)blockIdx.x * 64 + threadIdx.x;
    const bool active = c < (size_t)C;
    Samples<LDS> sm;
    const int n = trend_stage<LDS>(y, G, (size_t)C, c, active, tile, sm);
    // the means and the median of x: the x at the middle valid positions
    const int rl = (n - 1) / 2, ru = n / 2;  // n == 0: nothing matches below
    double sx = 0.0, sy = 0.0, xl = nan_d(), xu = nan_d();
    int seen = 0;
    for (int j = 0; j < G; ++j) {
        const double v = sm(j), xj = x[j];
        if (v == v) {
            sx = sx + xj;
            sy = sy + v;
            if (seen == rl) xl = xj;
            if (seen == ru) xu = xj;
            ++seen;
        }
    }
    const double xbar = sx / (double)n, ybar = sy / (double)n;  // n == 0: NaN
    double sxx = 0.0, sxy = 0.0, syy = 0.0;
    for (int j = 0; j < G; ++j) {
        const double v = sm(j);
        if (v == v) {
            const double dx = x[j] - xbar, dy = v - ybar;
            sxx = sxx + dx * dx;
            sxy = sxy + dx * dy;
            syy = syy + dy * dy;
        }
    }
    // per sample the valid samples below it and equal to it: S, the tie term and the middle samples of y
    int s = 0, ties = 0;
    double yl = nan_d(), yu = nan_d();
    for (int i = 0; i < G; ++i) {
        const double yi = sm(i);
        if (!__any(yi == yi)) continue;  // wave-uniform
        int lt = 0, eq = 1, after = 0;
        for (int j = 0; j < i; ++j) {
            const double yj = sm(j);
            lt += yj < yi;
            eq += yj == yi;
        }
        for (int j = i + 1; j < G; ++j) {
            const double yj = sm(j);
            lt += yj < yi;
            eq += yj == yi;
            after += (int)(yj > yi) - (int)(yj < yi);
        }
        if (yi == yi) {
            s += after;
            ties += (eq - 1) * (2 * eq + 5);
            if (lt <= rl && rl < lt + eq) yl = yi;
            if (lt <= ru && ru < lt + eq) yu = yi;
        }
    }
    if (active) {
        const size_t Cs = (size_t)C;
        n_out[c] = n;
        s_out[c] = s;
        ties_out[c] = ties;
        med[c] = 0.5 * (yl + yu) + 0.0;
        med[Cs + c] = 0.5 * (xl + xu) + 0.0;
        sums[c] = xbar;
        sums[Cs + c] = ybar;
        sums[2 * Cs + c] = sxx;
        sums[3 * Cs + c] = sxy;
        sums[4 * Cs + c] = syy;
    }
}

template <bool LDS>
__global__ void __launch_bounds__(64)
k_trend_select(const double* __restrict__ y, const double* __restrict__ x, int G, long C, const int* __restrict__ ranks, int K,
               double* __restrict__ out, long long* status) {
    extern __shared__ double tile[];
    const size_t c = (size_t)blockIdx.x * 64 + threadIdx.x, Cs = (size_t)C;
    const bool active = c < Cs;
    Samples<LDS> sm;
    const int n = trend_stage<LDS>(y, G, Cs, c, active, tile, sm);
    const int P = n * (n - 1) / 2;  // at most 32640
    int bad = 0;
    for (int k0 = 0; k0 < K; k0 += TREND_PIVOTS) {  // wave-uniform
        u64 lo[TREND_PIVOTS], hi[TREND_PIVOTS];
        int r[TREND_PIVOTS];
        bool asked[TREND_PIVOTS];
#pragma unroll
        for (int q = 0; q < TREND_PIVOTS; ++q) {
            r[q] = active && k0 + q < K ? ranks[(size_t)(k0 + q) * Cs + c] : -1;
            asked[q] = r[q] >= 0 && r[q] < P;
            lo[q] = KEY_NEG_INF;
            hi[q] = asked[q] ? KEY_POS_INF : KEY_NEG_INF;  // a closed interval takes no part
        }
        for (int step = 0; step < 64; ++step) {
            bool open = false;
            u64 mid[TREND_PIVOTS];
            double pv[TREND_PIVOTS];
            int cnt[TREND_PIVOTS];
#pragma unroll
            for (int q = 0; q < TREND_PIVOTS; ++q) {
                open = open || lo[q] < hi[q];
                mid[q] = lo[q] + ((hi[q] - lo[q]) >> 1);
                pv[q] = key_to_double(mid[q]);
                cnt[q] = 0;
            }
            if (!__any(open)) break;  // wave-uniform
            for (int i = 0; i + 1 < G; ++i) {
                const double yi = sm(i), xi = x[i];
                if (!__any(yi == yi)) continue;  // wave-uniform
#pragma unroll 4
                for (int j = i + 1; j < G; ++j) {
                    const double sl = (sm(j) - yi) / (x[j] - xi) + 0.0;  // NaN where a sample is missing: never counted
#pragma unroll
                    for (int q = 0; q < TREND_PIVOTS; ++q) cnt[q] += sl <= pv[q];
                }
            }
#pragma unroll
            for (int q = 0; q < TREND_PIVOTS; ++q) {
                if (lo[q] < hi[q]) {
                    if (cnt[q] > r[q])
                        hi[q] = mid[q];
                    else
                        lo[q] = mid[q] + 1;
                }
            }
        }
#pragma unroll
        for (int q = 0; q < TREND_PIVOTS; ++q) {
            double v = nan_d();
            if (asked[q]) {
                if (lo[q] == hi[q])
                    v = key_to_double(lo[q]) + 0.0;
                else
                    ++bad;
            }
            if (active && k0 + q < K) out[(size_t)(k0 + q) * Cs + c] = v;
        }
    }
    if (bad) atomicAdd((u64*)status + 1, (u64)bad);
}

static int trend_check(marex_ctx* ctx, const char* name, bool null, int G, int64_t C) {
    if (null || G < 2 || G > TREND_MAX_STEPS || C <= 0)
        return fail(ctx, -1, "%s: null pointer, G outside 2 .. %d, no cells or no ranks", name, TREND_MAX_STEPS);
    if (C >= 2147483647L) return fail(ctx, -4, "%s: 2^31 - 1 or more cells", name);
    return 0;
}

extern "C" int marex_trend_stats_f64(marex_ctx* ctx, const double* y, const double* x, int G, int64_t C, int32_t* n, int32_t* s,
                                     int32_t* ties, double* med, double* sums, int64_t* status) {
    const char* name = "marex_trend_stats_f64";
    if (!ctx) return -1;
    if (const int rc = trend_check(ctx, name, !y || !x || !n || !s || !ties || !med || !sums || !status, G, C)) return rc;
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    LaunchTimer lt(ctx, MAREX_K_MORPH);
    const dim3 grid((unsigned)((C + 63) / 64)), block(64);
    if (G <= TREND_STATS_LDS_STEPS)
        hipLaunchKernelGGL((k_trend_stats<true>), grid, block, (size_t)G * 512, ctx->stream, y, x, G, (long)C, n, s, ties, med, sums);
    else
        hipLaunchKernelGGL((k_trend_stats<false>), grid, block, 0, ctx->stream, y, x, G, (long)C, n, s, ties, med, sums);
    HIP_TRY(ctx, hipGetLastError());
    return 0;
}

extern "C" int marex_trend_select_f64(marex_ctx* ctx, const double* y, const double* x, int G, int64_t C, const int32_t* ranks,
                                      int K, double* out, int64_t* status) {
    const char* name = "marex_trend_select_f64";
    if (!ctx) return -1;
    if (const int rc = trend_check(ctx, name, !y || !x || !ranks || !out || !status || K <= 0, G, C)) return rc;
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    LaunchTimer lt(ctx, MAREX_K_MORPH);
    const dim3 grid((unsigned)((C + 63) / 64)), block(64);
    if (G <= TREND_SELECT_LDS_STEPS)
        hipLaunchKernelGGL((k_trend_select<true>), grid, block, (size_t)G * 512, ctx->stream, y, x, G, (long)C, ranks, K, out,
                           (long long*)status);
    else
        hipLaunchKernelGGL((k_trend_select<false>), grid, block, 0, ctx->stream, y, x, G, (long)C, ranks, K, out,
                           (long long*)status);
    HIP_TRY(ctx, hipGetLastError());
    return 0;
}
