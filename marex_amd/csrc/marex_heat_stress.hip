// marex_heat_stress.hip -- accumulated heat stress of a raw SST field against a fixed per-cell threshold: the monthly mean
// climatology whose maximum is the threshold (MMM), the HotSpot, its running accumulation over `window` steps (the Degree
// Heating Week of NOAA Coral Reef Watch: Liu et al. 2014, Skirving et al. 2020) and the bleaching alert class of every step.
//
// Layout (that of marex_local_intensity.hip at one cell per lane): a lane owns its cell for the whole call and walks the
// rows HS_U at a time, all loads of a batch in flight together.  Everything of a (group, cell) lives in the lane's
// registers: a stretch -- a maximal sequence of rows of one call under one (wave-uniform) group label -- LOADS the stored
// state of (group, cell) when it begins and stores it when it ends.  No register partial is ever added to memory and no
// atomic touches a per-cell output, so a float64 sum is one fixed sequence of additions in ascending step, whatever the
// windows, also for groups that are revisited (months).
//
// The running accumulation has two read streams, row t and row t - window: the step that leaves the window is recomputed
// from x[t - window] and m by the rule that admitted it, so a lane keeps 8 bytes of history (S), not a ring of `window`
// values.  S is exact: a counted HotSpot h is a float32 in [2^-10, 2^10) (hotspot_min >= 2^-10, |d| < 1024), hence a
// multiple of 2^-33 below 2^10; up to 512 of them sum below 2^52 of those units, so every partial sum of every subset of a
// window (at most 366 steps) plus the entering term is a float64, and S += h[t]; S -= h[t - window] never rounds: S[t] is
// the exact real sum whatever the order, a carried S never drifts, and a step that left leaves no residue.
//
// One cell per lane, not four through float4: a row is 256 B per wave and stream already, HS_U rows of both streams are
// 16 loads in flight per lane, and four cells would quadruple the 19 registers of per-cell state.
#include "marex_cellwalk.hip.h"

#ifndef HS_U
#define HS_U 8  // rows loaded together, of either stream
#endif
#define HS_MAXL 6               // alert levels at most
#define HS_NCLS (3 + HS_MAXL)   // alert classes 0 .. 2 + L at most

// Rows t0 .. t0 + Tb - 1 of x [Tb][C]; lab [T] by the global step: -1 skips the step, 0 .. G - 1 selects sum / cnt [G][C].
__global__ void __launch_bounds__(256)
k_group_mean(const float* __restrict__ x, long t0, long Tb, long C, const int* __restrict__ lab, int G, double* sum,
             unsigned* cnt, u64* status) {
    const long c = (long)blockIdx.x * 256 + threadIdx.x;
    const bool active = c < C;
    int cg = lab[t0];
    bool gok = false, dirty = false;
    double sm = 0.0;
    unsigned n = 0, lost = 0;
    auto open = [&]() {
        gok = cg >= 0 && cg < G;  // wave-uniform
        dirty = false;
        sm = 0.0;
        n = 0;
        if (gok && active) {
            const size_t o = (size_t)cg * (size_t)C + c;
            sm = sum[o];
            n = cnt[o];
        }
    };
    auto close = [&]() {
        if (!gok || !active || !dirty) return;
        const size_t o = (size_t)cg * (size_t)C + c;
        sum[o] = sm;
        cnt[o] = n;
    };
    open();
    for (long r = 0; r < Tb; r += HS_U) {
        float v[HS_U];
#pragma unroll
        for (int k = 0; k < HS_U; ++k)
            v[k] = (active && r + k < Tb) ? x[(size_t)(r + k) * (size_t)C + c] : __uint_as_float(0x7FC00000u);
#pragma unroll  // v[k] must stay in registers: no dynamic indexing
        for (int k = 0; k < HS_U; ++k) {
            if (r + k < Tb) {  // wave-uniform
                const int g = lab[t0 + r + k];
                if (g != cg) {
                    close();
                    cg = g;
                    open();
                }
                if (gok) {
                    if (finite_bits(v[k])) {  // a lane past C holds NaN
                        sm += (double)v[k];
                        n += 1;
                        dirty = true;
                    }
                } else if (cg != -1) {
                    lost += active;
                }
            }
        }
    }
    close();
    if (lost) atomicAdd(status, (u64)lost);
}

// x points at row t0 - lead: row t of the field is x[t - t0 + lead].  ACC: the per-(group, cell) accumulators are given.
template <bool ACC>
__global__ void __launch_bounds__(256)
k_heat_stress(const float* __restrict__ x, const float* __restrict__ mmm, long t0, long lead, long Tb, long C, int window,
              float hmin, double spw, const float* __restrict__ levels, int L, const int* __restrict__ grp, int G, double* state,
              unsigned* dmax, int* tmax, unsigned* hmax, unsigned* cls_steps, unsigned* invalid, int* onset, float* dhw,
              unsigned char* alert, u64* status) {
    const long c = (long)blockIdx.x * 256 + threadIdx.x;
    const bool active = c < C;
    const float nanf_ = __uint_as_float(0x7FC00000u);
    const float m = active ? mmm[c] : nanf_;
    const bool mok = finite_bits(m);
    float lev[HS_MAXL];
#pragma unroll
    for (int j = 0; j < HS_MAXL; ++j) lev[j] = j < L ? levels[j] : 0.f;
    const int ncls = 3 + L;
    double S = active ? state[c] : 0.0;
    unsigned dm = 0, hm = 0, ni = 0, cl[HS_NCLS], lost = 0;
    int tm = 0, on[HS_MAXL];
    int cg = (ACC && grp) ? grp[t0] : 0;
    bool gok = false;
    auto open = [&]() {  // a stretch begins: the stored state of (cg, cell) into the registers
        gok = cg >= 0 && cg < G;  // wave-uniform; a label outside 0 .. G - 1 addresses nothing
        dm = hm = ni = 0;
        tm = 0;
#pragma unroll
        for (int q = 0; q < HS_NCLS; ++q) cl[q] = 0;
#pragma unroll
        for (int j = 0; j < HS_MAXL; ++j) on[j] = 0;
        if (ACC && gok && active) {
            const size_t o = (size_t)cg * (size_t)C + c;
            dm = dmax[o];
            tm = tmax[o];
            hm = hmax[o];
            ni = invalid[o];
#pragma unroll
            for (int q = 0; q < HS_NCLS; ++q)
                if (q < ncls) cl[q] = cls_steps[((size_t)cg * ncls + q) * (size_t)C + c];
#pragma unroll
            for (int j = 0; j < HS_MAXL; ++j)
                if (j < L) on[j] = onset[((size_t)cg * L + j) * (size_t)C + c];
        }
    };
    auto close = [&]() {  // the stretch ends: every step touched a counter, so the registers always replace the stored state
        if (!ACC || !gok || !active) return;
        const size_t o = (size_t)cg * (size_t)C + c;
        dmax[o] = dm;
        tmax[o] = tm;
        hmax[o] = hm;
        invalid[o] = ni;
#pragma unroll
        for (int q = 0; q < HS_NCLS; ++q)
            if (q < ncls) cls_steps[((size_t)cg * ncls + q) * (size_t)C + c] = cl[q];
#pragma unroll
        for (int j = 0; j < HS_MAXL; ++j)
            if (j < L) onset[((size_t)cg * L + j) * (size_t)C + c] = on[j];
    };
    // the HotSpot of a sample: d = x - m in float32, counted where the step is valid and d >= hmin
    auto hotspot = [&](float v, float& d, bool& valid) -> float {
        d = v - m;
        valid = mok && finite_bits(v) && fabsf(d) < 1024.f;
        return (valid && d >= hmin) ? d : 0.f;
    };
    if (ACC) open();
    for (long r = 0; r < Tb; r += HS_U) {
        float xin[HS_U], xout[HS_U];
#pragma unroll
        for (int k = 0; k < HS_U; ++k) {
            const bool row = active && r + k < Tb;
            const long t = t0 + r + k;
            xin[k] = row ? x[(size_t)(lead + r + k) * (size_t)C + c] : nanf_;
            // the step that leaves: t - window >= 0 lies at row t - window - t0 + lead >= 0 (lead = min(window, t0))
            xout[k] = (row && t >= window) ? x[(size_t)(lead + r + k - window) * (size_t)C + c] : nanf_;
        }
#pragma unroll  // xin[k], xout[k] must stay in registers: no dynamic indexing
        for (int k = 0; k < HS_U; ++k) {
            if (r + k < Tb) {  // wave-uniform
                const long t = t0 + r + k;
                if (ACC && grp) {
                    const int g = grp[t];
                    if (g != cg) {
                        close();
                        cg = g;
                        open();
                    }
                }
                float d, dl;
                bool valid, vl;
                const float h = hotspot(xin[k], d, valid);
                const float hl = hotspot(xout[k], dl, vl);  // NaN where nothing leaves: 0
                S += (double)h;
                S -= (double)hl;
                const float w = mok ? (float)(S / spw) : nanf_;
                int nlev = 0;
#pragma unroll
                for (int j = 0; j < HS_MAXL; ++j) nlev += (j < L && w >= lev[j]);
                const int a = !valid ? 255 : d <= 0.f ? 0 : d < hmin ? 1 : 2 + nlev;
                if (active) {
                    if (dhw) dhw[(size_t)t * (size_t)C + c] = w;
                    if (alert) alert[(size_t)t * (size_t)C + c] = (unsigned char)a;
                }
                if (ACC) {
                    if (!gok) {
                        lost += active;
                        continue;
                    }
                    if (mok) {
                        const unsigned key = ordered_key(w);
                        if (key > dm) {
                            dm = key;
                            tm = (int)t;
                        }
                    }
                    if (valid) {
                        const unsigned key = ordered_key(d);
                        hm = key > hm ? key : hm;
                    }
                    ni += a == 255;
#pragma unroll
                    for (int q = 0; q < HS_NCLS; ++q) cl[q] += a == q;
#pragma unroll
                    for (int j = 0; j < HS_MAXL; ++j)
                        if (j < L && on[j] == 0 && w >= lev[j]) on[j] = (int)t + 1;
                }
            }
        }
    }
    if (ACC) close();
    if (active) state[c] = S;
    if (lost) atomicAdd(status, (u64)lost);
}

extern "C" int marex_group_mean_f32(marex_ctx* ctx, const float* x, int64_t t0, int64_t Tb, int64_t C, const int32_t* lab, int G,
                                    double* sum, uint32_t* cnt, uint64_t* status) {
    const char* name = "marex_group_mean_f32";
    if (!ctx) return -1;
    if (!x || !lab || !sum || !cnt || !status || t0 < 0 || Tb <= 0 || C <= 0 || G <= 0)
        return fail(ctx, -1, "%s: null pointer, empty shape, negative t0 or no group", name);
    if (const int rc = cell_stream_limits(ctx, name, t0, Tb, C)) return rc;
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    LaunchTimer lt(ctx, MAREX_K_MORPH);
    hipLaunchKernelGGL(k_group_mean, cell_grid<1>(C), dim3(256), 0, ctx->stream, x, (long)t0, (long)Tb, (long)C, lab, G, sum,
                       (unsigned*)cnt, (u64*)status);
    HIP_TRY(ctx, hipGetLastError());
    return 0;
}

extern "C" int marex_heat_stress_f32(marex_ctx* ctx, const float* x, const float* mmm, int64_t t0, int64_t lead, int64_t Tb,
                                     int64_t C, int window, float hotspot_min, double steps_per_week, const float* levels, int L,
                                     const int32_t* grp, int G, double* state, uint32_t* dhw_max, int32_t* tmax,
                                     uint32_t* hotspot_max, uint32_t* alert_steps, uint32_t* invalid, int32_t* onset, float* dhw,
                                     uint8_t* alert, uint64_t* status) {
    const char* name = "marex_heat_stress_f32";
    if (!ctx) return -1;
    const int nacc = (dhw_max != nullptr) + (tmax != nullptr) + (hotspot_max != nullptr) + (alert_steps != nullptr) +
                     (invalid != nullptr) + (onset != nullptr);
    if (!x || !mmm || !state || !status || t0 < 0 || Tb <= 0 || C <= 0 || window < 1 || window > 366 ||
        lead != (t0 < window ? t0 : (int64_t)window) || !(hotspot_min >= 0x1p-10f && hotspot_min < 1024.f) ||
        !(steps_per_week > 0.0) || !(steps_per_week <= 1.7976931348623157e308) || L < 0 || L > HS_MAXL || (L > 0 && !levels) ||
        G <= 0 || (!grp && G != 1) || (nacc != 0 && nacc != 6))
        return fail(ctx, -1, "%s: null pointer, empty shape, negative t0, window outside 1 .. 366, lead other than "
                             "min(window, t0), hotspot_min outside [2^-10, 1024), steps_per_week not positive and finite, more "
                             "than %d levels, no group, or accumulators given in part", name, HS_MAXL);
    if (const int rc = cell_stream_limits(ctx, name, t0, Tb, C)) return rc;
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    LaunchTimer lt(ctx, MAREX_K_MORPH);
    const dim3 grid = cell_grid<1>(C), block(256);
#define HS_GO(ACC)                                                                                                              \
    hipLaunchKernelGGL((k_heat_stress<ACC>), grid, block, 0, ctx->stream, x, mmm, (long)t0, (long)lead, (long)Tb, (long)C, window, \
                       hotspot_min, steps_per_week, levels, L, grp, G, state, (unsigned*)dhw_max, (int*)tmax,                   \
                       (unsigned*)hotspot_max, (unsigned*)alert_steps, (unsigned*)invalid, (int*)onset, dhw,                    \
                       (unsigned char*)alert, (u64*)status)
    if (nacc)
        HS_GO(true);
    else
        HS_GO(false);
#undef HS_GO
    HIP_TRY(ctx, hipGetLastError());
    return 0;
}
