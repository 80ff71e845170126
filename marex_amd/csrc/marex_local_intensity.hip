// marex_local_intensity.hip -- per-cell intensity of extremes: an event mask or a tracked ID field joined with the anomaly
// field and, optionally, the day-of-year thresholds (the notebooks' dat_anomaly.where(extreme_events)
// .groupby("time.year") sum / mean / max / idxmax, and the Hobday severity categories as multiples of the threshold).  One
// streaming pass: the presence field is read once, the anomalies and thresholds only under present cells.
//
// Layout (that of marex_occurrence.hip): a lane owns its cells for the whole call -- one cell, or four consecutive uint8
// cells through one 32-bit load -- and walks the rows LI_U1 / LI_U4 at a time: the presence words of the batch first, then
// the anomalies (and thresholds) of its present cells, all in flight together.  Everything of a (group, cell) lives in the
// lane's registers.  A stretch is a maximal sequence of rows of one call under one (wave-uniform) group label: when it
// begins the lane LOADS days, invalid, sum, vmax, tmax and the category counters of (group, cell), it adds one term per
// step, and it stores them when the stretch ends, if a present step touched them.  No register partial is ever added to
// memory, so sum[g][c] is one fixed sequence of float64 additions in ascending time: bit-identical to a row-by-row loop,
// equal from run to run, independent of the windows, also for groups that are revisited.  No atomic touches a per-cell
// output.  The section counts use occurrence's scheme: the wave's class partition is taken once, per row one ballot per
// category, popcount(ballot & lane mask), one integer atomicAdd per (class, category) when the section label changes.
#include "marex_cellwalk.hip.h"

// rows loaded together of the one-cell and of the four-cell layout
#ifndef LI_U1
#define LI_U1 8
#endif
#ifndef LI_U4
#define LI_U4 4
#endif
#define LI_NCAT 6  // below, moderate, strong, severe, extreme, undefined (severity_class)

// Rows t0 .. t0 + Tb - 1: x and anom [Tb][C].  V: cells per lane (4: C % 4 == 0 and x is 4-byte aligned -- the entry point
// checks); CATS: thr, doy and cat_days are given; SECT (only with CATS): sec_cnt, sgrp and cls are given.  Lanes past the
// last cell stay in the loop (they take part in the ballots) with nothing present.
template <typename T, int V, bool CATS, bool SECT>
__global__ void __launch_bounds__(256)
k_local_intensity(const T* __restrict__ x, const float* __restrict__ anom, long t0, long Tb, long C, int match,
                  const int* __restrict__ grp, int G, const float* __restrict__ thr, const int* __restrict__ doy, int n_doy,
                  const int* __restrict__ sgrp, int G2, const int* __restrict__ cls, int R, unsigned* days, unsigned* invalid,
                  double* sum, unsigned* vmax, int* tmax, unsigned* cat_days, u64* sec_cnt, u64* status) {
    typedef typename cell_word<T, V>::type W;
    constexpr bool SIGNED = std::is_same<T, int>::value;
    constexpr int U = V == 4 ? LI_U4 : LI_U1;
    constexpr int NC = CATS ? LI_NCAT : 1, NS = SECT ? LI_NCAT : 1;
    const int lane = threadIdx.x & 63;
    const long c0 = ((long)blockIdx.x * 256 + threadIdx.x) * V;
    const bool active = c0 < C;  // V == 4: C % 4 == 0, so all four cells exist
    unsigned nd[V], ni[V], vm[V], cat[V][NC];
    double sm[V];
    int tm[V];
    bool dirty[V];
    u64 smask[V], scnt[V][NS];
    int scls[V];
    unsigned neg = 0, lost = 0;
#pragma unroll
    for (int j = 0; j < V; ++j) {
        smask[j] = 0;
        scls[j] = 0;
#pragma unroll
        for (int q = 0; q < NS; ++q) scnt[j][q] = 0;
        if (SECT) {  // the wave's distinct classes among the sub-cells j: the k-th goes to lane k
            const int cj = active ? cls[c0 + j] : -1;
            wave_class_partition(cj, R, lane, smask[j], scls[j]);
        }
    }
    int cg = grp ? grp[t0] : 0;
    int csg = SECT ? sgrp[t0] : 0;
    bool gok = false;
    auto open = [&]() {  // a stretch begins: the stored state of (cg, cell) into the registers
        gok = cg >= 0 && cg < G;  // wave-uniform; a label outside 0 .. G - 1 addresses nothing
#pragma unroll
        for (int j = 0; j < V; ++j) {
            dirty[j] = false;
            nd[j] = ni[j] = vm[j] = 0;
            sm[j] = 0.0;
            tm[j] = 0;
#pragma unroll
            for (int q = 0; q < NC; ++q) cat[j][q] = 0;
            if (gok && active) {
                const size_t o = (size_t)cg * (size_t)C + c0 + j;
                nd[j] = days[o];
                ni[j] = invalid[o];
                sm[j] = sum[o];
                vm[j] = vmax[o];
                tm[j] = tmax[o];
                if (CATS) {
#pragma unroll
                    for (int q = 0; q < NC; ++q) cat[j][q] = cat_days[((size_t)cg * LI_NCAT + q) * (size_t)C + c0 + j];
                }
            }
        }
    };
    auto close = [&]() {  // the stretch ends: the registers replace the stored state where a present step touched them
        if (!gok || !active) return;
#pragma unroll
        for (int j = 0; j < V; ++j) {
            if (!dirty[j]) continue;
            const size_t o = (size_t)cg * (size_t)C + c0 + j;
            days[o] = nd[j];
            invalid[o] = ni[j];
            sum[o] = sm[j];
            vmax[o] = vm[j];
            tmax[o] = tm[j];
            if (CATS) {
#pragma unroll
                for (int q = 0; q < NC; ++q) cat_days[((size_t)cg * LI_NCAT + q) * (size_t)C + c0 + j] = cat[j][q];
            }
        }
    };
    auto flush_s = [&]() {
        const bool ok = csg >= 0 && csg < G2;  // wave-uniform
#pragma unroll
        for (int j = 0; j < V; ++j) {
#pragma unroll
            for (int q = 0; q < NS; ++q) {
                if (scnt[j][q])
                    atomicAdd(ok ? sec_cnt + ((size_t)csg * (size_t)R + scls[j]) * LI_NCAT + q : status + 1, scnt[j][q]);
                scnt[j][q] = 0;
            }
        }
    };
    open();
    for (long r = 0; r < Tb; r += U) {
        W w[U];
        float av[U][V], hv[U][V];
        int dk[U];
#pragma unroll
        for (int k = 0; k < U; ++k)
            w[k] = (active && r + k < Tb) ? *(const W*)(x + (size_t)(r + k) * (size_t)C + c0) : (W)0;
#pragma unroll
        for (int k = 0; k < U; ++k) {
            dk[k] = (CATS && r + k < Tb) ? doy[t0 + r + k] : 0;  // wave-uniform
            const bool dok = dk[k] >= 0 && dk[k] < n_doy;
#pragma unroll
            for (int j = 0; j < V; ++j) {
                const int v = cell_value<V>(w[k], j);
                const bool p = cell_present(v, match);  // a row past Tb or a lane past C holds 0: never present
                av[k][j] = p ? anom[(size_t)(r + k) * (size_t)C + c0 + j] : 0.f;
                hv[k][j] = (CATS && p && dok) ? thr[(size_t)dk[k] * (size_t)C + c0 + j] : 0.f;
            }
        }
#pragma unroll  // w[k], av[k], hv[k] must stay in registers: no dynamic indexing
        for (int k = 0; k < U; ++k) {
            if (r + k < Tb) {  // wave-uniform
                const long t = t0 + r + k;
                const int g = grp ? grp[t] : 0;
                if (g != cg) {
                    close();
                    cg = g;
                    open();
                }
                if (SECT) {
                    const int sg = sgrp[t];
                    if (sg != csg) {
                        flush_s();
                        csg = sg;
                    }
                }
                const bool row_ok = gok && (!CATS || (dk[k] >= 0 && dk[k] < n_doy));  // wave-uniform
#pragma unroll
                for (int j = 0; j < V; ++j) {
                    const int v = cell_value<V>(w[k], j);
                    const bool p = cell_present(v, match);
                    if (SIGNED) neg += v < 0;
                    if (!row_ok) {  // the step addresses nothing: its present cells are counted
                        lost += p;
                        continue;
                    }
                    const float a = av[k][j];
                    const bool ok = p && finite_bits(a);
                    dirty[j] = dirty[j] || p;
                    nd[j] += ok;
                    ni[j] += p && !ok;
                    if (ok) {
                        sm[j] += (double)a;
                        const unsigned key = ordered_key(a);
                        if (key > vm[j]) {
                            vm[j] = key;
                            tm[j] = (int)t;
                        }
                    }
                    if (CATS) {
                        const int c = ok ? severity_class(a, hv[k][j]) : -1;
#pragma unroll
                        for (int q = 0; q < NC; ++q) {
                            cat[j][q] += c == q;
                            if (SECT) scnt[j][q] += __popcll(__ballot(c == q) & smask[j]);
                        }
                    }
                }
            }
        }
    }
    close();
    if (SECT) flush_s();
    if (lost) atomicAdd(status + 1, (u64)lost);
    if (SIGNED && neg) atomicAdd(status, (u64)neg);
}

template <typename T, int V>
static void li_launch(marex_ctx* ctx, const T* x, const float* anom, long t0, long Tb, long C, int match, const int* grp, int G,
                      const float* thr, const int* doy, int n_doy, const int* sgrp, int G2, const int* cls, int R, unsigned* days,
                      unsigned* invalid, double* sum, unsigned* vmax, int* tmax, unsigned* cat_days, u64* sec_cnt, u64* status) {
    const dim3 grid = cell_grid<V>(C), block(256);
#define LI_GO(CATS, SECT)                                                                                                    \
    hipLaunchKernelGGL((k_local_intensity<T, V, CATS, SECT>), grid, block, 0, ctx->stream, x, anom, t0, Tb, C, match, grp, G, \
                       thr, doy, n_doy, sgrp, G2, cls, R, days, invalid, sum, vmax, tmax, cat_days, sec_cnt, status)
    if constexpr (V == 1) {  // the category builds exist at one cell per lane only
        if (sec_cnt)
            LI_GO(true, true);
        else if (thr)
            LI_GO(true, false);
        else
            LI_GO(false, false);
    } else {
        LI_GO(false, false);
    }
#undef LI_GO
}

template <typename T>
static int li_entry(marex_ctx* ctx, const char* name, const T* x, const float* anom, int64_t t0, int64_t Tb, int64_t C, int match,
                    const int32_t* grp, int G, const float* thr, const int32_t* doy, int n_doy, const int32_t* sgrp, int G2,
                    const int32_t* cls, int R, uint32_t* days, uint32_t* invalid, double* sum, uint32_t* vmax, int32_t* tmax,
                    uint32_t* cat_days, uint64_t* sec_cnt, uint64_t* status) {
    if (!ctx) return -1;
    const int ncat = (thr != nullptr) + (doy != nullptr) + (cat_days != nullptr);
    const int nsec = (sec_cnt != nullptr) + (sgrp != nullptr) + (cls != nullptr);
    if (!x || !anom || !days || !invalid || !sum || !vmax || !tmax || !status || t0 < 0 || Tb <= 0 || C <= 0 || match < 0 ||
        G <= 0 || (!grp && G != 1) || (ncat != 0 && ncat != 3) || (ncat == 3 && n_doy <= 0) || (nsec != 0 && nsec != 3) ||
        (nsec == 3 && (G2 <= 0 || R <= 0 || ncat != 3)))
        return fail(ctx, -1, "%s: null pointer, empty shape, negative match, no group, category or section arguments given in "
                             "part, or sections without thresholds", name);
    if (const int rc = cell_stream_limits(ctx, name, t0, Tb, C)) return rc;
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    LaunchTimer lt(ctx, MAREX_K_MORPH);
    // four cells per lane without categories; the category builds run one cell per lane (register budget: DESIGN.md section 4)
    const bool quad = sizeof(T) == 1 && !thr && C % 4 == 0 && ((uintptr_t)x & 3) == 0;
    if (sizeof(T) == 1 && quad)
        li_launch<unsigned char, 4>(ctx, (const unsigned char*)x, anom, (long)t0, (long)Tb, (long)C, match, grp, G, thr, doy, n_doy,
                                    sgrp, G2, cls, R, (unsigned*)days, (unsigned*)invalid, sum, (unsigned*)vmax, (int*)tmax,
                                    (unsigned*)cat_days, (u64*)sec_cnt, (u64*)status);
    else
        li_launch<T, 1>(ctx, x, anom, (long)t0, (long)Tb, (long)C, match, grp, G, thr, doy, n_doy, sgrp, G2, cls, R,
                        (unsigned*)days, (unsigned*)invalid, sum, (unsigned*)vmax, (int*)tmax, (unsigned*)cat_days,
                        (u64*)sec_cnt, (u64*)status);
    HIP_TRY(ctx, hipGetLastError());
    return 0;
}

#define LI_EXPORT(SFX, XT, T)  /* marex_local_intensity_u8, marex_local_intensity_i32 */                                           \
    extern "C" int marex_local_intensity_##SFX(                                                                                    \
        marex_ctx* ctx, const XT* x, const float* anom, int64_t t0, int64_t Tb, int64_t C, int match, const int32_t* grp, int G,   \
        const float* thr, const int32_t* doy, int n_doy, const int32_t* sgrp, int G2, const int32_t* cls, int R, uint32_t* days,   \
        uint32_t* invalid, double* sum, uint32_t* vmax, int32_t* tmax, uint32_t* cat_days, uint64_t* sec_cnt, uint64_t* status) {  \
        return li_entry<T>(ctx, "marex_local_intensity_" #SFX, (const T*)x, anom, t0, Tb, C, match, grp, G, thr, doy, n_doy, sgrp, \
                           G2, cls, R, days, invalid, sum, vmax, tmax, cat_days, sec_cnt, status);                                 \
    }
LI_EXPORT(u8, uint8_t, unsigned char)
LI_EXPORT(i32, int32_t, int)
