// marex_occurrence.hip -- occurrence statistics of an event mask or a tracked ID field: per-cell counts by time group
// (the notebooks' (ID_field > 0).mean("time") and .groupby("time.season").mean("time"), (ID_field == id).sum("time")),
// per-cell run statistics, and counts per (time group, spatial class) ((ID_field > 0).mean("lon").resample(time="ME")
// .mean(), groupby_bins(lat, bins).mean("ncells")).  One streaming pass: the field is read once, nothing else of its size
// is touched.
//
// Layout: a lane owns its cells for the whole call -- one cell, or four consecutive uint8 cells through one 32-bit load --
// and walks the rows with OCC_U1 / OCC_U4 independent loads in flight.  Everything of a cell lives in the lane's
// registers: the open run, the runs begun, the longest run and the counter of the current time group, which is added to cell_cnt by a
// plain read-modify-write of the owning lane when the (wave-uniform) group label changes.  No atomic touches a per-cell
// output.  For the section counts the lanes of a wave fall into the same classes at every row, so the partition is taken
// once before the time loop: lane k keeps the 64-bit lane mask and the class of the wave's k-th distinct class (per
// sub-cell of the four-cell layout), adds popcount(ballot(present) & mask) per row, and issues one integer atomicAdd per
// class when the section label changes -- no per-lane atomic on a shared address inside the row loop.
// All results are integers: exact, and independent of any order and of how the rows are cut into calls.
#include "marex_cellwalk.hip.h"

// rows loaded together (loads in flight per lane) of the one-cell and of the four-cell layout
#ifndef OCC_U1
#define OCC_U1 8
#endif
#ifndef OCC_U4
#define OCC_U4 16
#endif

// Rows t0 .. t0 + Tb - 1 of the field: x [Tb][C].  T: int or unsigned char; V: cells per lane (4: C % 4 == 0 and x, cell_cnt
// and run_state are aligned for the vector accesses -- the entry point checks); RUNS: run_state is given; SECT: sec_cnt,
// sgrp and cls are given.  Lanes past the last cell stay in the loop (they take part in the ballots) with nothing present.
template <typename T, int V, bool RUNS, bool SECT>
__global__ void __launch_bounds__(256)
k_occurrence(const T* __restrict__ x, long t0, long Tb, long C, int match, const int* __restrict__ grp, int G,
             const int* __restrict__ sgrp, int G2, const int* __restrict__ cls, int R, unsigned* run_state, unsigned* cell_cnt,
             u64* sec_cnt, u64* status) {
    typedef typename cell_word<T, V>::type W;
    constexpr bool SIGNED = std::is_same<T, int>::value;
    constexpr int OCC_U = V == 4 ? OCC_U4 : OCC_U1;
    const int lane = threadIdx.x & 63;
    const long c0 = ((long)blockIdx.x * 256 + threadIdx.x) * V;
    const bool active = c0 < C;  // V == 4: C % 4 == 0, so all four cells exist
    unsigned run[V], nrun[V], lng[V], gcnt[V];
    u64 smask[V], scnt[V];
    int scls[V];
    unsigned neg = 0;
#pragma unroll
    for (int j = 0; j < V; ++j) {
        run[j] = nrun[j] = lng[j] = gcnt[j] = 0;
        smask[j] = scnt[j] = 0;
        scls[j] = 0;
        if (RUNS && active) {
            run[j] = run_state[c0 + j];
            nrun[j] = run_state[(size_t)C + c0 + j];
            lng[j] = run_state[2 * (size_t)C + c0 + j];
        }
        if (SECT) {  // the wave's distinct classes among the sub-cells j: the k-th goes to lane k
            const int cj = active ? cls[c0 + j] : -1;
            wave_class_partition(cj, R, lane, smask[j], scls[j]);
        }
    }
    int cg = grp ? grp[t0] : 0;
    int csg = SECT ? sgrp[t0] : 0;
    auto flush_g = [&]() {
        if (cg >= 0 && cg < G) {  // wave-uniform
            if (active) {
                unsigned* p = cell_cnt + (size_t)cg * (size_t)C + c0;
                if (V == 4) {
                    if (gcnt[0] | gcnt[V > 1 ? 1 : 0] | gcnt[V > 2 ? 2 : 0] | gcnt[V > 3 ? 3 : 0]) {
                        uint4 v = *(uint4*)p;
                        v.x += gcnt[0];
                        v.y += gcnt[V > 1 ? 1 : 0];
                        v.z += gcnt[V > 2 ? 2 : 0];
                        v.w += gcnt[V > 3 ? 3 : 0];
                        *(uint4*)p = v;
                    }
                } else if (gcnt[0]) {
                    p[0] += gcnt[0];
                }
            }
        } else {  // a label outside 0 .. G - 1 addresses nothing
            u64 s = 0;
#pragma unroll
            for (int j = 0; j < V; ++j) s += gcnt[j];
            if (s) atomicAdd(status + 1, s);
        }
#pragma unroll
        for (int j = 0; j < V; ++j) gcnt[j] = 0;
    };
    auto flush_s = [&]() {
        const bool ok = csg >= 0 && csg < G2;  // wave-uniform
#pragma unroll
        for (int j = 0; j < V; ++j) {
            if (scnt[j]) atomicAdd(ok ? sec_cnt + (size_t)csg * (size_t)R + scls[j] : status + 1, scnt[j]);
            scnt[j] = 0;
        }
    };
    for (long r = 0; r < Tb; r += OCC_U) {
        W w[OCC_U];
#pragma unroll
        for (int k = 0; k < OCC_U; ++k)
            w[k] = (active && r + k < Tb) ? *(const W*)(x + (size_t)(r + k) * (size_t)C + c0) : (W)0;
#pragma unroll  // w[k] must stay in registers: no dynamic indexing
        for (int k = 0; k < OCC_U; ++k) {
            if (r + k < Tb) {  // wave-uniform
                const long t = t0 + r + k;
                const int g = grp ? grp[t] : 0;
                if (g != cg) {
                    flush_g();
                    cg = g;
                }
                if (SECT) {
                    const int sg = sgrp[t];
                    if (sg != csg) {
                        flush_s();
                        csg = sg;
                    }
                }
#pragma unroll
                for (int j = 0; j < V; ++j) {
                    const int v = cell_value<V>(w[k], j);
                    const bool p = cell_present(v, match);
                    if (SIGNED) neg += v < 0;
                    gcnt[j] += p;
                    if (RUNS) {
                        nrun[j] += p && run[j] == 0;
                        run[j] = p ? run[j] + 1 : 0;
                        lng[j] = run[j] > lng[j] ? run[j] : lng[j];
                    }
                    if (SECT) scnt[j] += __popcll(__ballot(p) & smask[j]);
                }
            }
        }
    }
    flush_g();
    if (SECT) flush_s();
    if (RUNS && active) {
#pragma unroll
        for (int j = 0; j < V; ++j) {
            run_state[c0 + j] = run[j];
            run_state[(size_t)C + c0 + j] = nrun[j];
            run_state[2 * (size_t)C + c0 + j] = lng[j];
        }
    }
    if (SIGNED && neg) atomicAdd(status, (u64)neg);
}

template <typename T, int V>
static void occ_launch(marex_ctx* ctx, const T* x, long t0, long Tb, long C, int match, const int* grp, int G, const int* sgrp,
                       int G2, const int* cls, int R, unsigned* rs, unsigned* cell_cnt, u64* sec_cnt, u64* status) {
    const dim3 grid = cell_grid<V>(C), block(256);
#define OCC_GO(RUNS, SECT)                                                                                                  \
    hipLaunchKernelGGL((k_occurrence<T, V, RUNS, SECT>), grid, block, 0, ctx->stream, x, t0, Tb, C, match, grp, G, sgrp, G2, \
                       cls, R, rs, cell_cnt, sec_cnt, status)
    if (rs && sec_cnt)
        OCC_GO(true, true);
    else if (rs)
        OCC_GO(true, false);
    else if (sec_cnt)
        OCC_GO(false, true);
    else
        OCC_GO(false, false);
#undef OCC_GO
}

template <typename T>
static int occ_entry(marex_ctx* ctx, const char* name, const T* x, int64_t t0, int64_t Tb, int64_t C, int match,
                     const int32_t* grp, int G, const int32_t* sgrp, int G2, const int32_t* cls, int R, uint32_t* run_state,
                     uint32_t* cell_cnt, uint64_t* sec_cnt, uint64_t* status) {
    if (!ctx) return -1;
    const int nsec = (sec_cnt != nullptr) + (sgrp != nullptr) + (cls != nullptr);
    if (!x || !cell_cnt || !status || t0 < 0 || Tb <= 0 || C <= 0 || match < 0 || G <= 0 || (!grp && G != 1) ||
        (nsec != 0 && nsec != 3) || (nsec == 3 && (G2 <= 0 || R <= 0)))
        return fail(ctx, -1, "%s: null pointer, empty shape, negative match, no group, or section arguments given in part", name);
    if (const int rc = cell_stream_limits(ctx, name, t0, Tb, C)) return rc;
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    LaunchTimer lt(ctx, MAREX_K_MORPH);
    const bool quad = sizeof(T) == 1 && C % 4 == 0 && ((uintptr_t)x & 3) == 0 && ((uintptr_t)cell_cnt & 15) == 0 &&
                      ((uintptr_t)run_state & 15) == 0;
    if (sizeof(T) == 1 && quad)
        occ_launch<unsigned char, 4>(ctx, (const unsigned char*)x, (long)t0, (long)Tb, (long)C, match, grp, G, sgrp, G2, cls, R,
                                     (unsigned*)run_state, (unsigned*)cell_cnt, (u64*)sec_cnt, (u64*)status);
    else
        occ_launch<T, 1>(ctx, x, (long)t0, (long)Tb, (long)C, match, grp, G, sgrp, G2, cls, R, (unsigned*)run_state,
                         (unsigned*)cell_cnt, (u64*)sec_cnt, (u64*)status);
    HIP_TRY(ctx, hipGetLastError());
    return 0;
}

#define OCC_EXPORT(SFX, XT, T)  /* marex_occurrence_u8, marex_occurrence_i32 */                                                \
    extern "C" int marex_occurrence_##SFX(marex_ctx* ctx, const XT* x, int64_t t0, int64_t Tb, int64_t C, int match,           \
                                          const int32_t* grp, int G, const int32_t* sgrp, int G2, const int32_t* cls, int R,   \
                                          uint32_t* run_state, uint32_t* cell_cnt, uint64_t* sec_cnt, uint64_t* status) {      \
        return occ_entry<T>(ctx, "marex_occurrence_" #SFX, (const T*)x, t0, Tb, C, match, grp, G, sgrp, G2, cls, R, run_state, \
                            cell_cnt, sec_cnt, status);                                                                        \
    }
OCC_EXPORT(u8, uint8_t, unsigned char)
OCC_EXPORT(i32, int32_t, int)
