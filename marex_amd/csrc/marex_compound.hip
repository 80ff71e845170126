// marex_compound.hip -- compound events of two presence fields A and B (the guide's "Advanced Features" entry,
// docs/user_guide.rst:821-833: sst_extremes.extreme_events & salinity_extremes.extreme_events): per cell the steps with A,
// with B and with both by time group, the run statistics of the joint mask, the pairs A[t] and B[t + l] at the lags
// l = -L .. L, and the runs of each field that the other one meets within a tolerance of K steps; per (time group, spatial
// class) the three counts; optionally the joint mask itself.  One streaming pass: both fields are read once, nothing else
// of their size is touched but the rows of the joint mask when it is asked for.
//
// Layout: that of k_occurrence (marex_occurrence.hip) -- a lane owns one cell, or four consecutive uint8 cells of both
// fields through one 32-bit load each, for the whole call and walks the rows with CMP_U loads of each field in flight.
// Everything of a cell lives in the lane's registers and is carried between calls in state [CMP_STATE_ROWS][C]:
//   0 .. 2   the open joint run, the joint runs begun, the longest joint run (run_state of marex_occurrence_*);
//   3, 4     the history word of A and of B: bit l is the presence l steps ago (bit 0: the step just taken); without lags
//            it is kept up to bit K;
//   5, 6     the run-coincidence word of A and of B: bit 30 a run is open, bit 31 it has met the other field, bits 0 ..
//            K - 1 the unmet runs that ended i + 1 steps ago (several may wait at once: two short runs inside K steps);
//   7 .. 10  runs of A, coincident runs of A, runs of B, coincident runs of B;
//   11, 12   with lags only: the histories' steps 32 .. 61 ago.
// A run is counted as coincident once, at the first step that decides it: at its start (the other field's history holds a
// step of the last K), while it is open, or while it waits in bits 0 .. K - 1 and the other field turns up.
// A lane whose cells hold nothing -- no presence in the row, empty histories, no open or waiting run -- skips the row's
// arithmetic.
// The three counters of the current time group are added to cell_cnt by plain read-modify-writes of the owning lane when
// the (wave-uniform) group label changes.  The lag counters live in the global rows lag_cnt [2 L + 1][C]; no step touches
// them.  Every CMP_LAG_BLOCK = 32 rows, and at the end of the call, the owning lane counts the pairs whose later step lies
// in the rows since the last such point -- popcount(new steps of B & (history of A >> l)) for l >= 0, the reverse for
// l < 0 -- and adds each lag's count to its row, one read-modify-write per lag, block and cell that has one (DESIGN.md
// section 4).  A pair is counted exactly once, in the block of its later step, so the windows do not matter.  No atomic
// touches a per-cell output.  The section counts take the wave's class partition once (wave_class_partition), shared by
// the three counts.
// All results are integers: exact, and independent of any order and of how the rows are cut into calls.
#include "marex_cellwalk.hip.h"

// rows loaded together: loads of each field in flight per lane, in both layouts
#ifndef CMP_U
#define CMP_U 8
#endif
#define CMP_STATE_ROWS 13
#define CMP_MAX_LAG 30
// rows between two additions to the lag counters: the new steps fill a 32-bit word, new steps + CMP_MAX_LAG a 64-bit one
#define CMP_LAG_BLOCK 32
static_assert(CMP_LAG_BLOCK % CMP_U == 0 && CMP_LAG_BLOCK + CMP_MAX_LAG <= 64, "the lag blocks end with a batch of rows");

static constexpr unsigned CO_OPEN = 1u << 30, CO_HIT = 1u << 31;

template <int V>
__device__ __forceinline__ void cells_get(const unsigned* p, unsigned (&v)[V]) {
    if constexpr (V == 4) {
        const uint4 q = *(const uint4*)p;
        v[0] = q.x, v[1] = q.y, v[2] = q.z, v[3] = q.w;
    } else {
        v[0] = p[0];
    }
}

template <int V>
__device__ __forceinline__ void cells_put(unsigned* p, const unsigned (&v)[V]) {
    if constexpr (V == 4)
        *(uint4*)p = make_uint4(v[0], v[1], v[2], v[3]);
    else
        p[0] = v[0];
}

// p[j] += v[j], v[j] = 0; nothing is touched where every v[j] is 0
template <int V>
__device__ __forceinline__ void cells_add(unsigned* p, unsigned (&v)[V]) {
    unsigned any = 0;
#pragma unroll
    for (int j = 0; j < V; ++j) any |= v[j];
    if (any) {
        unsigned q[V];
        cells_get<V>(p, q);
#pragma unroll
        for (int j = 0; j < V; ++j) q[j] += v[j];
        cells_put<V>(p, q);
    }
#pragma unroll
    for (int j = 0; j < V; ++j) v[j] = 0;
}

// One step of the run coincidence of a field (present: a) against the other one (present: b; other: its history with
// this step at bit 0).  kmask: bits 0 .. K, pmask: bits 0 .. K - 1.
__device__ __forceinline__ void coincidence_step(unsigned& co, bool a, bool b, unsigned other, unsigned kmask, unsigned pmask,
                                                 unsigned& runs, unsigned& met) {
    const bool open = co & CO_OPEN, hit = co & CO_HIT;
    unsigned pend = (co << 1) & pmask;           // a step older; past K steps a run waits no longer
    if (open && !a && !hit) pend |= 1u & pmask;  // the run ended one step ago, unmet
    if (b) {
        met += __popc(pend);
        pend = 0;
    }
    bool nhit = false;
    if (a) {
        nhit = open ? (hit || b) : (other & kmask) != 0;
        runs += !open;
        met += nhit && !(open && hit);
    }
    co = pend | (a ? CO_OPEN : 0u) | (nhit ? CO_HIT : 0u);
}

// Rows t0 .. t0 + Tb - 1 of both fields: xa, xb [Tb][C].  V: cells per lane (4: C % 4 == 0 and xa, xb, mask, state and
// cell_cnt are aligned for the vector accesses -- the entry point checks); SECT: sec_cnt, sgrp and cls are given; LAG:
// L > 0 and lag_cnt (aligned as cell_cnt) is given; MASK: mask is given.  Lanes past the last cell stay in the loop (they take part in the
// ballots) with nothing present.
template <int V, bool SECT, bool LAG, bool MASK>
__global__ void __launch_bounds__(256)
k_compound(const unsigned char* __restrict__ xa, const unsigned char* __restrict__ xb, long t0, long Tb, long C, int L, int K,
           const int* __restrict__ grp, int G, const int* __restrict__ sgrp, int G2, const int* __restrict__ cls, int R,
           unsigned* state, unsigned* cell_cnt, unsigned* lag_cnt, u64* sec_cnt, unsigned char* mask, u64* status) {
    typedef typename cell_word<unsigned char, V>::type W;
    const int lane = threadIdx.x & 63;
    const long c0 = ((long)blockIdx.x * 256 + threadIdx.x) * V;
    const bool active = c0 < C;  // V == 4: C % 4 == 0, so all four cells exist
    const unsigned kmask = (2u << K) - 1u, pmask = (1u << K) - 1u;
    const unsigned hmask = LAG ? ~0u : kmask, himask = (1u << (CMP_LAG_BLOCK + CMP_MAX_LAG - 32)) - 1u;
    constexpr int NS = LAG ? CMP_STATE_ROWS : CMP_STATE_ROWS - 2;  // rows this instantiation carries
    unsigned st[CMP_STATE_ROWS][V];  // indexed by constants only: registers
    unsigned ga[V], gb[V], gab[V];
    u64 smask[V], sa[V], sb[V], sab[V];
    int scls[V];
    unsigned live = 0;
#pragma unroll
    for (int j = 0; j < V; ++j) {
        ga[j] = gb[j] = gab[j] = 0;
        smask[j] = sa[j] = sb[j] = sab[j] = 0;
        scls[j] = 0;
        if (SECT) {  // the wave's distinct classes among the sub-cells j: the k-th goes to lane k
            const int cj = active ? cls[c0 + j] : -1;
            wave_class_partition(cj, R, lane, smask[j], scls[j]);
        }
    }
#pragma unroll
    for (int s = 0; s < CMP_STATE_ROWS; ++s) {
#pragma unroll
        for (int j = 0; j < V; ++j) st[s][j] = 0;
        if (active && s < NS) cells_get<V>(state + (size_t)s * (size_t)C + c0, st[s]);
    }
#pragma unroll
    for (int j = 0; j < V; ++j) live |= st[0][j] | st[3][j] | st[4][j] | st[5][j] | st[6][j] | st[11][j] | st[12][j];
    int cg = grp ? grp[t0] : 0;
    int csg = SECT ? sgrp[t0] : 0;
    auto flush_g = [&]() {
        if (cg >= 0 && cg < G) {  // wave-uniform
            if (active) {
                cells_add<V>(cell_cnt + (size_t)cg * (size_t)C + c0, ga);
                cells_add<V>(cell_cnt + ((size_t)G + cg) * (size_t)C + c0, gb);
                cells_add<V>(cell_cnt + (2 * (size_t)G + cg) * (size_t)C + c0, gab);
            }
        } else {  // a label outside 0 .. G - 1 addresses nothing
            u64 s = 0;
#pragma unroll
            for (int j = 0; j < V; ++j) s += (u64)ga[j] + gb[j];
            if (s) atomicAdd(status + 1, s);
        }
#pragma unroll
        for (int j = 0; j < V; ++j) ga[j] = gb[j] = gab[j] = 0;
    };
    auto flush_s = [&]() {
        const bool ok = csg >= 0 && csg < G2;  // wave-uniform
        const size_t plane = (size_t)G2 * (size_t)R;
#pragma unroll
        for (int j = 0; j < V; ++j) {
            u64* p = sec_cnt + (size_t)csg * (size_t)R + scls[j];
            if (ok) {
                if (sa[j]) atomicAdd(p, sa[j]);
                if (sb[j]) atomicAdd(p + plane, sb[j]);
                if (sab[j]) atomicAdd(p + 2 * plane, sab[j]);
            } else if (sa[j] + sb[j]) {
                atomicAdd(status + 1, sa[j] + sb[j]);
            }
            sa[j] = sb[j] = sab[j] = 0;
        }
    };
    // the pairs whose later step is one of the last n rows (1 .. 32), added to the rows of their lags
    auto flush_lag = [&](int n) {
        const unsigned fresh = n >= 32 ? ~0u : (1u << n) - 1u;
        unsigned an[V], bn[V], any = 0;
#pragma unroll
        for (int j = 0; j < V; ++j) {
            an[j] = st[3][j] & fresh;
            bn[j] = st[4][j] & fresh;
            any |= an[j] | bn[j];
        }
        if (!any || !active) return;
        for (int l = 0; l <= L; ++l) {  // B now or later: A[t], B[t + l]
            unsigned v[V];
#pragma unroll
            for (int j = 0; j < V; ++j) v[j] = __popc(bn[j] & (unsigned)((((u64)st[11][j] << 32) | st[3][j]) >> l));
            cells_add<V>(lag_cnt + (size_t)(L + l) * (size_t)C + c0, v);
        }
        for (int l = 1; l <= L; ++l) {  // B earlier: A[t], B[t - l]
            unsigned v[V];
#pragma unroll
            for (int j = 0; j < V; ++j) v[j] = __popc(an[j] & (unsigned)((((u64)st[12][j] << 32) | st[4][j]) >> l));
            cells_add<V>(lag_cnt + (size_t)(L - l) * (size_t)C + c0, v);
        }
    };
    for (long r = 0; r < Tb; r += CMP_U) {
        W wa[CMP_U], wb[CMP_U];
#pragma unroll
        for (int k = 0; k < CMP_U; ++k) {
            const bool in = active && r + k < Tb;
            const size_t at = (size_t)(r + k) * (size_t)C + c0;
            wa[k] = in ? *(const W*)(xa + at) : (W)0;
            wb[k] = in ? *(const W*)(xb + at) : (W)0;
        }
#pragma unroll  // wa[k], wb[k] must stay in registers: no dynamic indexing
        for (int k = 0; k < CMP_U; ++k) {
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
                bool pa[V], pb[V];
                unsigned out = 0;
#pragma unroll
                for (int j = 0; j < V; ++j) {
                    pa[j] = cell_value<V>(wa[k], j) != 0;
                    pb[j] = cell_value<V>(wb[k], j) != 0;
                    out |= (unsigned)(pa[j] && pb[j]) << (8 * j);
                }
                if (wa[k] | wb[k] | live) {  // else: nothing present, nothing remembered, nothing changes
                    live = 0;
#pragma unroll
                    for (int j = 0; j < V; ++j) {
                        const bool a = pa[j], b = pb[j], ab = a && b;
                        ga[j] += a;
                        gb[j] += b;
                        gab[j] += ab;
                        st[1][j] += ab && st[0][j] == 0;
                        st[0][j] = ab ? st[0][j] + 1 : 0;
                        st[2][j] = st[0][j] > st[2][j] ? st[0][j] : st[2][j];
                        if (LAG) {
                            st[11][j] = ((st[11][j] << 1) | (st[3][j] >> 31)) & himask;
                            st[12][j] = ((st[12][j] << 1) | (st[4][j] >> 31)) & himask;
                        }
                        st[3][j] = ((st[3][j] << 1) | (unsigned)a) & hmask;
                        st[4][j] = ((st[4][j] << 1) | (unsigned)b) & hmask;
                        coincidence_step(st[5][j], a, b, st[4][j], kmask, pmask, st[7][j], st[8][j]);
                        coincidence_step(st[6][j], b, a, st[3][j], kmask, pmask, st[9][j], st[10][j]);
                        live |= st[0][j] | st[3][j] | st[4][j] | st[5][j] | st[6][j] | st[11][j] | st[12][j];
                    }
                }
                if (MASK && active) *(W*)(mask + (size_t)t * (size_t)C + c0) = (W)out;  // every byte, zeros included
                if (SECT) {
#pragma unroll
                    for (int j = 0; j < V; ++j) {
                        const u64 ba = __ballot(pa[j]), bb = __ballot(pb[j]);
                        sa[j] += __popcll(ba & smask[j]);
                        sb[j] += __popcll(bb & smask[j]);
                        sab[j] += __popcll(ba & bb & smask[j]);
                    }
                }
            }
        }
        if (LAG && r + CMP_U <= Tb && (r + CMP_U) % CMP_LAG_BLOCK == 0) flush_lag(CMP_LAG_BLOCK);  // wave-uniform
    }
    if (LAG && Tb % CMP_LAG_BLOCK) flush_lag((int)(Tb % CMP_LAG_BLOCK));
    flush_g();
    if (SECT) flush_s();
    if (active) {
#pragma unroll
        for (int s = 0; s < NS; ++s) cells_put<V>(state + (size_t)s * (size_t)C + c0, st[s]);
    }
}

template <int V>
static void cmp_launch(marex_ctx* ctx, const unsigned char* xa, const unsigned char* xb, long t0, long Tb, long C, int L, int K,
                       const int* grp, int G, const int* sgrp, int G2, const int* cls, int R, unsigned* state, unsigned* cell_cnt,
                       unsigned* lag_cnt, u64* sec_cnt, unsigned char* mask, u64* status) {
    const dim3 grid = cell_grid<V>(C), block(256);
#define CMP_GO(SECT, LAG, MASK)                                                                                              \
    hipLaunchKernelGGL((k_compound<V, SECT, LAG, MASK>), grid, block, 0, ctx->stream, xa, xb, t0, Tb, C, L, K, grp, G, sgrp, \
                       G2, cls, R, state, cell_cnt, lag_cnt, sec_cnt, mask, status)
    switch ((sec_cnt ? 4 : 0) | (lag_cnt ? 2 : 0) | (mask ? 1 : 0)) {
        case 0: CMP_GO(false, false, false); break;
        case 1: CMP_GO(false, false, true); break;
        case 2: CMP_GO(false, true, false); break;
        case 3: CMP_GO(false, true, true); break;
        case 4: CMP_GO(true, false, false); break;
        case 5: CMP_GO(true, false, true); break;
        case 6: CMP_GO(true, true, false); break;
        default: CMP_GO(true, true, true); break;
    }
#undef CMP_GO
}

extern "C" int marex_compound_u8(marex_ctx* ctx, const uint8_t* a, const uint8_t* b, int64_t t0, int64_t Tb, int64_t C,
                                 int max_lag, int tolerance, const int32_t* grp, int G, const int32_t* sgrp, int G2,
                                 const int32_t* cls, int R, uint32_t* state, uint32_t* cell_cnt, uint32_t* lag_cnt,
                                 uint64_t* sec_cnt, uint8_t* mask, uint64_t* status) {
    const char* name = "marex_compound_u8";
    if (!ctx) return -1;
    const int nsec = (sec_cnt != nullptr) + (sgrp != nullptr) + (cls != nullptr);
    if (!a || !b || !state || !cell_cnt || !status || t0 < 0 || Tb <= 0 || C <= 0 || G <= 0 || (!grp && G != 1) ||
        (nsec != 0 && nsec != 3) || (nsec == 3 && (G2 <= 0 || R <= 0)))
        return fail(ctx, -1, "%s: null pointer, empty shape, no group, or section arguments given in part", name);
    if (max_lag < 0 || max_lag > CMP_MAX_LAG || tolerance < 0 || tolerance > CMP_MAX_LAG || (max_lag > 0) != (lag_cnt != nullptr))
        return fail(ctx, -1, "%s: max_lag and tolerance must lie in 0 .. %d, and lag_cnt is given exactly with max_lag > 0", name,
                    CMP_MAX_LAG);
    if (const int rc = cell_stream_limits(ctx, name, t0, Tb, C)) return rc;
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    LaunchTimer lt(ctx, MAREX_K_MORPH);
    const bool quad = C % 4 == 0 && (((uintptr_t)a | (uintptr_t)b | (uintptr_t)mask) & 3) == 0 &&
                      (((uintptr_t)state | (uintptr_t)cell_cnt | (uintptr_t)lag_cnt) & 15) == 0;
    if (quad)
        cmp_launch<4>(ctx, a, b, (long)t0, (long)Tb, (long)C, max_lag, tolerance, grp, G, sgrp, G2, cls, R, (unsigned*)state,
                      (unsigned*)cell_cnt, (unsigned*)lag_cnt, (u64*)sec_cnt, mask, (u64*)status);
    else
        cmp_launch<1>(ctx, a, b, (long)t0, (long)Tb, (long)C, max_lag, tolerance, grp, G, sgrp, G2, cls, R, (unsigned*)state,
                      (unsigned*)cell_cnt, (unsigned*)lag_cnt, (u64*)sec_cnt, mask, (u64*)status);
    HIP_TRY(ctx, hipGetLastError());
    return 0;
}
