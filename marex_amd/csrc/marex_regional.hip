// marex_regional.hip -- per-(timestep, region) series of an event mask or a tracked ID field: the area in an extreme state,
// its cells, the weighted anomaly sums, the largest anomaly and the severity categories of every region at every step
// (the figure the marine-heatwave literature leads with: Hobday et al. 2018, Fig. 3; the basin series of Oliver et al.
// 2018).  One streaming pass: the presence field is read once, the anomalies only under present cells, the thresholds
// and weights only under present cells with a finite anomaly.
//
// Shape: unlike the per-cell kernels (marex_cellwalk.hip.h), where a lane keeps its cell for the whole call, every row is
// reduced ACROSS cells into a few (step, region) slots, and the key of a lane -- its region -- is the same at every row.
// A workgroup of four waves takes REG_WG_CELLS consecutive cells and every gridDim.y-th row; a wave takes IT consecutive
// 64-lane pieces of V cells per lane.  Before the row loop a wave tests each piece once: all its cells of one region
// (the common case: regions are spatially coherent), of none, or mixed.  In the row loop the lanes add their cells into
// their own registers for as long as consecutive pieces share the region; only when the region changes, and at the end of
// the row, the run is reduced over the wave (dpp_wave_sum) and flushed.  Where all four waves hold one and the same
// region (R = 1; the interior of a basin) the four wave sums are combined through LDS and one wave issues the global
// atomics: one set per workgroup and row instead of one per wave.  A mixed piece takes the general path: per distinct
// region of its present lanes one reduction and one flush.
//
// Arithmetic contract: counts and areas are integers, exact and independent of order, windows and layout.  The two
// float64 sums follow marex_event_intensity_f32: sums of exact products ((double)w * (double)a of two float32 values;
// -ffp-contract=off), added in an order that depends on the layout and on the arrival of the atomics: bit for bit
// reproducible whenever the partial sums are exactly representable, otherwise within 2 n u sum|w a| of the exact sum.
#include "marex_cellwalk.hip.h"

#define REG_TSTRIDE 32  // rows in flight: a workgroup walks every REG_TSTRIDE-th row
#define REG_NCAT 6      // below, moderate, strong, severe, extreme, undefined (severity_class)

// 64-lane pieces per wave: 4 x 256 cells with four uint8 cells per lane, 8 x 64 cells with one
template <int V>
struct reg_iters { static constexpr int n = V == 4 ? 4 : 8; };

// what a wave hands to the combining wave of its workgroup
struct RegPartial {
    unsigned nf, nb, key, has;
    long long ar;
    double sw, swa;
    unsigned cc[REG_NCAT];
    long long ca[REG_NCAT];
};

template <int V>
__device__ __forceinline__ void reg_load_f(const float* p, float (&o)[V]) {
    if constexpr (V == 4) {
        const float4 t = *(const float4*)p;
        o[0] = t.x, o[1] = t.y, o[2] = t.z, o[3] = t.w;
    } else {
        o[0] = *p;
    }
}

template <int V>
__device__ __forceinline__ void reg_load_q(const long long* p, long long (&o)[V]) {
    if constexpr (V == 4) {
        const longlong2 a = *(const longlong2*)p, b = *(const longlong2*)(p + 2);
        o[0] = a.x, o[1] = a.y, o[2] = b.x, o[3] = b.y;
    } else {
        o[0] = *p;
    }
}

// The wave reductions of this unit are dpp_wave_sum and dpp_wave_max_u32 (marex_common.hip.h).  The flushes are many -- one
// per wave, row and run -- and a shuffle butterfly of six LDS permutes per word made them the kernel's bound (DESIGN.md
// section 4); those take two.

// the merge of two "one region" summaries: -1 nothing, -2 more than one region, else the region
__device__ __forceinline__ int reg_merge(int a, int b) {
    if (a == -2 || b == -2) return -2;
    if (a == -1) return b;
    if (b == -1) return a;
    return a == b ? a : -2;
}

// Rows t0 .. t0 + Tb - 1: x (and anom) [Tb][C].  V: cells per lane (4: C % 4 == 0 and every array is aligned for the vector
// loads -- the entry point checks).  LEVEL 0: presence only; 1: with anom; 2: with anom, thr and doy.  q, wf and cat_area
// may be null at any level that has them.  Slot (t, r) is t * R + r; the entry point has checked t0 + Tb <= T, and a region
// outside 0 .. R - 1 is -1 here before it addresses anything.
template <typename T, int V, int LEVEL>
__global__ void __launch_bounds__(256)
k_regional_series(const T* __restrict__ x, long t0, long Tb, long C, int match, const int* __restrict__ reg, int R,
                  const long long* __restrict__ q, const float* __restrict__ wf, const float* __restrict__ anom,
                  const float* __restrict__ thr, const int* __restrict__ doy, int n_doy, long long* __restrict__ area,
                  u64* __restrict__ cnt, double* __restrict__ sums, unsigned* __restrict__ vmax, u64* __restrict__ cat_cnt,
                  long long* __restrict__ cat_area, u64* __restrict__ status) {
    typedef typename cell_word<T, V>::type W;
    constexpr bool SIGNED = std::is_same<T, int>::value;
    constexpr bool ANOM = LEVEL >= 1, CATS = LEVEL == 2;
    constexpr int IT = reg_iters<V>::n;
    constexpr int NC = CATS ? REG_NCAT : 1;
    __shared__ int s_one[4];
    __shared__ RegPartial s_part[2][4];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const long wave_cells = 64L * V * IT;
    const long rw = ((long)blockIdx.x * 4 + wave) * wave_cells;

    // the regions of this lane's cells, and per piece: its one region, -1 (no cell of a region) or -2 (mixed)
    int rg[IT][V], ru[IT];
    int one = -1;
#pragma unroll
    for (int k = 0; k < IT; ++k) {
        const long c0 = rw + ((long)k * 64 + lane) * V;
        int m = -1;
#pragma unroll
        for (int j = 0; j < V; ++j) {
            const int rv = c0 + j < C ? reg[c0 + j] : -1;
            rg[k][j] = (rv >= 0 && rv < R) ? rv : -1;
            m = rg[k][j] > m ? rg[k][j] : m;
        }
        const u64 have = __ballot(m >= 0);
        int u = -1;
        if (have) {  // wave-uniform
            const int lead = __shfl(m, __ffsll((long long)have) - 1, 64);
            bool ok = true;
#pragma unroll
            for (int j = 0; j < V; ++j) ok = ok && (rg[k][j] < 0 || rg[k][j] == lead);
            u = __ballot(!ok) ? -2 : lead;
        }
        ru[k] = __builtin_amdgcn_readfirstlane(u);
        one = reg_merge(one, ru[k]);
    }
    if (lane == 0) s_one[wave] = one;
    __syncthreads();
    const int bu = reg_merge(reg_merge(s_one[0], s_one[1]), reg_merge(s_one[2], s_one[3]));
    const bool shared = bu >= 0;  // workgroup-uniform: every cell of a region here belongs to region bu

    // the run of the current region, in the lanes' own registers
    unsigned nf = 0, nb = 0, key = 0, cc[NC];
    long long ar = 0, ca[NC];
    double sw = 0, swa = 0;
    unsigned neg = 0, lost = 0;
    auto clear = [&]() {
        nf = nb = key = 0;
        ar = 0;
        sw = swa = 0;
#pragma unroll
        for (int n = 0; n < NC; ++n) cc[n] = 0, ca[n] = 0;
    };
    clear();
    // the lanes' registers summed over the wave, in every lane; false (wave-uniform) where no lane holds a cell
    auto reduce = [&]() -> bool {
        if (!__ballot((nf | nb) != 0)) return false;
        // a wave's run holds at most 64 * IT * V <= 1024 cells: both counts in one word
        const unsigned both = dpp_wave_sum(nf | (nb << 16));
        nf = both & 0xFFFFu;
        nb = both >> 16;
        ar = q ? dpp_wave_sum(ar) : (long long)nf;
        if (ANOM && nf) {  // wave-uniform
            sw = wf ? dpp_wave_sum(sw) : (double)nf;
            swa = dpp_wave_sum(swa);
            key = dpp_wave_max_u32(key);
        }
        if (CATS && nf) {
            static_assert(!CATS || 64 * IT * V < 1024, "the six class counts of a run share one word, ten bits each");
            u64 six = 0;
#pragma unroll
            for (int n = 0; n < NC; ++n) six |= (u64)cc[n] << (10 * n);
            six = dpp_wave_sum(six);
#pragma unroll
            for (int n = 0; n < NC; ++n) {
                cc[n] = (unsigned)(six >> (10 * n)) & 1023u;
                if (cat_area && cc[n]) ca[n] = dpp_wave_sum(ca[n]);  // wave-uniform; a class without a cell holds 0 in every lane
            }
        }
        return true;
    };
    // the totals, equal in every lane, into slot (t, r): contiguous bytes per array, one lane per element
    auto emit = [&](long long t, int r) {
        const size_t s = (size_t)t * (size_t)R + (size_t)r;
        if (lane < 2) {
            const u64 v = lane == 0 ? nf : nb;
            if (v) atomicAdd(cnt + s * 2 + lane, v);
            if (ANOM && nf) atomicAdd(sums + s * 2 + lane, lane == 0 ? sw : swa);
        } else if (lane == 2) {
            if (nf) atomicAdd((u64*)area + s, (u64)ar);
            if (ANOM && key) atomicMax(vmax + s, key);
        }
        if (CATS && nf && lane < REG_NCAT) {
            unsigned v = 0;
            long long a = 0;
#pragma unroll
            for (int n = 0; n < NC; ++n) {
                v = lane == n ? cc[n] : v;
                a = lane == n ? ca[n] : a;
            }
            if (v) atomicAdd(cat_cnt + s * REG_NCAT + lane, (u64)v);
            if (cat_area && a) atomicAdd((u64*)cat_area + s * REG_NCAT + lane, (u64)a);
        }
    };
    int par = 0;
    for (long row = blockIdx.y; row < Tb; row += gridDim.y) {  // workgroup-uniform bounds: the barriers below are met by all
        const long long t = t0 + row;
        const T* xrow = x + (size_t)row * (size_t)C;
        int dk = 0;
        if (CATS) dk = doy[t];
        const bool dok = !CATS || (dk >= 0 && dk < n_doy);  // workgroup-uniform
        W w[IT];
        unsigned pm[IT];
        float av[IT][V];
#pragma unroll
        for (int k = 0; k < IT; ++k) {
            const long c0 = rw + ((long)k * 64 + lane) * V;
            w[k] = c0 < C ? *(const W*)(xrow + c0) : (W)0;  // V == 4: C % 4 == 0, so all four cells exist
        }
#pragma unroll
        for (int k = 0; k < IT; ++k) {
            pm[k] = 0;
#pragma unroll
            for (int j = 0; j < V; ++j) {
                const int v = cell_value<V>(w[k], j);
                if (SIGNED) neg += v < 0;
                pm[k] |= (unsigned)(cell_present(v, match) && rg[k][j] >= 0) << j;  // a lane past C holds 0 and region -1
            }
            if (!dok) {  // the step addresses nothing: its present cells are counted
                lost += __popc(pm[k]);
                pm[k] = 0;
            }
        }
        if (ANOM) {
#pragma unroll
            for (int k = 0; k < IT; ++k) {
                const long c0 = rw + ((long)k * 64 + lane) * V;  // pm[k] != 0 implies c0 < C
#pragma unroll
                for (int j = 0; j < V; ++j) av[k][j] = 0.f;
                if (pm[k]) reg_load_f<V>(anom + (size_t)row * (size_t)C + c0, av[k]);
            }
        }
        int cur = -1;
        auto flush = [&]() {  // the run of region cur ends inside a wave's cells: its own atomics
            if (cur >= 0 && reduce()) emit(t, cur);
            clear();
        };
#pragma unroll  // w[k], pm[k], av[k], rg[k] must stay in registers: no dynamic indexing
        for (int k = 0; k < IT; ++k) {
            if (ru[k] == -1 || !__ballot(pm[k] != 0)) continue;  // wave-uniform
            const long c0 = rw + ((long)k * 64 + lane) * V;
            unsigned fm = 0;  // the present cells with a finite anomaly: what the area, the sums and the classes see
            float hv[V], wv[V];
            long long qv[V];
#pragma unroll
            for (int j = 0; j < V; ++j) {
                fm |= (unsigned)(((pm[k] >> j) & 1u) && (!ANOM || finite_bits(av[k][j]))) << j;
                hv[j] = 0.f, wv[j] = 1.f, qv[j] = 1;
            }
            if (fm) {
                if (CATS) reg_load_f<V>(thr + (size_t)dk * (size_t)C + c0, hv);
                if (ANOM && wf) reg_load_f<V>(wf + c0, wv);
                if (q) reg_load_q<V>(q + c0, qv);
            }
            auto add = [&](int j) {  // cell j of the piece into the lane's run
                if (!((fm >> j) & 1u)) {
                    nb += 1;  // present, anomaly NaN or +-inf: counted, nothing else
                    return;
                }
                nf += 1;
                ar += qv[j];
                if (ANOM) {
                    const float a = av[k][j];
                    const double wd = (double)wv[j];
                    sw += wd;
                    swa += wd * (double)a;
                    const unsigned ky = ordered_key(a);
                    key = ky > key ? ky : key;
                    if (CATS) {
                        const int c = severity_class(a, hv[j]);
#pragma unroll
                        for (int n = 0; n < NC; ++n) {
                            cc[n] += c == n;
                            ca[n] += c == n ? qv[j] : 0;
                        }
                    }
                }
            };
            if (ru[k] >= 0) {  // one region: its run goes on, or begins
                if (ru[k] != cur) {
                    flush();
                    cur = ru[k];
                }
#pragma unroll
                for (int j = 0; j < V; ++j)
                    if ((pm[k] >> j) & 1u) add(j);
                continue;
            }
            flush();  // mixed: per distinct region of the present cells one reduction and one flush
            cur = -1;
            unsigned pend = pm[k];
            for (;;) {
                const u64 todo = __ballot(pend != 0);
                if (!todo) break;
                int mine = -1;
#pragma unroll
                for (int j = V - 1; j >= 0; --j) mine = ((pend >> j) & 1u) ? rg[k][j] : mine;
                const int rl = __shfl(mine, __ffsll((long long)todo) - 1, 64);  // each round takes at least that cell: at most 64 V rounds
#pragma unroll
                for (int j = 0; j < V; ++j) {
                    if (((pend >> j) & 1u) && rg[k][j] == rl) {
                        add(j);
                        pend &= ~(1u << j);
                    }
                }
                if (reduce()) emit(t, rl);
                clear();
            }
        }
        if (!shared) {
            flush();
            continue;
        }
        // every run of this row is region bu: the four wave sums meet in LDS, wave 0 adds them up and issues the atomics
        const bool any = reduce();
        if (lane == 0) {
            RegPartial& p = s_part[par][wave];
            p.has = any;
            if (any) {
                p.nf = nf, p.nb = nb, p.key = key, p.ar = ar, p.sw = sw, p.swa = swa;
#pragma unroll
                for (int n = 0; n < NC; ++n) p.cc[n] = cc[n], p.ca[n] = ca[n];
            }
        }
        clear();
        __syncthreads();
        if (wave == 0) {
            bool some = false;
            for (int v = 0; v < 4; ++v) {
                const RegPartial& p = s_part[par][v];
                if (!p.has) continue;
                some = true;
                nf += p.nf, nb += p.nb, ar += p.ar, sw += p.sw, swa += p.swa;
                key = p.key > key ? p.key : key;
#pragma unroll
                for (int n = 0; n < NC; ++n) cc[n] += p.cc[n], ca[n] += p.ca[n];
            }
            if (some) emit(t, bu);
            clear();
        }
        par ^= 1;  // the next row writes the other half: wave 0 has read this one before it meets the next barrier
    }
    if (lost) atomicAdd(status + 1, (u64)lost);
    if (SIGNED && neg) atomicAdd(status, (u64)neg);
}

template <typename T, int V>
static void reg_launch(marex_ctx* ctx, const T* x, long t0, long Tb, long C, int match, const int* reg, int R, const long long* q,
                       const float* wf, const float* anom, const float* thr, const int* doy, int n_doy, long long* area, u64* cnt,
                       double* sums, unsigned* vmax, u64* cat_cnt, long long* cat_area, u64* status) {
    const long wg = 4L * 64 * V * reg_iters<V>::n;
    const dim3 grid = slice_grid(Tb, C, wg, REG_TSTRIDE), block(256);
#define REG_GO(LEVEL)                                                                                                         \
    hipLaunchKernelGGL((k_regional_series<T, V, LEVEL>), grid, block, 0, ctx->stream, x, t0, Tb, C, match, reg, R, q, wf, anom, \
                       thr, doy, n_doy, area, cnt, sums, vmax, cat_cnt, cat_area, status)
    if constexpr (V == 1) {  // the category build exists at one cell per lane only (262 registers at four)
        if (thr) {
            REG_GO(2);
            return;
        }
    }
    if (anom)
        REG_GO(1);
    else
        REG_GO(0);
#undef REG_GO
}

template <typename T>
static int reg_entry(marex_ctx* ctx, const char* name, const T* x, int64_t t0, int64_t Tb, int64_t C, int64_t Tn, int match,
                     const int32_t* reg, int R, const int64_t* q, const float* wf, const float* anom, const float* thr,
                     const int32_t* doy, int n_doy, int64_t* area, uint64_t* cnt, double* sums, uint32_t* vmax, uint64_t* cat_cnt,
                     int64_t* cat_area, uint64_t* status) {
    if (!ctx) return -1;
    const int nan = (anom != nullptr) + (sums != nullptr) + (vmax != nullptr);
    const int ncat = (thr != nullptr) + (doy != nullptr) + (cat_cnt != nullptr);
    if (!x || !reg || !area || !cnt || !status || t0 < 0 || Tb <= 0 || C <= 0 || Tn < t0 + Tb || match < 0 || R <= 0 ||
        (nan != 0 && nan != 3) || (wf && !anom) || (ncat != 0 && ncat != 3) || (ncat == 3 && (n_doy <= 0 || !anom)) ||
        ((cat_area != nullptr) != (ncat == 3 && q != nullptr)))
        return fail(ctx, -1, "%s: null pointer, empty shape, a window past the slots, negative match, no region, anomaly or "
                             "category arguments given in part, weights or thresholds without anomalies, or cat_area without "
                             "thresholds and areas", name);
    if (const int rc = cell_stream_limits(ctx, name, t0, Tb, C)) return rc;
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    LaunchTimer lt(ctx, MAREX_K_MORPH);
    // four cells per lane without thresholds: a 32-bit word of x, 16-byte vectors of anom, wf and q
    const auto al = [](const void* p, uintptr_t a) { return ((uintptr_t)p & (a - 1)) == 0; };
    const bool quad = sizeof(T) == 1 && !thr && C % 4 == 0 && al(x, 4) && al(anom, 16) && al(wf, 16) && al(q, 16);
    if (sizeof(T) == 1 && quad)
        reg_launch<unsigned char, 4>(ctx, (const unsigned char*)x, (long)t0, (long)Tb, (long)C, match, reg, R, (const long long*)q,
                                     wf, anom, thr, doy, n_doy, (long long*)area, (u64*)cnt, sums, (unsigned*)vmax, (u64*)cat_cnt,
                                     (long long*)cat_area, (u64*)status);
    else
        reg_launch<T, 1>(ctx, x, (long)t0, (long)Tb, (long)C, match, reg, R, (const long long*)q, wf, anom, thr, doy, n_doy,
                         (long long*)area, (u64*)cnt, sums, (unsigned*)vmax, (u64*)cat_cnt, (long long*)cat_area, (u64*)status);
    HIP_TRY(ctx, hipGetLastError());
    return 0;
}

// the constants the kernels above are compiled with, for callers and tests that place cases at their edges
extern "C" int marex_regional_layout(int cells_per_lane, int32_t* out) {
    if (!out || (cells_per_lane != 1 && cells_per_lane != 4)) return -1;
    const int it = cells_per_lane == 4 ? reg_iters<4>::n : reg_iters<1>::n;
    out[0] = 64 * cells_per_lane * it;  // cells of a wave per row
    out[1] = 4 * out[0];                // cells of a workgroup per row
    out[2] = REG_TSTRIDE;               // rows between two of a workgroup's
    return 0;
}

#define REG_EXPORT(SFX, XT, T)  /* marex_regional_series_u8, marex_regional_series_i32 */                                        \
    extern "C" int marex_regional_series_##SFX(                                                                                  \
        marex_ctx* ctx, const XT* x, int64_t t0, int64_t Tb, int64_t C, int64_t T_slots, int match, const int32_t* reg, int R,    \
        const int64_t* q, const float* wf, const float* anom, const float* thr, const int32_t* doy, int n_doy, int64_t* area,     \
        uint64_t* cnt, double* sums, uint32_t* vmax, uint64_t* cat_cnt, int64_t* cat_area, uint64_t* status) {                    \
        return reg_entry<T>(ctx, "marex_regional_series_" #SFX, (const T*)x, t0, Tb, C, T_slots, match, reg, R, q, wf, anom, thr, \
                            doy, n_doy, area, cnt, sums, vmax, cat_cnt, cat_area, status);                                        \
    }
REG_EXPORT(u8, uint8_t, unsigned char)
REG_EXPORT(i32, int32_t, int)
