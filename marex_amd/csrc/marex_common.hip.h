#pragma once
// marex_common.hip.h -- shared by every translation unit of libmarex_hip.so: context, error / timing helpers,
// device helpers.  Hand-written gfx950 (CDNA4) kernels + C ABI for the preprocess_data hot path:
//   marex_context.hip     context, stream, timing
//   marex_synth.hip       synthetic field (bench / tests)
//   marex_shifting.hip    K_A: shifting-baseline anomaly (general kernel, fast kernel, classification)
//   marex_thresholds.hip  K_T: day-of-year thresholds (band algorithm, sliding histograms)
//   marex_mask.hip        anomaly >= threshold, transpose
//   marex_anomalies.hip   fixed baseline, digitize, detrend, std_normalise
//   marex_quantiles.hip   exact Hobday percentile, global thresholds
//   marex_tails.hip       tail extraction, thresholds and mask from tails (the default approximate-Hobday path)
//
// Build: hipcc --offload-arch=gfx950 -O3 -ffp-contract=off -fPIC, one object per file, linked -shared (csrc/build.py).
// -ffp-contract=off is part of the arithmetic contract (oracle/marex_oracle.py C1-C6): every float
// add / multiply / divide below is an individually rounded IEEE operation, never fused.
//
// All kernels are HBM / LDS bound streaming or counting kernels (no MFMA): wave64, 256-thread
// workgroups, one lane per grid cell so that a wave reads 256 contiguous bytes of a (time, cell) row.
#include <hip/hip_runtime.h>

#include <cmath>
#include <type_traits>
#include <cstdarg>
#include <cstdio>
#include <cstring>
#include <map>
#include <string>
#include <vector>

#include "marex_hip.h"

#define NDOY MAREX_NDOY

typedef unsigned long long u64;

// ------------------------------------------------------------------------------------------------
// context
// ------------------------------------------------------------------------------------------------
struct TimedLaunch {
    int kid;
    hipEvent_t a, b;
};

struct marex_ctx {
    int device = 0;
    hipStream_t stream = nullptr;
    std::string err;
    bool timing = false;
    std::vector<TimedLaunch> pending;
    double total_ms[MAREX_K_COUNT] = {0};
    int64_t launches[MAREX_K_COUNT] = {0};
    int* shift_info = nullptr;  // device, SHIFT_INFO_WORDS ints: which dayofyear chunks the fast anomaly kernel takes
    int* shift_plan = nullptr;  // device, [calendar years][92 chunks][8] ints: per-year records of the fast anomaly kernel
    size_t shift_plan_years = 0;
    int* shift_lplan = nullptr;  // device, [calendar years + 2][92 chunks][8] ints: lean records of k_shift_lean
    size_t shift_lplan_years = 0;
    unsigned char* thr_scratch = nullptr;  // device, per-(tile, day, lane) state bytes of the 1024-thread threshold tiles
    size_t thr_scratch_bytes = 0;
    unsigned char* detrend_scratch = nullptr;  // device, partial sums / coefficients / means of the detrend reductions
    size_t detrend_scratch_bytes = 0;
    unsigned char* morph_scratch = nullptr;  // device, two bit-packed padded images of the morphology passes
    size_t morph_scratch_bytes = 0;
    int n_cu = 0;  // compute units of the device (queried on first use)
    std::map<std::string, int> opts;          // tuning / diagnostic options (marex_set_option; seeded from MAREX_* at creation)
    long long* row_off = nullptr;             // device, byte offset of every kept row in dayofyear order (tail extraction)
    size_t row_off_bytes = 0;
    long long* row_off_mask = nullptr;        // the same for the one-byte-per-cell mask array (mask from tails)
    size_t row_off_mask_bytes = 0;
    unsigned long long* dbg_counters = nullptr;  // device, MAREX_DBG_COUNTERS event counters of the tail kernels
};

#define MAREX_DBG_COUNTERS 8

// Option lookup: options are set through marex_set_option (or, once, from the environment variables MAREX_<NAME> that
// exist when the context is created); nothing reads the environment at launch time.
static inline int ctx_opt(marex_ctx* ctx, const char* name, int dflt) {
    auto it = ctx->opts.find(name);
    return it == ctx->opts.end() ? dflt : it->second;
}

static inline unsigned long long* ctx_debug_counters(marex_ctx* ctx) {
    if (!ctx->dbg_counters) {
        if (hipMalloc((void**)&ctx->dbg_counters, MAREX_DBG_COUNTERS * sizeof(unsigned long long)) != hipSuccess) return nullptr;
        (void)hipMemsetAsync(ctx->dbg_counters, 0, MAREX_DBG_COUNTERS * sizeof(unsigned long long), ctx->stream);
    }
    return ctx->dbg_counters;
}

static inline int device_cus(marex_ctx* ctx) {
    if (ctx->n_cu <= 0) {
        int n = 0;
        if (hipDeviceGetAttribute(&n, hipDeviceAttributeMultiprocessorCount, ctx->device) != hipSuccess || n <= 0) n = 256;
        ctx->n_cu = n;
    }
    return ctx->n_cu;
}

static inline int fail(marex_ctx* ctx, int code, const char* fmt, ...) {
    char buf[512];
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(buf, sizeof buf, fmt, ap);
    va_end(ap);
    if (ctx) ctx->err = buf;
    return code;
}

#define HIP_TRY(ctx, expr)                                                                      \
    do {                                                                                        \
        hipError_t e__ = (expr);                                                                \
        if (e__ != hipSuccess) return fail(ctx, -2, "%s failed: %s", #expr, hipGetErrorString(e__)); \
    } while (0)

// Grow a device scratch buffer of the context (pointer and its size field) to at least `need` bytes; the old contents are
// not kept.  Returns the HIP error for HIP_TRY: after a failed hipMalloc the buffer is empty (null, 0 bytes), after a failed
// hipFree it is as it was.
template <typename T>
static inline hipError_t grow_scratch(T*& buf, size_t& bytes, size_t need) {
    if (need <= bytes) return hipSuccess;
    if (buf) {
        const hipError_t e = hipFree(buf);
        if (e != hipSuccess) return e;
    }
    buf = nullptr;
    bytes = 0;
    const hipError_t e = hipMalloc((void**)&buf, need);
    if (e == hipSuccess) bytes = need;
    return e;
}

struct LaunchTimer {
    marex_ctx* ctx;
    int kid;
    hipEvent_t a = nullptr, b = nullptr;
    LaunchTimer(marex_ctx* c, int k) : ctx(c), kid(k) {
        if (ctx->timing) {
            (void)hipEventCreate(&a);
            (void)hipEventCreate(&b);
            (void)hipEventRecord(a, ctx->stream);
        }
    }
    ~LaunchTimer() {
        if (ctx->timing) {
            (void)hipEventRecord(b, ctx->stream);
            ctx->pending.push_back({kid, a, b});
        }
    }
};

static inline void drain_timers(marex_ctx* ctx) {
    for (auto& p : ctx->pending) {
        float ms = 0.f;
        (void)hipEventSynchronize(p.b);
        if (hipEventElapsedTime(&ms, p.a, p.b) == hipSuccess) {
            ctx->total_ms[p.kid] += ms;
            ctx->launches[p.kid] += 1;
        }
        (void)hipEventDestroy(p.a);
        (void)hipEventDestroy(p.b);
    }
    ctx->pending.clear();
}

// ------------------------------------------------------------------------------------------------
// device helpers
// ------------------------------------------------------------------------------------------------
__device__ __forceinline__ float nan_f() { return __builtin_nanf(""); }
__device__ __forceinline__ bool finite_f(float v) { return fabsf(v) <= 3.402823466e+38f; }
// The same answer on every input (an all-ones exponent is exactly NaN and +-inf) from the bits: what the event and cell
// statistics were written with; finite_f stays for the anomaly and shifting kernels, whose instructions are pinned.
__device__ __forceinline__ bool finite_bits(float v) { return (__float_as_uint(v) & 0x7F800000u) != 0x7F800000u; }

// The class of a finite anomaly a under the threshold h: 5 where h is not a positive finite number, else the number of
// h, 2 h, 3 h, 4 h (float32 products, one rounding each, ascending) that a reaches.
__device__ __forceinline__ int severity_class(float a, float h) {
    if (!(h > 0.f) || !finite_bits(h)) return 5;
    const float h2 = 2.f * h, h3 = 3.f * h, h4 = 4.f * h;
    return (int)(a >= h) + (int)(a >= h2) + (int)(a >= h3) + (int)(a >= h4);
}

// index of key v in keys[0 .. n) (ascending, distinct), -1 when absent
__device__ __forceinline__ int sorted_find(const int* __restrict__ keys, int n, int v) {
    int lo = 0, hi = n - 1;
    while (lo <= hi) {
        const int mid = lo + ((hi - lo) >> 1);
        const int k = keys[mid];
        if (k == v) return mid;
        if (k < v) lo = mid + 1; else hi = mid - 1;
    }
    return -1;
}

// splitmix64 finaliser: neighbouring pair keys land far apart in the table
__device__ __forceinline__ u64 splitmix64(u64 k) {
    k ^= k >> 30; k *= 0xbf58476d1ce4e5b9ull;
    k ^= k >> 27; k *= 0x94d049bb133111ebull;
    return k ^ (k >> 31);
}

// The keyed tables of marex_event_exposure.hip and marex_event_matching.hip: keys u64 [cap], cap a power of two, 0 = empty,
// linear probing from the splitmix64 home.  The entry of `key` (claimed by one CAS if it is new), or -1 after cap probes:
// bounded, so a full table is the caller's status and never a spin.
__device__ __forceinline__ long table_claim(u64* __restrict__ keys, long cap, u64 key) {
    const u64 mask = (u64)cap - 1;
    u64 h = splitmix64(key) & mask;
    long p = 0;
    for (; p < cap; ++p) {
        const u64 prev = atomicCAS(&keys[h], 0ull, key);
        if (prev == 0ull || prev == key) break;
        h = (h + 1) & mask;
    }
    return p < cap ? (long)h : -1L;
}

// The occupied entries of such a table -> the out arrays, in no particular order; status[ST_OUT] = how many there are (more
// than out_cap: the caller's sizing error, nothing is written past out_cap).  area, and sums with vmax, may be absent.
template <int ST_OUT>
__global__ void __launch_bounds__(256)
k_table_compact(long cap, const u64* __restrict__ keys, const u64* __restrict__ cnt, const u64* __restrict__ area,
                const double* __restrict__ sums, const unsigned* __restrict__ vmax, long out_cap, u64* __restrict__ status,
                u64* __restrict__ out_keys, u64* __restrict__ out_cnt, u64* __restrict__ out_area, double* __restrict__ out_sums,
                unsigned* __restrict__ out_vmax) {
    for (long h = (long)blockIdx.x * 256 + threadIdx.x; h < cap; h += (long)gridDim.x * 256) {
        const u64 k = keys[h];
        if (!k) continue;
        const u64 p = atomicAdd(&status[ST_OUT], 1ull);
        if (p >= (u64)out_cap) continue;
        out_keys[p] = k;
        out_cnt[p] = cnt[h];
        if (area) out_area[p] = area[h];
        if (sums) {
            out_sums[2 * p] = sums[2 * h];
            out_sums[2 * p + 1] = sums[2 * h + 1];
            out_vmax[p] = vmax[h];
        }
    }
}

// blocks of 256 threads of a grid-stride loop over n items
static inline unsigned stride_grid(long n) { return (unsigned)(n < 256L * 8192 ? (n + 255) / 256 : 8192); }

// The strided-row grid over a [T][C] field: a column of workgroups per `chunk` cells of a row, min(T, tstride) of them per
// column, each striding over the rows by gridDim.y.  The chunk (a register budget) and the row stride are the unit's own.
static inline dim3 slice_grid(long T, long C, long chunk, int tstride) {
    return dim3((unsigned)((C + chunk - 1) / chunk), (unsigned)(T < tstride ? T : tstride));
}

// What the (timestep, event) slot entry points refuse alike (`ptrs`: the entry point's own are there); `tail` ends the sentence.
static inline int evt_slot_args(marex_ctx* ctx, const char* name, bool ptrs, const void* ev_tmin, const void* ev_off, int64_t t0,
                                int64_t Tb, int64_t C, int n_ev, int64_t n_slots, const char* tail = " or no slot") {
    if (!ptrs || !ev_tmin || !ev_off || t0 < 0 || Tb <= 0 || C <= 0 || n_ev <= 0 || n_slots <= 0)
        return fail(ctx, -1, "%s: null pointer, empty shape, no event%s", name, tail);
    return 0;
}

// rows and steps are addressed through int: 0 where they fit, else the entry point's failure
static inline int cell_stream_limits(marex_ctx* ctx, const char* name, int64_t t0, int64_t Tb, int64_t C) {
    if (C >= 2147483647L || t0 >= 2147483647L || Tb >= 2147483647L || t0 + Tb >= 2147483647L)
        return fail(ctx, -4, "%s: a row or the time axis has 2^31 - 1 or more entries", name);
    return 0;
}

// Workgroups are dealt round-robin over the 8 XCDs (b % 8).  Map the linear block id so that the
// `inner` consecutive work items of one `outer` group (which re-read each other's rows) land on the
// same XCD / L2.  Returns false for padding blocks.
__device__ __forceinline__ bool xcd_swizzle(unsigned b, int n_outer, int n_inner, int& outer, int& inner) {
    unsigned xcd = b & 7u;
    unsigned k = b >> 3;
    inner = (int)(k % (unsigned)n_inner);
    outer = (int)((k / (unsigned)n_inner) * 8u + xcd);
    return outer < n_outer;
}
static inline unsigned xcd_grid(int n_outer, int n_inner) { return (unsigned)(((n_outer + 7) / 8) * 8) * (unsigned)n_inner; }

// Bin matrix layout: blocks of 16 consecutive cells, inside a block the dayofyear-sorted rows are
// contiguous: element (row r, cell c) at ((c >> 4) * T_out + r) * 16 + (c & 15).  The threshold kernel's
// 16-cell-wide tile rows then read whole contiguous runs (a tile row's entire day window) instead of
// 32 bytes out of every 128-byte line of a row-major [T_out, C] matrix (measured: 17x over-fetch).
__device__ __forceinline__ size_t bins_index(long r, long c, long T_out) {
    return ((size_t)(c >> 4) * (size_t)T_out + (size_t)r) * 16 + (size_t)(c & 15);
}

// np.digitize(v, edges) - 1 for an increasing table edges[0..nb] with edges[0] = -inf  (contract C4).
// The guess assumes equal-width bins above edges[1]; the two correction loops make it exact for any
// increasing table.
__device__ __forceinline__ int digitize_bin(float v, const float* e, int nb, float inv_width) {
    // straight-line: NaN / out-of-range inputs run through with a clamped guess and are fixed by selects at the end
    // the guess is clamped as a FLOAT: converting +-inf / huge values to int and adding 1 is signed-overflow UB, which
    // the compiler turned into an unclamped index (NaN clamps to 0)
    int k = 1 + (int)fminf(fmaxf((v - e[1]) * inv_width, 0.0f), (float)(nb - 2));
    k = k < 1 ? 1 : (k > nb - 1 ? nb - 1 : k);
    k += (v >= e[k + 1]) - (v < e[k]);  // the guess is off by at most one for equal-width tables
    k = k < 1 ? 1 : (k > nb - 1 ? nb - 1 : k);
    const bool inside = v >= e[1] && v < e[nb];
    if (inside && !(v >= e[k] && v < e[k + 1])) {  // arbitrary increasing tables: walk (never taken for uniform bins)
        while (k > 1 && v < e[k]) --k;
        while (k < nb - 1 && v >= e[k + 1]) ++k;
    }
    k = v < e[1] ? 0 : k;
    return (v >= e[nb] || !(v == v)) ? nb : k;
}

// Same result without touching memory, for tables that equal NumPy's float32 arange bit for bit:
// edges[j] = fl32(first + fl32(fl32(j-1) * delta)) for j >= 1 (separately rounded multiply and add, which is what
// -ffp-contract=off compiles to).  Whether a table has that form is checked once per workgroup (edges_are_arange).
__device__ __forceinline__ float arange_edge(int j, float first, float delta) { return first + (float)(j - 1) * delta; }

__device__ __forceinline__ int digitize_arange(float v, float first, float delta, float e_last, int nb, float inv_width) {
    int k = 1 + (int)fminf(fmaxf((v - first) * inv_width, 0.0f), (float)(nb - 2));  // float clamp: see digitize_bin
    k = k < 1 ? 1 : (k > nb - 1 ? nb - 1 : k);
    k += (v >= arange_edge(k + 1, first, delta)) - (v < arange_edge(k, first, delta));
    k = k < 1 ? 1 : (k > nb - 1 ? nb - 1 : k);
    const bool inside = v >= first && v < e_last;
    if (inside && !(v >= arange_edge(k, first, delta) && v < arange_edge(k + 1, first, delta))) {
        while (k > 1 && v < arange_edge(k, first, delta)) --k;
        while (k < nb - 1 && v >= arange_edge(k + 1, first, delta)) ++k;
    }
    k = v < first ? 0 : k;
    return (v >= e_last || !(v == v)) ? nb : k;
}

// block-wide: does the LDS copy e[0..nb] of the edge table have the arange form?  (all threads must call)
__device__ __forceinline__ bool edges_are_arange(const float* e, int nb) {
    const float first = e[1], delta = e[2] - e[1];
    bool ok = delta > 0.f;
    for (int j = 1 + (int)threadIdx.x; j <= nb; j += (int)blockDim.x)
        ok = ok && (__float_as_uint(e[j]) == __float_as_uint(arange_edge(j, first, delta)));
    return __syncthreads_and(ok ? 1 : 0) != 0;
}

__device__ __forceinline__ unsigned ordered_key(float v) {
    unsigned b = __float_as_uint(v);
    return (b & 0x80000000u) ? ~b : (b | 0x80000000u);
}

__device__ __forceinline__ unsigned hist_get(const unsigned* h, int b, int lane) {
    return (h[(b >> 1) * 64 + lane] >> ((b & 1) * 16)) & 0xFFFFu;  // [dword][64 lanes], two uint16 counters per dword
}

__device__ __forceinline__ void wave_sync() {
    __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
    __builtin_amdgcn_wave_barrier();
}

__device__ __forceinline__ float key_to_float(unsigned k) {
    return __uint_as_float((k & 0x80000000u) ? (k & 0x7FFFFFFFu) : ~k);
}

// min / max of an int over the 64 lanes of the wave, in every lane (DPP inside the rows of 16, two cross-row shuffles): one LDS
// atomic per WAVE instead of one per lane on a shared address (64 lanes on one address are 64 serial LDS operations)
__device__ __forceinline__ int wave_min_i32(int m) {
    int o;
    o = __builtin_amdgcn_update_dpp(m, m, 0x128, 0xF, 0xF, false); m = o < m ? o : m;  // row_ror 8 / 4 / 2 / 1
    o = __builtin_amdgcn_update_dpp(m, m, 0x124, 0xF, 0xF, false); m = o < m ? o : m;
    o = __builtin_amdgcn_update_dpp(m, m, 0x122, 0xF, 0xF, false); m = o < m ? o : m;
    o = __builtin_amdgcn_update_dpp(m, m, 0x121, 0xF, 0xF, false); m = o < m ? o : m;
    o = __shfl_xor(m, 16, 64); m = o < m ? o : m;
    o = __shfl_xor(m, 32, 64); m = o < m ? o : m;
    return m;
}
__device__ __forceinline__ int wave_max_i32(int m) { return -wave_min_i32(-m); }

// the sum of v over the 64 lanes of the wave, in every lane (a shuffle butterfly; double, long long or unsigned)
template <typename T>
__device__ __forceinline__ T wave_sum(T v) {
    for (int o = 32; o; o >>= 1) v += __shfl_xor(v, o, 64);
    return v;
}

// The same sum, and a maximum, for kernels that reduce often (marex_regional.hip, marex_event_exposure.hip): inside the rows
// of 16 lanes by DPP rotations (row_ror 8 / 4 / 2 / 1: after them every lane holds its row's result), across the four rows
// by two shuffles, as wave_min_i32 does -- two LDS permutes per word where the butterfly takes six.  CTRL: the DPP control
// word, 0x120 + n = row_ror n.  Every lane of the wave must be active.
template <int CTRL, typename T>
__device__ __forceinline__ T dpp_row_ror(T v) {
    if constexpr (sizeof(T) == 4) {
        const int u = __builtin_bit_cast(int, v);
        return __builtin_bit_cast(T, __builtin_amdgcn_update_dpp(u, u, CTRL, 0xF, 0xF, false));
    } else {
        static_assert(sizeof(T) == 8, "32- or 64-bit values");
        const u64 u = __builtin_bit_cast(u64, v);
        const int lo = (int)(unsigned)u, hi = (int)(unsigned)(u >> 32);
        const unsigned l2 = (unsigned)__builtin_amdgcn_update_dpp(lo, lo, CTRL, 0xF, 0xF, false);
        const unsigned h2 = (unsigned)__builtin_amdgcn_update_dpp(hi, hi, CTRL, 0xF, 0xF, false);
        return __builtin_bit_cast(T, ((u64)h2 << 32) | l2);
    }
}

// the sum of v over the 64 lanes, in every lane (unsigned, u64, long long or double)
template <typename T>
__device__ __forceinline__ T dpp_wave_sum(T v) {
    v += dpp_row_ror<0x128>(v);
    v += dpp_row_ror<0x124>(v);
    v += dpp_row_ror<0x122>(v);
    v += dpp_row_ror<0x121>(v);
    v += __shfl_xor(v, 16, 64);
    v += __shfl_xor(v, 32, 64);
    return v;
}

__device__ __forceinline__ unsigned dpp_wave_max_u32(unsigned v) {
    unsigned o;
    o = dpp_row_ror<0x128>(v); v = o > v ? o : v;
    o = dpp_row_ror<0x124>(v); v = o > v ? o : v;
    o = dpp_row_ror<0x122>(v); v = o > v ? o : v;
    o = dpp_row_ror<0x121>(v); v = o > v ? o : v;
    o = (unsigned)__shfl_xor((int)v, 16, 64); v = o > v ? o : v;
    o = (unsigned)__shfl_xor((int)v, 32, 64); v = o > v ? o : v;
    return v;
}

// v of lane src, in every lane
__device__ __forceinline__ u64 wave_shfl_u64(u64 v, int src) {
    const unsigned lo = __shfl((unsigned)v, src, 64), hi = __shfl((unsigned)(v >> 32), src, 64);
    return ((u64)hi << 32) | lo;
}

#define MASK_DOY_CHUNKS 6  // default number of pieces the dayofyear axis is cut into by the doy-grouped streaming kernels
