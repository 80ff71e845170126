// marex_event_shapes.hip -- per-(timestep, event) shape sums of a tracked, gridded ID field: second moments, bounding box and
// exposed sides (the reference hands bbox, perimeter, eccentricity, orientation and the axis lengths to regionprops_table;
// the side count and the orientation convention here are this project's own).  One streaming pass of the shape of
// k_evt_intensity (marex_intensity.hip) over the int32 event IDs; the four neighbours, the mask bytes and the table rows
// are fetched only under the cells that belong to an event.
//
// Arithmetic contract: every accumulator is an integer, added with 64-bit integer atomics or raised / lowered with 32-bit
// atomicMin / atomicMax, so nothing depends on the order in which waves arrive or on the time blocks.
//
// Bounds of the accumulators (mom, u64 per slot): the entry point refuses ny or nx above SHP_MAX_SIDE = 2^16 and a slice of
// 2^31 - 1 cells or more.  With n <= ny nx < 2^31 cells in a slot: sum x^2 <= nx^2 n < 2^32 2^31 = 2^63, sum y^2 likewise, and
// sum x y <= (x y) n < 2^31 2^31 = 2^62 (x y < ny nx).  The first moments and the counts are below 2^47.  Intermediate terms
// of a group may wrap; two's complement addition brings the exact sum back.  The table sums (lengths, areas) are bounded by
// the caller's fixed-point scale: no sum of them reaches 2^62.
#include "marex_common.hip.h"

#define SHP_ITERS 16                  // 64-cell pieces per wave
#define SHP_BATCH 4                   // pieces loaded together; SHP_ITERS is a multiple
#define SHP_CHUNK (256 * SHP_ITERS)   // cells of a row per workgroup (4 waves)
#define SHP_TSTRIDE 64                // rows in flight: a workgroup walks every SHP_TSTRIDE-th row
#define SHP_MOM 16                    // u64 per slot (include/marex_hip.h has the layout)
#define SHP_BOX 6                     // int32 per slot
#define SHP_MAX_SIDE 65536
#define SHP_INT_MAX 2147483647

__device__ __forceinline__ int shp_wave_max_i32(int m) { return ~wave_min_i32(~m); }

// the sum of v over the 64 lanes, in every lane: DPP rotations inside the rows of 16, two cross-row shuffles (the shape of
// wave_min_i32); every lane of the wave must be active
__device__ __forceinline__ unsigned shp_wave_sum_u32(unsigned v) {
    int s = (int)v;
    s += __builtin_amdgcn_update_dpp(s, s, 0x128, 0xF, 0xF, false);  // row_ror 8 / 4 / 2 / 1
    s += __builtin_amdgcn_update_dpp(s, s, 0x124, 0xF, 0xF, false);
    s += __builtin_amdgcn_update_dpp(s, s, 0x122, 0xF, 0xF, false);
    s += __builtin_amdgcn_update_dpp(s, s, 0x121, 0xF, 0xF, false);
    s += __shfl_xor(s, 16, 64);
    s += __shfl_xor(s, 32, 64);
    return (unsigned)__builtin_amdgcn_readfirstlane(s);
}

// a value that is the same in every lane, as a uniform one
__device__ __forceinline__ int shp_uniform(int v) { return __builtin_amdgcn_readfirstlane(v); }
__device__ __forceinline__ long long shp_uniform(long long v) {
    const unsigned lo = (unsigned)__builtin_amdgcn_readfirstlane((int)(unsigned)v);
    const unsigned hi = (unsigned)__builtin_amdgcn_readfirstlane((int)(unsigned)((u64)v >> 32));
    return (long long)(((u64)hi << 32) | lo);
}

// Rows t0 .. t0 + Tb - 1 of the field, ids [Tb][ny * nx]; the slots are those of k_evt_intensity.  A wave walks SHP_ITERS
// consecutive 64-cell pieces of a slice, SHP_BATCH at a time: the IDs of the batch are loaded first; in a piece that holds an
// event cell, the lanes under one then load their four neighbours (and, with MASK, the neighbours' mask bytes) -- a piece
// without an event costs its one cache line.  Every neighbour index is formed from a (y, x) inside the grid and a side that
// is not on the border, so it lies in 0 .. ny nx - 1.  The lanes of a piece are grouped by event (ballot); inside a piece lane
// l is cell r0 + l, so with (y0, x0) the coordinates of r0 and dy = y - y0 <= 63 a cell has x = x0 + l - nx dy, and the
// moments of a group follow from the wave sums of l, dy, l^2, dy^2 and l dy (packed into three 32-bit words).  The side
// counts are popcounts of ballots; the side lengths are those counts per row times the row's table entries.  The run of an
// event is carried across the pieces in uniform registers and flushed once, when the event changes; zero-valued terms are
// not sent.  The slot index is checked against the event's own span and n_slots before it addresses anything; a run outside
// adds its cells to status[0] instead.
template <bool MASK, bool TABLES>
__global__ void __launch_bounds__(256)
k_evt_shapes(const int* __restrict__ ids, long t0, long Tb, int ny, int nx, int regional, int n_ev,
             const int* __restrict__ ev_tmin, const long long* __restrict__ ev_off, long long n_slots,
             const unsigned char* __restrict__ mask, const long long* __restrict__ area_q, const long long* __restrict__ ns_q,
             const long long* __restrict__ ew_q, u64* __restrict__ mom, int* __restrict__ box, u64* __restrict__ status) {
    // what is equal in every lane is said to be so (readfirstlane): the run's 64-bit sums are then scalar arithmetic
    const int lane = threadIdx.x & 63, wave = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    const long C = (long)ny * nx;
    const long rw = (long)blockIdx.x * SHP_CHUNK + (long)wave * (64 * SHP_ITERS);
    const int half = nx / 2, right0 = nx - 100;
    const long long lnx = nx;
    for (long row = blockIdx.y; row < Tb; row += gridDim.y) {
        const int* irow = ids + row * C;
        const long long t = t0 + row;
        int cur = 0;
        long long n = 0, sy = 0, sx = 0, nr = 0, syy = 0, sxx = 0, sxy = 0, srx = 0, sry = 0;
        long long ens = 0, eew = 0, ebd = 0, ecs = 0, slen = 0, sarea = 0;
        unsigned fl = 0;
        int ylo = SHP_INT_MAX, yhi = -1, xlo_l = SHP_INT_MAX, xhi_l = -1, xlo_r = SHP_INT_MAX, xhi_r = -1;
        auto flush = [&]() {
            if (cur <= 0) return;  // wave-uniform
            const int tm = ev_tmin[cur];
            const long long o0 = ev_off[cur], o1 = ev_off[cur + 1];
            const long long s = o0 + (t - tm);
            if (t < tm || o0 < 0 || s >= o1 || s >= n_slots) {  // outside the declared span: counted, not accumulated
                if (lane == 0) atomicAdd(status, (u64)n);
                return;
            }
            if (lane != 0) return;
            u64* p = mom + (size_t)s * SHP_MOM;
            atomicAdd(p + 0, (u64)n);
            if (sy) atomicAdd(p + 1, (u64)sy);
            if (sx) atomicAdd(p + 2, (u64)sx);
            if (nr) atomicAdd(p + 3, (u64)nr);
            if (fl) atomicOr(p + 4, (u64)fl);
            if (syy) atomicAdd(p + 5, (u64)syy);
            if (sxx) atomicAdd(p + 6, (u64)sxx);
            if (sxy) atomicAdd(p + 7, (u64)sxy);
            if (srx) atomicAdd(p + 8, (u64)srx);
            if (sry) atomicAdd(p + 9, (u64)sry);
            if (ens) atomicAdd(p + 10, (u64)ens);
            if (eew) atomicAdd(p + 11, (u64)eew);
            if (ebd) atomicAdd(p + 12, (u64)ebd);
            if (ecs) atomicAdd(p + 13, (u64)ecs);
            if (slen) atomicAdd(p + 14, (u64)slen);
            if (sarea) atomicAdd(p + 15, (u64)sarea);
            int* q = box + (size_t)s * SHP_BOX;
            atomicMin(q + 0, ylo);
            atomicMax(q + 1, yhi);
            if (xhi_l >= 0) {
                atomicMin(q + 2, xlo_l);
                atomicMax(q + 3, xhi_l);
            }
            if (xhi_r >= 0) {
                atomicMin(q + 4, xlo_r);
                atomicMax(q + 5, xhi_r);
            }
        };
#pragma unroll 1
        for (int b = 0; b < SHP_ITERS; b += SHP_BATCH) {
            if (rw + 64 * b >= C) break;  // wave-uniform
            int ev[SHP_BATCH], yy[SHP_BATCH], xx[SHP_BATCH];
            int vn[SHP_BATCH], vs[SHP_BATCH], vw[SHP_BATCH], ve[SHP_BATCH];
            unsigned mk[SHP_BATCH];  // with MASK, bits 0 .. 3: the north, south, west, east neighbour is inside and land
            long long aqv[SHP_BATCH];
#pragma unroll
            for (int k = 0; k < SHP_BATCH; ++k) {
                const long r = rw + 64 * (b + k) + lane;
                const int v = r < C ? irow[r] : 0;
                ev[k] = (v > 0 && v <= n_ev) ? v : 0;  // ev_tmin / ev_off are never indexed by an unchecked value
            }
#pragma unroll
            for (int k = 0; k < SHP_BATCH; ++k) {
                yy[k] = xx[k] = 0;
                vn[k] = vs[k] = vw[k] = ve[k] = -1;  // -1: outside the domain (differs from every event)
                mk[k] = 0;
                aqv[k] = 0;
                if (!__ballot(ev[k] > 0)) continue;  // wave-uniform: no event in the piece, nothing more is fetched
                const long r0 = rw + 64 * (b + k);
                const unsigned ur = (unsigned)r0 + lane, unx = (unsigned)nx;  // r0 + 63 < C + 64 < 2^32
                const unsigned y = ur / unx;
                const int x = (int)(ur - y * unx);
                yy[k] = (int)y;
                xx[k] = x;
                if (ev[k] > 0) {  // implies r < C, so 0 <= y < ny and 0 <= x < nx
                    const long r = r0 + lane;
                    const bool in_n = y > 0, in_s = (int)y < ny - 1;
                    const bool in_w = x > 0 || !regional, in_e = x < nx - 1 || !regional;
                    const long rn = r - nx, rs = r + nx;
                    const long rwst = x > 0 ? r - 1 : r + nx - 1, rest = x < nx - 1 ? r + 1 : r - nx + 1;  // periodic at the seam
                    if (in_n) vn[k] = irow[rn];
                    if (in_s) vs[k] = irow[rs];
                    if (in_w) vw[k] = irow[rwst];
                    if (in_e) ve[k] = irow[rest];
                    if (TABLES && area_q) aqv[k] = area_q[r];
                    if (MASK) {
                        unsigned m = 0;
                        if (in_n && mask[rn] == 0) m |= 1u;
                        if (in_s && mask[rs] == 0) m |= 2u;
                        if (in_w && mask[rwst] == 0) m |= 4u;
                        if (in_e && mask[rest] == 0) m |= 8u;
                        mk[k] = m;
                    }
                }
            }
#pragma unroll  // the per-piece values must stay in registers: no dynamic indexing
            for (int k = 0; k < SHP_BATCH; ++k) {
                const int e = ev[k];
                u64 todo = __ballot(e > 0);
                if (!todo) continue;
                const bool act = e > 0;
                const long r0 = rw + 64 * (b + k);
                const int y = yy[k], x = xx[k];
                const long long y0 = shp_uniform((int)((unsigned)r0 / (unsigned)nx)), x0 = (long long)r0 - y0 * lnx;
                const unsigned dy = (unsigned)(y - (int)y0);
                const bool xn = act && vn[k] != e, xs = act && vs[k] != e, xw = act && vw[k] != e, xe = act && ve[k] != e;
                const bool on_n = y == 0, on_s = y == ny - 1, on_w = regional && x == 0, on_e = regional && x == nx - 1;
                const u64 b_n = __ballot(xn), b_s = __ballot(xs), b_w = __ballot(xw), b_e = __ballot(xe);
                const u64 o_n = __ballot(xn && on_n), o_s = __ballot(xs && on_s), o_w = __ballot(xw && on_w),
                          o_e = __ballot(xe && on_e);
                u64 c_n = 0, c_s = 0, c_w = 0, c_e = 0;
                if (MASK) {
                    const unsigned m = mk[k];  // a neighbour outside the domain has no bit
                    c_n = __ballot(xn && (m & 1u));
                    c_s = __ballot(xs && (m & 2u));
                    c_w = __ballot(xw && (m & 4u));
                    c_e = __ballot(xe && (m & 8u));
                }
                const u64 b_right = __ballot(act && x > half);
                const u64 b_left_band = __ballot(act && x < 100);
                const u64 b_right_band = __ballot(act && x >= right0);
                const long long aq = aqv[k];
                const unsigned pa = (unsigned)lane | (dy << 16);
                // l dy <= 63 * 63 is split at bit 6: over 64 lanes each part sums below 2^12, each square below 2^18
                const unsigned ldy = (unsigned)lane * dy;
                const unsigned pb = (unsigned)(lane * lane) | ((ldy & 63u) << 18), pc = (dy * dy) | ((ldy >> 6) << 18);
                while (todo) {
                    const int lead = __ffsll((long long)todo) - 1;
                    const int el = shp_uniform(__shfl(e, lead, 64));
                    const u64 same = __ballot(e == el) & todo;
                    todo &= ~same;
                    const bool me = (same >> lane) & 1ull;
                    const u64 right = same & b_right, left = same & ~b_right;
                    const unsigned s1 = shp_wave_sum_u32(me ? pa : 0u), s2 = shp_wave_sum_u32(me ? pb : 0u),
                                   s4 = shp_wave_sum_u32(me ? pc : 0u);
                    const long long c = __popcll(same), sl = s1 & 0xFFFFu, sdy = s1 >> 16;
                    const long long sll = s2 & 0x3FFFFu, sdd = s4 & 0x3FFFFu, sld = (long long)(s2 >> 18) + 64 * (long long)(s4 >> 18);
                    long long cr = 0, gsrx = 0, gsry = 0;
                    if (right) {  // wave-uniform
                        const unsigned s3 = shp_wave_sum_u32(((right >> lane) & 1ull) ? pa : 0u);
                        const long long rl = s3 & 0xFFFFu, rdy = s3 >> 16;
                        cr = __popcll(right);
                        gsrx = cr * x0 + rl - lnx * rdy;
                        gsry = cr * y0 + rdy;
                    }
                    // the box of the group: y grows with the lane; x does too where the group lies in one row
                    const int first = __ffsll((long long)same) - 1, last = 63 - __clzll((long long)same);
                    const int gy0 = shp_uniform(__shfl(y, first, 64)), gy1 = shp_uniform(__shfl(y, last, 64));
                    long long glen = 0, garea = 0;
                    if (TABLES) {
                        // the lengths depend on the row alone: per row of the group (its lanes are lo .. hi - 1 of the piece, and
                        // every row between the group's first and last has a lane in the piece) the side counts times the row's
                        // table entries, in uniform registers; a group without an exposed side fetches nothing
                        const u64 g_n = same & b_n, g_s = same & b_s, g_w = same & b_w, g_e = same & b_e;
                        if (ns_q && (g_n | g_s | g_w | g_e)) {
                            for (int yr = gy0; yr <= gy1; ++yr) {
                                long lo = (long)yr * nx - r0, hi = lo + nx;
                                lo = lo < 0 ? 0 : lo;
                                hi = hi > 64 ? 64 : hi;  // 0 <= lo < hi <= 64
                                const u64 rm = (hi == 64 ? ~0ull : ((1ull << hi) - 1)) & ~((1ull << lo) - 1);
                                const long long side = __popcll(g_w & rm) + __popcll(g_e & rm);
                                if (g_n & rm) glen += __popcll(g_n & rm) * ns_q[yr];
                                if (g_s & rm) glen += __popcll(g_s & rm) * ns_q[yr + 1];
                                if (side) glen += side * ew_q[yr];
                            }
                        }
                        if (area_q) garea = shp_uniform(wave_sum(me ? aq : 0ll));
                    }
                    int gl0 = SHP_INT_MAX, gl1 = -1, gr0 = SHP_INT_MAX, gr1 = -1;
                    if (gy0 == gy1) {
                        if (left) {
                            gl0 = shp_uniform(__shfl(x, __ffsll((long long)left) - 1, 64));
                            gl1 = shp_uniform(__shfl(x, 63 - __clzll((long long)left), 64));
                        }
                        if (right) {
                            gr0 = shp_uniform(__shfl(x, __ffsll((long long)right) - 1, 64));
                            gr1 = shp_uniform(__shfl(x, 63 - __clzll((long long)right), 64));
                        }
                    } else {
                        const bool ml = (left >> lane) & 1ull, mr = (right >> lane) & 1ull;
                        gl0 = shp_uniform(wave_min_i32(ml ? x : SHP_INT_MAX));
                        gl1 = shp_uniform(shp_wave_max_i32(ml ? x : -1));
                        gr0 = shp_uniform(wave_min_i32(mr ? x : SHP_INT_MAX));
                        gr1 = shp_uniform(shp_wave_max_i32(mr ? x : -1));
                    }
                    if (el != cur) {
                        flush();
                        cur = el;
                        n = sy = sx = nr = syy = sxx = sxy = srx = sry = 0;
                        ens = eew = ebd = ecs = slen = sarea = 0;
                        fl = 0;
                        ylo = xlo_l = xlo_r = SHP_INT_MAX;
                        yhi = xhi_l = xhi_r = -1;
                    }
                    const long long rx = sl - lnx * sdy;                          // sum of x - x0
                    const long long rxx = sll - 2 * lnx * sld + lnx * lnx * sdd;  // sum of (x - x0)^2
                    const long long rxy = sld - lnx * sdd;                        // sum of (x - x0) dy
                    n += c;
                    sy += c * y0 + sdy;
                    sx += c * x0 + rx;
                    nr += cr;
                    syy += c * y0 * y0 + 2 * y0 * sdy + sdd;
                    sxx += c * x0 * x0 + 2 * x0 * rx + rxx;
                    sxy += c * x0 * y0 + x0 * sdy + y0 * rx + rxy;
                    srx += gsrx;
                    sry += gsry;
                    ens += __popcll(same & b_n) + __popcll(same & b_s);
                    eew += __popcll(same & b_w) + __popcll(same & b_e);
                    ebd += __popcll(same & o_n) + __popcll(same & o_s) + __popcll(same & o_w) + __popcll(same & o_e);
                    if (MASK) ecs += __popcll(same & c_n) + __popcll(same & c_s) + __popcll(same & c_w) + __popcll(same & c_e);
                    slen += glen;
                    sarea += garea;
                    fl |= ((same & b_left_band) ? 1u : 0u) | ((same & b_right_band) ? 2u : 0u);
                    ylo = gy0 < ylo ? gy0 : ylo;
                    yhi = gy1 > yhi ? gy1 : yhi;
                    xlo_l = gl0 < xlo_l ? gl0 : xlo_l;
                    xhi_l = gl1 > xhi_l ? gl1 : xhi_l;
                    xlo_r = gr0 < xlo_r ? gr0 : xlo_r;
                    xhi_r = gr1 > xhi_r ? gr1 : xhi_r;
                }
            }
        }
        flush();
    }
}

extern "C" int marex_event_shapes_i32(marex_ctx* ctx, const int32_t* ids, int64_t t0, int64_t Tb, int ny, int nx, int regional,
                                      int n_ev, const int32_t* ev_tmin, const int64_t* ev_off, int64_t n_slots,
                                      const uint8_t* mask, const int64_t* area_q, const int64_t* ns_q, const int64_t* ew_q,
                                      uint64_t* mom, int32_t* box, uint64_t* status) {
    if (!ctx) return -1;
    // the edge tables come as a pair or not at all, which counts with the pointers; the cells of a row are given by two sides
    if (const int rc = evt_slot_args(ctx, "marex_event_shapes_i32", ids && mom && box && status && (ns_q == nullptr) == (ew_q == nullptr),
                                     ev_tmin, ev_off, t0, Tb, /* C > 0 */ ny > 0 && nx > 0 ? 1 : 0, n_ev, n_slots,
                                     ", no slot, or half a pair of edge tables"))
        return rc;
    if (ny > SHP_MAX_SIDE || nx > SHP_MAX_SIDE)
        return fail(ctx, -4, "marex_event_shapes_i32: a grid side above %d (the second moments are 64-bit sums)", SHP_MAX_SIDE);
    const int64_t C = (int64_t)ny * nx;
    if (const int rc = cell_stream_limits(ctx, "marex_event_shapes_i32", t0, Tb, C)) return rc;
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    LaunchTimer lt(ctx, MAREX_K_MORPH);
    const dim3 grid = slice_grid(Tb, C, SHP_CHUNK, SHP_TSTRIDE);
    const bool tables = area_q || ns_q;
#define SHP_LAUNCH(M, W)                                                                                                    \
    hipLaunchKernelGGL((k_evt_shapes<M, W>), grid, dim3(256), 0, ctx->stream, ids, (long)t0, (long)Tb, ny, nx, regional, n_ev, \
                       ev_tmin, (const long long*)ev_off, (long long)n_slots, mask, (const long long*)area_q,               \
                       (const long long*)ns_q, (const long long*)ew_q, (u64*)mom, box, (u64*)status)
    if (mask && tables) SHP_LAUNCH(true, true);
    else if (mask) SHP_LAUNCH(true, false);
    else if (tables) SHP_LAUNCH(false, true);
    else SHP_LAUNCH(false, false);
#undef SHP_LAUNCH
    HIP_TRY(ctx, hipGetLastError());
    return 0;
}
