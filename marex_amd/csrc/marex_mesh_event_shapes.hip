// marex_mesh_event_shapes.hip -- per-(timestep, event) shape sums of a tracked ID field on an unstructured mesh of three-sided
// cells: the weighted first and second moments of the cells' unit vectors, a latitude / longitude box in integer keys and the
// exposed sides over the three neighbour slots (nothing of this exists in the reference; the definitions are this project's
// own, marex_amd/shapes_mesh.py).  One streaming pass of the shape of k_evt_shapes (marex_event_shapes.hip) over the int32
// event IDs; the neighbour indices, the neighbours' IDs and mask bytes, the ten table rows, the side lengths and the two
// coordinate keys are fetched only under the cells that belong to an event.
//
// Arithmetic contract: every accumulator is an integer, added with 64-bit integer atomics or raised / lowered with 32-bit
// atomicMin / atomicMax, so nothing depends on the order in which waves arrive or on the time blocks.
//
// Bounds: the caller scales the ten rows of q so that the sum of any row over any set of cells stays below 2^62 in magnitude
// (rows 1 .. 9 are signed: a partial sum is two's complement arithmetic in a u64), and the side lengths so that the sum over
// any set of (slot, cell) sides, each counted once, does.  A cell counts a side at most once per slot, and the counts are
// below 3 * 2^31.
#include "marex_common.hip.h"

#define MSH_ITERS 16                  // 64-cell pieces per wave
#define MSH_BATCH 4                   // pieces whose IDs and neighbours are loaded together; MSH_ITERS is a multiple
#define MSH_CHUNK (256 * MSH_ITERS)   // cells of a row per workgroup (4 waves)
#define MSH_TSTRIDE 64                // rows in flight: a workgroup walks every MSH_TSTRIDE-th row
#define MSH_MOM 16                    // u64 per slot (include/marex_hip.h has the layout)
#define MSH_BOX 6                     // int32 per slot
#define MSH_ROWS 10                   // rows of q
#define MSH_INT_MAX 2147483647
#define MSH_INT_MIN (-2147483647 - 1)
// per-lane side flags of a piece, one bit per neighbour slot k = 0 .. 2
#define MSH_F_EXPOSED 0x001u
#define MSH_F_BORDER 0x008u
#define MSH_F_COAST 0x040u
#define MSH_F_CONTACT 0x200u

__device__ __forceinline__ int msh_wave_max_i32(int m) { return ~wave_min_i32(~m); }

// a value that is the same in every lane, as a uniform one
__device__ __forceinline__ int msh_uniform(int v) { return __builtin_amdgcn_readfirstlane(v); }
__device__ __forceinline__ long long msh_uniform(long long v) {
    const unsigned lo = (unsigned)__builtin_amdgcn_readfirstlane((int)(unsigned)v);
    const unsigned hi = (unsigned)__builtin_amdgcn_readfirstlane((int)(unsigned)((u64)v >> 32));
    return (long long)(((u64)hi << 32) | lo);
}

// Rows t0 .. t0 + Tb - 1 of the field, ids [Tb][C]; the slots are those of k_evt_intensity.  A wave walks MSH_ITERS consecutive
// 64-cell pieces of a slice, MSH_BATCH at a time: the IDs of the batch are loaded first; in a piece that holds an event cell,
// the lanes under one then gather their three neighbour indices, the neighbours' IDs (and, with MASK, mask bytes; with LEN,
// the lengths of the exposed sides) -- a piece without an event costs its one cache line.  A neighbour index outside
// 0 .. C - 1 is "no neighbour" whatever its value, so nothing is read out of bounds even from a corrupt table.  The ten table
// values and the two keys of a piece are loaded when it is reduced.  The lanes of a piece are grouped by event (ballot); the
// 64-bit sums of a group are wave reductions, the side counts popcounts of ballots.  The run of an event is carried across
// the pieces in uniform registers and flushed once, when the event changes; zero-valued terms are not sent.  The slot index
// is checked against the event's own span and n_slots before it addresses anything; a run outside adds its cells to
// status[0] instead.
template <bool MASK, bool LEN>
__global__ void __launch_bounds__(256)
k_mesh_evt_shapes(const int* __restrict__ ids, long t0, long Tb, long C, int n_ev, const int* __restrict__ ev_tmin,
                  const long long* __restrict__ ev_off, long long n_slots, const int* __restrict__ nbr,
                  const unsigned char* __restrict__ mask, const long long* __restrict__ q, const long long* __restrict__ len_q,
                  const int* __restrict__ lat_k, const int* __restrict__ lon_k, u64* __restrict__ mom, int* __restrict__ box,
                  u64* __restrict__ status) {
    const int lane = threadIdx.x & 63, wave = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    const long rw = (long)blockIdx.x * MSH_CHUNK + (long)wave * (64 * MSH_ITERS);
    for (long row = blockIdx.y; row < Tb; row += gridDim.y) {
        const int* irow = ids + row * C;
        const long long t = t0 + row;
        int cur = 0;
        long long n = 0, sq[MSH_ROWS], eex = 0, ebd = 0, ecs = 0, ect = 0, slen = 0;
#pragma unroll
        for (int i = 0; i < MSH_ROWS; ++i) sq[i] = 0;
        int la0 = MSH_INT_MAX, la1 = MSH_INT_MIN, w0 = MSH_INT_MAX, w1 = MSH_INT_MIN, e0 = MSH_INT_MAX, e1 = MSH_INT_MIN;
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
            u64* p = mom + (size_t)s * MSH_MOM;
            atomicAdd(p + 0, (u64)n);
#pragma unroll
            for (int i = 0; i < MSH_ROWS; ++i)
                if (sq[i]) atomicAdd(p + 1 + i, (u64)sq[i]);
            if (eex) atomicAdd(p + 11, (u64)eex);
            if (ebd) atomicAdd(p + 12, (u64)ebd);
            if (ecs) atomicAdd(p + 13, (u64)ecs);
            if (slen) atomicAdd(p + 14, (u64)slen);
            if (ect) atomicAdd(p + 15, (u64)ect);
            if (lat_k) {
                int* b = box + (size_t)s * MSH_BOX;
                atomicMin(b + 0, la0);
                atomicMax(b + 1, la1);
                if (w0 <= w1) {
                    atomicMin(b + 2, w0);
                    atomicMax(b + 3, w1);
                }
                if (e0 <= e1) {
                    atomicMin(b + 4, e0);
                    atomicMax(b + 5, e1);
                }
            }
        };
#pragma unroll 1
        for (int b = 0; b < MSH_ITERS; b += MSH_BATCH) {
            if (rw + 64 * b >= C) break;  // wave-uniform
            int ev[MSH_BATCH];
            unsigned fl[MSH_BATCH];
            long long sl[MSH_BATCH];  // with LEN, the length of the lane's exposed sides
#pragma unroll
            for (int k = 0; k < MSH_BATCH; ++k) {
                const long r = rw + 64 * (b + k) + lane;
                const int v = r < C ? irow[r] : 0;
                ev[k] = (v > 0 && v <= n_ev) ? v : 0;  // ev_tmin / ev_off are never indexed by an unchecked value
            }
#pragma unroll
            for (int k = 0; k < MSH_BATCH; ++k) {
                fl[k] = 0;
                sl[k] = 0;
                if (!__ballot(ev[k] > 0)) continue;  // wave-uniform: no event in the piece, nothing more is fetched
                if (ev[k] > 0) {                     // implies r < C
                    const long r = rw + 64 * (b + k) + lane;
                    const int e = ev[k];
                    int j[3], v[3];
                    bool in[3];
#pragma unroll
                    for (int s = 0; s < 3; ++s) {
                        j[s] = nbr[(long)s * C + r];
                        in[s] = j[s] >= 0 && (long)j[s] < C;
                    }
#pragma unroll
                    for (int s = 0; s < 3; ++s) v[s] = in[s] ? irow[j[s]] : 0;
                    unsigned f = 0;
#pragma unroll
                    for (int s = 0; s < 3; ++s) {
                        if (!in[s]) f |= (MSH_F_EXPOSED | MSH_F_BORDER) << s;
                        else if (v[s] != e) {
                            f |= MSH_F_EXPOSED << s;
                            if (v[s] > 0) f |= MSH_F_CONTACT << s;
                            if (MASK && mask[j[s]] == 0) f |= MSH_F_COAST << s;
                        }
                    }
                    if (LEN) {
                        long long l = 0;
#pragma unroll
                        for (int s = 0; s < 3; ++s)
                            if (f & (MSH_F_EXPOSED << s)) l += len_q[(long)s * C + r];
                        sl[k] = l;
                    }
                    fl[k] = f;
                }
            }
#pragma unroll  // the per-piece values must stay in registers: no dynamic indexing
            for (int k = 0; k < MSH_BATCH; ++k) {
                const int e = ev[k];
                u64 todo = __ballot(e > 0);
                if (!todo) continue;
                const bool act = e > 0;
                const long r = rw + 64 * (b + k) + lane;
                const unsigned f = fl[k];
                u64 bex[3], bbd[3], bcs[3], bct[3];
#pragma unroll
                for (int s = 0; s < 3; ++s) {
                    bex[s] = __ballot((f & (MSH_F_EXPOSED << s)) != 0);
                    bbd[s] = __ballot((f & (MSH_F_BORDER << s)) != 0);
                    bcs[s] = MASK ? __ballot((f & (MSH_F_COAST << s)) != 0) : 0ull;
                    bct[s] = __ballot((f & (MSH_F_CONTACT << s)) != 0);
                }
                long long qv[MSH_ROWS];
#pragma unroll
                for (int i = 0; i < MSH_ROWS; ++i) qv[i] = act ? q[(long)i * C + r] : 0ll;
                int la = 0, lo = 0;
                if (lat_k && act) {
                    la = lat_k[r];
                    lo = lon_k[r];
                }
                while (todo) {
                    const int lead = __ffsll((long long)todo) - 1;
                    const int el = msh_uniform(__shfl(e, lead, 64));
                    const u64 same = __ballot(e == el) & todo;
                    todo &= ~same;
                    const bool me = (same >> lane) & 1ull;
                    long long g[MSH_ROWS], gl = 0;
#pragma unroll
                    for (int i = 0; i < MSH_ROWS; ++i) g[i] = msh_uniform(dpp_wave_sum(me ? qv[i] : 0ll));
                    if (LEN) gl = msh_uniform(dpp_wave_sum(me ? sl[k] : 0ll));
                    int gla0 = MSH_INT_MAX, gla1 = MSH_INT_MIN, gw0 = MSH_INT_MAX, gw1 = MSH_INT_MIN, ge0 = MSH_INT_MAX,
                        ge1 = MSH_INT_MIN;
                    if (lat_k) {  // wave-uniform
                        const bool west = me && lo < 0, east = me && lo >= 0;
                        gla0 = msh_uniform(wave_min_i32(me ? la : MSH_INT_MAX));
                        gla1 = msh_uniform(msh_wave_max_i32(me ? la : MSH_INT_MIN));
                        if (__ballot(west)) {
                            gw0 = msh_uniform(wave_min_i32(west ? lo : MSH_INT_MAX));
                            gw1 = msh_uniform(msh_wave_max_i32(west ? lo : MSH_INT_MIN));
                        }
                        if (__ballot(east)) {
                            ge0 = msh_uniform(wave_min_i32(east ? lo : MSH_INT_MAX));
                            ge1 = msh_uniform(msh_wave_max_i32(east ? lo : MSH_INT_MIN));
                        }
                    }
                    if (el != cur) {
                        flush();
                        cur = el;
                        n = eex = ebd = ecs = ect = slen = 0;
#pragma unroll
                        for (int i = 0; i < MSH_ROWS; ++i) sq[i] = 0;
                        la0 = w0 = e0 = MSH_INT_MAX;
                        la1 = w1 = e1 = MSH_INT_MIN;
                    }
                    n += __popcll(same);
#pragma unroll
                    for (int i = 0; i < MSH_ROWS; ++i) sq[i] += g[i];
#pragma unroll
                    for (int s = 0; s < 3; ++s) {
                        eex += __popcll(same & bex[s]);
                        ebd += __popcll(same & bbd[s]);
                        if (MASK) ecs += __popcll(same & bcs[s]);
                        ect += __popcll(same & bct[s]);
                    }
                    slen += gl;
                    la0 = gla0 < la0 ? gla0 : la0;
                    la1 = gla1 > la1 ? gla1 : la1;
                    w0 = gw0 < w0 ? gw0 : w0;
                    w1 = gw1 > w1 ? gw1 : w1;
                    e0 = ge0 < e0 ? ge0 : e0;
                    e1 = ge1 > e1 ? ge1 : e1;
                }
            }
        }
        flush();
    }
}

extern "C" int marex_mesh_event_shapes_i64(marex_ctx* ctx, const int32_t* ids, int64_t t0, int64_t Tb, int64_t C, int n_ev,
                                           const int32_t* ev_tmin, const int64_t* ev_off, int64_t n_slots, const int32_t* nbr,
                                           const uint8_t* mask, const int64_t* q, const int64_t* len_q, const int32_t* lat_k,
                                           const int32_t* lon_k, uint64_t* mom, int32_t* box, uint64_t* status) {
    if (!ctx) return -1;
    // the two coordinate keys come as a pair or not at all, which counts with the pointers
    if (const int rc = evt_slot_args(ctx, "marex_mesh_event_shapes_i64",
                                     ids && nbr && q && mom && box && status && (lat_k == nullptr) == (lon_k == nullptr), ev_tmin,
                                     ev_off, t0, Tb, C, n_ev, n_slots, ", no slot, or one coordinate key without the other"))
        return rc;
    if (const int rc = cell_stream_limits(ctx, "marex_mesh_event_shapes_i64", t0, Tb, C)) return rc;
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    LaunchTimer lt(ctx, MAREX_K_MORPH);
    const dim3 grid = slice_grid(Tb, C, MSH_CHUNK, MSH_TSTRIDE);
#define MSH_LAUNCH(M, L)                                                                                                       \
    hipLaunchKernelGGL((k_mesh_evt_shapes<M, L>), grid, dim3(256), 0, ctx->stream, ids, (long)t0, (long)Tb, (long)C, n_ev,      \
                       ev_tmin, (const long long*)ev_off, (long long)n_slots, nbr, mask, (const long long*)q,                  \
                       (const long long*)len_q, lat_k, lon_k, (u64*)mom, box, (u64*)status)
    if (mask && len_q) MSH_LAUNCH(true, true);
    else if (mask) MSH_LAUNCH(true, false);
    else if (len_q) MSH_LAUNCH(false, true);
    else MSH_LAUNCH(false, false);
#undef MSH_LAUNCH
    HIP_TRY(ctx, hipGetLastError());
    return 0;
}
