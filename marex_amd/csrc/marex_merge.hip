// marex_merge.hip -- the device stages of the reference's merge tracker on grids (marEx/track.py:2554-3802, 4826-5113):
// partition of merging children by the nearest parent centroid or the nearest parent cell, relabelling of ID fields
// through a sorted (or dense) old -> new table, and the per-(timestep, event) pass behind area, centroid and global_ID of
// cluster_rename_objects_and_props.
//
// The host drives the per-timestep loop of split_and_merge_objects: per step only the overlap tables and the small
// child -> parents tables cross PCIe; the ID field stays in HBM.  Distances are float64 sqrt(dy * dy + dx * dx), compiled
// with -ffp-contract=off, so no fused multiply-add can move a tie; the reference's first minimum (np.argmin / strict <)
// is kept by scanning parents in order with a strict comparison.
#include "marex_common.hip.h"

#define MRG_NMOM 5  // int64 per event slot: cell count, sum y, sum x, sum of x with x > nx / 2 shifted by -nx, near-edge flags
#define MRG_NWMOM 4 // float64 per event slot (weighted): area, sum a y, sum a x, sum a x_shifted

// the x offset of a child cell to a parent point, wrapped by +-nx when |dx| > nx / 2 (wrapped_euclidian_distance_*)
__device__ __forceinline__ double mrg_dist(double dy, double dx, double nx, bool wrap) {
    if (wrap) {
        if (dx > 0.5 * nx) dx -= nx;
        else if (dx < -0.5 * nx) dx += nx;
    }
    return sqrt(dy * dy + dx * dx);
}

// ids[i] -> vals[j] where keys[j] == ids[i] (sorted table, n_keys entries) or vals[ids[i]] for 0 < ids[i] < n_keys
// (dense table, keys == nullptr); IDs without an entry (and background) are left as they are.
__global__ void __launch_bounds__(256)
k_mrg_relabel(int* __restrict__ ids, long n, const int* __restrict__ keys, const int* __restrict__ vals, int n_keys) {
    for (long i = (long)blockIdx.x * 256 + threadIdx.x; i < n; i += (long)gridDim.x * 256) {
        const int v = ids[i];
        if (v <= 0) continue;
        if (keys) {
            const int j = sorted_find(keys, n_keys, v);
            if (j >= 0) ids[i] = vals[j];
        } else if (v < n_keys) {
            ids[i] = vals[v];
        }
    }
}

// Centroid partition of every merging child of one iteration in one launch: child k (child_keys[k], ascending) has the
// parent entries off[k] .. off[k + 1] with centroids (pcy, pcx) and the labels lab; each child cell takes the label of
// the first nearest centroid.
__global__ void __launch_bounds__(256)
k_mrg_part_centroid(int* __restrict__ ids, int ny, int nx, const int* __restrict__ child_keys, int n_child,
                    const int* __restrict__ off, const double* __restrict__ pcy, const double* __restrict__ pcx,
                    const int* __restrict__ lab, int wrap) {
    const long C = (long)ny * nx;
    for (long i = (long)blockIdx.x * 256 + threadIdx.x; i < C; i += (long)gridDim.x * 256) {
        const int v = ids[i];
        if (v <= 0) continue;
        const int k = sorted_find(child_keys, n_child, v);
        if (k < 0) continue;
        const double y = (double)(i / nx), x = (double)(i % nx);
        int best = off[k];
        double bd = __builtin_huge_val();
        for (int j = off[k]; j < off[k + 1]; ++j) {
            const double d = mrg_dist(y - pcy[j], x - pcx[j], (double)nx, wrap != 0);
            if (d < bd) {
                bd = d;
                best = j;
            }
        }
        ids[i] = lab[best];
    }
}

// Buckets of the parent cells for the nearest-neighbour partition.  Entry j (a parent of one merging child) has bucket
// size gs[j], ngx[j] buckets per row and its buckets at base[j] ..; parent ID par_keys[q] (ascending) owns the entries
// pent[poff[q] .. poff[q + 1]) (a parent of several merging children has one entry per child).
// FILL = false: cnt[bucket] += 1 per (cell, entry); FILL = true: cell index written at cur[bucket]++ (cur = the bucket
// starts on entry).
template <bool FILL>
__global__ void __launch_bounds__(256)
k_mrg_nn_buckets(const int* __restrict__ prev, int ny, int nx, const int* __restrict__ par_keys, int n_par,
                 const int* __restrict__ poff, const int* __restrict__ pent, const int* __restrict__ gs,
                 const int* __restrict__ ngy, const int* __restrict__ ngx, const long long* __restrict__ base,
                 long long* __restrict__ cnt, int* __restrict__ cells, long long n_cells) {
    const long C = (long)ny * nx;
    for (long i = (long)blockIdx.x * 256 + threadIdx.x; i < C; i += (long)gridDim.x * 256) {
        const int v = prev[i];
        if (v <= 0) continue;
        const int q = sorted_find(par_keys, n_par, v);
        if (q < 0) continue;
        const int y = (int)(i / nx), x = (int)(i % nx);
        for (int e = poff[q]; e < poff[q + 1]; ++e) {
            const int j = pent[e], g = gs[j];
            const int by = min(y / g, ngy[j] - 1), bx = min(x / g, ngx[j] - 1);
            const long long b = base[j] + (long long)by * ngx[j] + bx;
            if (FILL) {
                const long long p = (long long)atomicAdd((u64*)&cnt[b], 1ull);
                if (p < n_cells) cells[p] = (int)i;
            } else {
                atomicAdd((u64*)&cnt[b], 1ull);
            }
        }
    }
}

// exclusive scan of cnt[0 .. n) into start[0 .. n], start[n] = the total, by one workgroup
__global__ void __launch_bounds__(1024) k_mrg_scan(const long long* __restrict__ cnt, long n, long long* __restrict__ start) {
    __shared__ long long part[1024];
    const long per = (n + 1023) / 1024;
    const long a = threadIdx.x * per < n ? threadIdx.x * per : n, b = a + per < n ? a + per : n;
    long long s = 0;
    for (long j = a; j < b; ++j) s += cnt[j];
    part[threadIdx.x] = s;
    __syncthreads();
    for (int d = 1; d < 1024; d <<= 1) {
        const long long v = threadIdx.x >= (unsigned)d ? part[threadIdx.x - d] : 0;
        __syncthreads();
        part[threadIdx.x] += v;
        __syncthreads();
    }
    long long run = part[threadIdx.x] - s;
    for (long j = a; j < b; ++j) {
        start[j] = run;
        run += cnt[j];
    }
    if (threadIdx.x == 1023) start[n] = part[1023];
}

// Nearest-neighbour partition (partition_nn_grid, track.py:4972-5113) of every merging child of one iteration: for each
// parent entry j of the cell's child, in order, the candidates are the cells of that parent in the 3 x 3 buckets around
// the cell's bucket (bucket indices modulo the bucket counts in y and x, as the reference does even in regional mode)
// within maxd[j]; the parent with the smallest distance wins, the first on a tie (the reference's early exit at distance
// 0 chooses the same parent).  A cell without candidates takes the first nearest centroid.  bstart = the bucket starts
// (k_mrg_scan), cells = the parent cells bucket by bucket.
__global__ void __launch_bounds__(256)
k_mrg_part_nn(int* __restrict__ ids, int ny, int nx, const int* __restrict__ child_keys, int n_child,
              const int* __restrict__ off, const double* __restrict__ pcy, const double* __restrict__ pcx,
              const int* __restrict__ lab, const int* __restrict__ gs, const int* __restrict__ ngy,
              const int* __restrict__ ngx, const int* __restrict__ maxd, const long long* __restrict__ base,
              const long long* __restrict__ bstart, const int* __restrict__ cells, int wrap) {
    const long C = (long)ny * nx;
    for (long i = (long)blockIdx.x * 256 + threadIdx.x; i < C; i += (long)gridDim.x * 256) {
        const int v = ids[i];
        if (v <= 0) continue;
        const int k = sorted_find(child_keys, n_child, v);
        if (k < 0) continue;
        const int y = (int)(i / nx), x = (int)(i % nx);
        const double inf = __builtin_huge_val();
        int best = -1;
        double bd = inf;
        for (int j = off[k]; j < off[k + 1]; ++j) {
            const int g = gs[j], gy = ngy[j], gx = ngx[j];
            const int by = min(y / g, gy - 1), bx = min(x / g, gx - 1);
            const double md = (double)maxd[j];
            double m = inf;
            for (int dy = -1; dy <= 1; ++dy) {
                const int cy = ((by + dy) % gy + gy) % gy;
                for (int dx = -1; dx <= 1; ++dx) {
                    const int cx = ((bx + dx) % gx + gx) % gx;
                    const long long b = base[j] + (long long)cy * gx + cx;
                    for (long long p = bstart[b]; p < bstart[b + 1]; ++p) {
                        const int c = cells[p];
                        const double d = mrg_dist((double)(y - c / nx), (double)(x - c % nx), (double)nx, wrap != 0);
                        if (d <= md && d < m) m = d;
                    }
                }
            }
            if (m < bd) {
                bd = m;
                best = j;
            }
        }
        if (best < 0) {  // no parent cell within reach: the nearest centroid
            best = off[k];
            for (int j = off[k]; j < off[k + 1]; ++j) {
                const double d = mrg_dist((double)y - pcy[j], (double)x - pcx[j], (double)nx, wrap != 0);
                if (d < bd) {
                    bd = d;
                    best = j;
                }
            }
        }
        ids[i] = lab[best];
    }
}

__device__ __forceinline__ int mrg_wave_max_i32(int v) {
    for (int o = 32; o; o >>= 1) {
        const int w = __shfl_xor(v, o, 64);
        v = w > v ? w : v;
    }
    return v;
}

// Per-(timestep, event) slot t * n_ev + e - 1 of the event field ev (values 1 .. n_ev, 0 background): acc[slot][0..4]
// += cells, sum y, sum x, sum of x - (x > nx / 2 ? nx : 0), flags (1: a cell with x < 100, 2: one with x >= nx - 100);
// gid[slot] = max of the original IDs orig under the event's cells (the last of the reference's sorted unique pairs).
// With weights w (float32 per cell of a slice) also wacc[slot][0..3] += sum w, sum w y, sum w x, sum w x_shifted in
// float64.  A wave groups the lanes of one 64-cell piece by event (ballot) and sends one set of atomics per group.
__global__ void __launch_bounds__(256)
k_mrg_event_moments(const int* __restrict__ ev, const int* __restrict__ orig, long T, int ny, int nx, int n_ev,
                    const float* __restrict__ w, u64* __restrict__ acc, double* __restrict__ wacc, int* __restrict__ gid) {
    const int lane = threadIdx.x & 63;
    const long C = (long)ny * nx;
    const long pieces = (C + 63) / 64;
    const long wave0 = ((long)blockIdx.x * 256 + threadIdx.x) >> 6, nwaves = ((long)gridDim.x * 256) >> 6;
    for (long t = blockIdx.y; t < T; t += gridDim.y) {
        const int* er = ev + t * C;
        const int* orr = orig + t * C;
        for (long pc = wave0; pc < pieces; pc += nwaves) {
            const long r = pc * 64 + lane;
            const int e = r < C ? er[r] : 0;
            u64 todo = __ballot(e > 0 && e <= n_ev);
            if (!todo) continue;
            const int y = (int)(r / nx), x = (int)(r % nx);
            const int o = e > 0 ? orr[r] : 0;
            const float wc = (w && e > 0) ? w[r] : 0.f;
            const int xs = 2 * x > nx ? x - nx : x;
            const unsigned fl = (x < 100 ? 1u : 0u) | (x >= nx - 100 ? 2u : 0u);
            while (todo) {
                const int lead = __ffsll((long long)todo) - 1;
                const int el = __shfl(e, lead, 64);
                const u64 same = __ballot(e == el) & todo;
                todo &= ~same;
                const bool me = (same >> lane) & 1ull;
                const long long n = __popcll(same);
                const long long sy = wave_sum<long long>(me ? y : 0), sx = wave_sum<long long>(me ? x : 0),
                                sxs = wave_sum<long long>(me ? xs : 0);
                const u64 bl = __ballot(me && (fl & 1u)), br = __ballot(me && (fl & 2u));
                const int om = mrg_wave_max_i32(me ? o : 0);
                double wa = 0, wy = 0, wx = 0, wxs = 0;
                if (w) {
                    const double a = me ? (double)wc : 0.0;
                    wa = wave_sum(a);
                    wy = wave_sum(a * (double)y);
                    wx = wave_sum(a * (double)x);
                    wxs = wave_sum(a * (double)xs);
                }
                if (lane == 0) {
                    const size_t s = (size_t)t * n_ev + (el - 1);
                    u64* p = acc + s * MRG_NMOM;
                    atomicAdd(p + 0, (u64)n);
                    atomicAdd(p + 1, (u64)sy);
                    atomicAdd(p + 2, (u64)sx);
                    atomicAdd(p + 3, (u64)sxs);
                    const u64 f = (bl ? 1ull : 0ull) | (br ? 2ull : 0ull);
                    if (f) atomicOr(p + 4, f);
                    atomicMax(gid + s, om);
                    if (w) {
                        double* q = wacc + s * MRG_NWMOM;
                        atomicAdd(q + 0, wa);
                        atomicAdd(q + 1, wy);
                        atomicAdd(q + 2, wx);
                        atomicAdd(q + 3, wxs);
                    }
                }
            }
        }
    }
}

#define MRG_ITERS 16                  // 64-cell pieces per wave of the rename pass
#define MRG_BATCH 4                   // pieces loaded together (loads in flight per lane); MRG_ITERS is a multiple
#define MRG_CHUNK (256 * MRG_ITERS)   // cells of a slice per workgroup (4 waves)
#define MRG_TSTRIDE 64                // slices in flight: a workgroup walks every MRG_TSTRIDE-th slice

// cluster_rename_objects_and_props in one pass over the field, in place: ids[t][c] = e = lut[v] for 0 < v = ids[t][c] <
// lut_len (anything else, and an e outside 1 .. n_ev: 0), written back only where it differs, and for e > 0 the compact
// slot s = ev_off[e] + (t - ev_tmin[e]) takes the sums of k_mrg_event_moments (same definitions) and gid[s] = max v.
// A cell is read and written by one lane only.  A wave walks MRG_ITERS consecutive 64-cell pieces of a slice, groups the
// lanes of a piece by event (ballot) and carries the run of an event across its pieces in uniform registers (the pieces
// are loaded MRG_BATCH at a time: unrolling all of them costs more registers than the loads in flight are worth); the run is
// flushed once, when the event changes: lanes 0 .. 3 add the four integer sums (and the four float64 sums) of the slot as
// ONE wave instruction over 32 contiguous bytes each, lane 4 sets the flags, lane 5 the largest original ID -- the
// interior of a large event costs one set of atomics per 1024 cells, not one per piece.  The slot index is checked against
// the event's own span [ev_off[e], ev_off[e + 1]) and against n_slots before it addresses anything; a run outside it adds
// its cells to status[0] instead.
template <bool WEIGHTED>
__global__ void __launch_bounds__(256)
k_mrg_event_rename(int* ids, long T, int ny, int nx, const int* __restrict__ lut, long lut_len, int n_ev,
                   const int* __restrict__ ev_tmin, const long long* __restrict__ ev_off, long long n_slots,
                   const float* __restrict__ w, u64* __restrict__ acc, double* __restrict__ wacc, int* __restrict__ gid,
                   u64* __restrict__ status) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const long C = (long)ny * nx;
    const long rw = (long)blockIdx.x * MRG_CHUNK + (long)wave * (64 * MRG_ITERS);
    for (long t = blockIdx.y; t < T; t += gridDim.y) {
        int* row = ids + t * C;
        int cur = 0, big = 0;
        unsigned cfl = 0;
        long long n = 0, sy = 0, sx = 0, sxs = 0;
        double wa = 0, wy = 0, wx = 0, wxs = 0;
        auto flush = [&]() {
            if (cur <= 0) return;  // wave-uniform
            const int tm = ev_tmin[cur];
            const long long o0 = ev_off[cur], o1 = ev_off[cur + 1];
            const long long s = o0 + ((long long)t - tm);
            if (t < tm || o0 < 0 || s >= o1 || s >= n_slots) {  // outside the declared span: counted, not accumulated
                if (lane == 0) atomicAdd(status, (u64)n);
                return;
            }
            u64* p = acc + (size_t)s * MRG_NMOM;
            if (lane < 4) {
                atomicAdd(p + lane, (u64)(lane == 0 ? n : lane == 1 ? sy : lane == 2 ? sx : sxs));
                if (WEIGHTED) atomicAdd(wacc + (size_t)s * MRG_NWMOM + lane, lane == 0 ? wa : lane == 1 ? wy : lane == 2 ? wx : wxs);
            } else if (lane == 4) {
                if (cfl) atomicOr(p + 4, (u64)cfl);
            } else if (lane == 5) {
                atomicMax(gid + s, big);
            }
        };
#pragma unroll 1
        for (int b = 0; b < MRG_ITERS; b += MRG_BATCH) {
            if (rw + 64 * b >= C) break;  // wave-uniform
            int v[MRG_BATCH], ev[MRG_BATCH];
#pragma unroll
            for (int k = 0; k < MRG_BATCH; ++k) {
                const long r = rw + 64 * (b + k) + lane;
                v[k] = r < C ? row[r] : 0;
            }
#pragma unroll
            for (int k = 0; k < MRG_BATCH; ++k) {
                const long r = rw + 64 * (b + k) + lane;
                int e = (v[k] > 0 && (long)v[k] < lut_len) ? lut[v[k]] : 0;
                e = (e > 0 && e <= n_ev) ? e : 0;  // ev_tmin / ev_off below are never indexed by an unchecked value
                ev[k] = e;
                if (r < C && e != v[k]) row[r] = e;
            }
#pragma unroll  // v[k], ev[k] must stay in registers: no dynamic indexing
            for (int k = 0; k < MRG_BATCH; ++k) {
                const long r0 = rw + 64 * (b + k);
                if (r0 >= C) break;  // wave-uniform
                const int e = ev[k];
                u64 todo = __ballot(e > 0);
                if (!todo) continue;
                const unsigned r = (unsigned)(r0 + lane);  // below 2^31 - 1 wherever e > 0
                const int y = (int)(r / (unsigned)nx), x = (int)(r % (unsigned)nx);
                const int xs = 2 * x > nx ? x - nx : x;
                const unsigned fl = (x < 100 ? 1u : 0u) | (x >= nx - 100 ? 2u : 0u);
                float wc = 0.f;
                if (WEIGHTED && e > 0) wc = w[r0 + lane];  // e > 0 implies r0 + lane < C
                while (todo) {
                    const int lead = __ffsll((long long)todo) - 1;
                    const int el = __shfl(e, lead, 64);
                    const u64 same = __ballot(e == el) & todo;
                    todo &= ~same;
                    const bool me = (same >> lane) & 1ull;
                    const long long gy = wave_sum<long long>(me ? y : 0), gx = wave_sum<long long>(me ? x : 0),
                                    gxs = wave_sum<long long>(me ? xs : 0);
                    const u64 bl = __ballot(me && (fl & 1u)), br = __ballot(me && (fl & 2u));
                    const int gm = mrg_wave_max_i32(me ? v[k] : 0);  // v > 0 wherever e > 0
                    double ga = 0, gwy = 0, gwx = 0, gwxs = 0;
                    if (WEIGHTED) {
                        const double a = me ? (double)wc : 0.0;
                        ga = wave_sum(a);
                        gwy = wave_sum(a * (double)y);
                        gwx = wave_sum(a * (double)x);
                        gwxs = wave_sum(a * (double)xs);
                    }
                    if (el != cur) {
                        flush();
                        cur = el;
                        n = sy = sx = sxs = 0;
                        wa = wy = wx = wxs = 0;
                        big = 0;
                        cfl = 0;
                    }
                    n += __popcll(same);
                    sy += gy;
                    sx += gx;
                    sxs += gxs;
                    cfl |= (bl ? 1u : 0u) | (br ? 2u : 0u);
                    big = gm > big ? gm : big;
                    if (WEIGHTED) {
                        wa += ga;
                        wy += gwy;
                        wx += gwx;
                        wxs += gwxs;
                    }
                }
            }
        }
        flush();
    }
}


extern "C" int marex_relabel_i32(marex_ctx* ctx, int32_t* ids, int64_t n, const int32_t* keys, const int32_t* vals,
                                 int n_keys) {
    if (!ctx) return -1;
    if (!ids || !vals || n <= 0 || n_keys <= 0) return fail(ctx, -1, "marex_relabel_i32: null pointer or empty table");
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    LaunchTimer lt(ctx, MAREX_K_MORPH);
    hipLaunchKernelGGL(k_mrg_relabel, dim3(stride_grid(n)), dim3(256), 0, ctx->stream, ids, (long)n, keys, vals, n_keys);
    HIP_TRY(ctx, hipGetLastError());
    return 0;
}

extern "C" int marex_partition_centroid_i32(marex_ctx* ctx, int32_t* ids, int ny, int nx, const int32_t* child_keys,
                                            int n_child, const int32_t* off, const double* pcy, const double* pcx,
                                            const int32_t* lab, int wrap) {
    if (!ctx) return -1;
    if (!ids || !child_keys || !off || !pcy || !pcx || !lab || ny <= 0 || nx <= 0 || n_child <= 0)
        return fail(ctx, -1, "marex_partition_centroid_i32: null pointer, empty slice or no child");
    if ((long)ny * nx >= 2147483647L) return fail(ctx, -4, "marex_partition_centroid_i32: a slice has 2^31 - 1 or more cells");
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    LaunchTimer lt(ctx, MAREX_K_MORPH);
    hipLaunchKernelGGL(k_mrg_part_centroid, dim3(stride_grid((long)ny * nx)), dim3(256), 0, ctx->stream, ids, ny, nx, child_keys,
                       n_child, off, pcy, pcx, lab, wrap);
    HIP_TRY(ctx, hipGetLastError());
    return 0;
}

extern "C" int marex_nn_bucket_count_i32(marex_ctx* ctx, const int32_t* prev, int ny, int nx, const int32_t* par_keys,
                                         int n_par, const int32_t* poff, const int32_t* pent, const int32_t* gs,
                                         const int32_t* ngy, const int32_t* ngx, const int64_t* base, int64_t n_buckets,
                                         int64_t* cnt, int64_t* bstart) {
    if (!ctx) return -1;
    if (!prev || !par_keys || !poff || !pent || !gs || !ngy || !ngx || !base || !cnt || !bstart || ny <= 0 || nx <= 0 ||
        n_par <= 0 || n_buckets <= 0)
        return fail(ctx, -1, "marex_nn_bucket_count_i32: null pointer, empty slice or no parent");
    if ((long)ny * nx >= 2147483647L) return fail(ctx, -4, "marex_nn_bucket_count_i32: a slice has 2^31 - 1 or more cells");
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    LaunchTimer lt(ctx, MAREX_K_MORPH);
    HIP_TRY(ctx, hipMemsetAsync(cnt, 0, (size_t)n_buckets * sizeof(int64_t), ctx->stream));
    hipLaunchKernelGGL(k_mrg_nn_buckets<false>, dim3(stride_grid((long)ny * nx)), dim3(256), 0, ctx->stream, prev, ny, nx, par_keys,
                       n_par, poff, pent, gs, ngy, ngx, (const long long*)base, (long long*)cnt, (int*)nullptr, 0LL);
    hipLaunchKernelGGL(k_mrg_scan, dim3(1), dim3(1024), 0, ctx->stream, (const long long*)cnt, (long)n_buckets, (long long*)bstart);
    HIP_TRY(ctx, hipGetLastError());
    return 0;
}

extern "C" int marex_partition_nn_i32(marex_ctx* ctx, int32_t* ids, const int32_t* prev, int ny, int nx,
                                      const int32_t* par_keys, int n_par, const int32_t* poff, const int32_t* pent,
                                      const int32_t* child_keys, int n_child, const int32_t* off, const double* pcy,
                                      const double* pcx, const int32_t* lab, const int32_t* gs, const int32_t* ngy,
                                      const int32_t* ngx, const int32_t* maxd, const int64_t* base, int64_t n_buckets,
                                      const int64_t* bstart, int64_t* cursor, int32_t* cells, int64_t n_cells, int wrap) {
    if (!ctx) return -1;
    if (!ids || !prev || !par_keys || !poff || !pent || !child_keys || !off || !pcy || !pcx || !lab || !gs || !ngy || !ngx ||
        !maxd || !base || !bstart || !cursor || !cells || ny <= 0 || nx <= 0 || n_par <= 0 || n_child <= 0 ||
        n_buckets <= 0 || n_cells <= 0)
        return fail(ctx, -1, "marex_partition_nn_i32: null pointer, empty slice or empty table");
    if ((long)ny * nx >= 2147483647L) return fail(ctx, -4, "marex_partition_nn_i32: a slice has 2^31 - 1 or more cells");
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    LaunchTimer lt(ctx, MAREX_K_MORPH);
    HIP_TRY(ctx, hipMemcpyAsync(cursor, bstart, (size_t)n_buckets * sizeof(int64_t), hipMemcpyDeviceToDevice, ctx->stream));
    const unsigned g = stride_grid((long)ny * nx);
    hipLaunchKernelGGL(k_mrg_nn_buckets<true>, dim3(g), dim3(256), 0, ctx->stream, prev, ny, nx, par_keys, n_par, poff, pent, gs,
                       ngy, ngx, (const long long*)base, (long long*)cursor, cells, (long long)n_cells);
    hipLaunchKernelGGL(k_mrg_part_nn, dim3(g), dim3(256), 0, ctx->stream, ids, ny, nx, child_keys, n_child, off, pcy, pcx, lab,
                       gs, ngy, ngx, maxd, (const long long*)base, (const long long*)bstart, cells, wrap);
    HIP_TRY(ctx, hipGetLastError());
    return 0;
}

extern "C" int marex_event_moments_i32(marex_ctx* ctx, const int32_t* ev, const int32_t* orig, int64_t T, int ny, int nx,
                                       int n_ev, const float* w, uint64_t* acc, double* wacc, int32_t* gid) {
    if (!ctx) return -1;
    if (!ev || !orig || !acc || !gid || (w && !wacc) || T <= 0 || ny <= 0 || nx <= 0 || n_ev <= 0)
        return fail(ctx, -1, "marex_event_moments_i32: null pointer, empty field or no event");
    const long C = (long)ny * nx;
    if (C >= 2147483647L || T >= 2147483647L) return fail(ctx, -4, "marex_event_moments_i32: a slice or the time axis has 2^31 - 1 or more entries");
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    LaunchTimer lt(ctx, MAREX_K_MORPH);
    const size_t slots = (size_t)T * n_ev;
    HIP_TRY(ctx, hipMemsetAsync(acc, 0, slots * MRG_NMOM * sizeof(u64), ctx->stream));
    HIP_TRY(ctx, hipMemsetAsync(gid, 0, slots * sizeof(int32_t), ctx->stream));
    if (w) HIP_TRY(ctx, hipMemsetAsync(wacc, 0, slots * MRG_NWMOM * sizeof(double), ctx->stream));
    const long pieces = (C + 63) / 64;
    const unsigned gx = (unsigned)(pieces < 4L * 2048 ? (pieces + 3) / 4 : 2048);
    const unsigned gy = (unsigned)(T < 64 ? T : 64);
    hipLaunchKernelGGL(k_mrg_event_moments, dim3(gx, gy), dim3(256), 0, ctx->stream, ev, orig, (long)T, ny, nx, n_ev, w,
                       (u64*)acc, wacc, gid);
    HIP_TRY(ctx, hipGetLastError());
    return 0;
}

extern "C" int marex_event_rename_i32(marex_ctx* ctx, int32_t* ids, int64_t T, int ny, int nx, const int32_t* lut,
                                      int64_t lut_len, int n_ev, const int32_t* ev_tmin, const int64_t* ev_off,
                                      int64_t n_slots, const float* w, uint64_t* acc, double* wacc, int32_t* gid,
                                      uint64_t* status) {
    if (!ctx) return -1;
    if (!ids || !lut || !ev_tmin || !ev_off || !acc || !gid || !status || (w && !wacc) || T <= 0 || ny <= 0 || nx <= 0 ||
        lut_len <= 0 || n_ev <= 0 || n_slots <= 0)
        return fail(ctx, -1, "marex_event_rename_i32: null pointer, empty field, empty table or no slot");
    const long C = (long)ny * nx;
    if (C >= 2147483647L || T >= 2147483647L) return fail(ctx, -4, "marex_event_rename_i32: a slice or the time axis has 2^31 - 1 or more entries");
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    LaunchTimer lt(ctx, MAREX_K_MORPH);
    HIP_TRY(ctx, hipMemsetAsync(acc, 0, (size_t)n_slots * MRG_NMOM * sizeof(u64), ctx->stream));
    HIP_TRY(ctx, hipMemsetAsync(gid, 0, (size_t)n_slots * sizeof(int32_t), ctx->stream));
    HIP_TRY(ctx, hipMemsetAsync(status, 0, sizeof(u64), ctx->stream));
    if (w) HIP_TRY(ctx, hipMemsetAsync(wacc, 0, (size_t)n_slots * MRG_NWMOM * sizeof(double), ctx->stream));
    const dim3 grid = slice_grid(T, C, MRG_CHUNK, MRG_TSTRIDE);
    if (w)
        hipLaunchKernelGGL(k_mrg_event_rename<true>, grid, dim3(256), 0, ctx->stream, ids, (long)T, ny, nx, lut, (long)lut_len, n_ev,
                           ev_tmin, (const long long*)ev_off, (long long)n_slots, w, (u64*)acc, wacc, gid, (u64*)status);
    else
        hipLaunchKernelGGL(k_mrg_event_rename<false>, grid, dim3(256), 0, ctx->stream, ids, (long)T, ny, nx, lut, (long)lut_len, n_ev,
                           ev_tmin, (const long long*)ev_off, (long long)n_slots, w, (u64*)acc, wacc, gid, (u64*)status);
    HIP_TRY(ctx, hipGetLastError());
    return 0;
}
