// marex_cell_events.hip -- per-cell marine-heatwave events under the duration and gap rule of Hobday et al. (2016): a run of
// at least D consecutive present steps qualifies, qualifying runs at most G absent-or-short steps apart are one event, gap
// steps included.  One streaming pass over an event mask and, optionally, the anomaly field gives the per-cell event
// statistics by the group of the event's start step, the filtered mask, and (in a second pass, with per-cell offsets) one
// record per event.
//
// Layout (that of marex_occurrence.hip): a lane owns its cells for the whole call -- one cell, or without anomalies four
// consecutive uint8 cells through one 32-bit load -- and walks the rows CE_U1 / CE_U4 at a time.  The decision lags the data by D + G - 1
// steps, so each cell is a small state machine carried through time and, between windows, in memory (one [C] plane per
// variable): the run length, the open event's start and last qualifying step, the records written, and with anomalies two
// accumulators -- the EVENT (float64 sum, maximum, its step, invalid steps) and the TAIL, which covers the steps since the
// event's last qualifying step or, with no event open, the steps of the current run.  Steps of a qualified run go straight to
// the event; the tail joins it as ONE term when a run qualifies.  That order is fixed by the data alone: no window boundary
// changes a bit of a sum.  The anomalies are fetched only under present steps and under absent steps of an open event: the
// integer part of the state machine runs ahead over the batch to know which.  A lane writes only bytes it owns: no atomics
// (but for the status counters) and no LDS.  An emitted event is added to the [G][C] accumulators by a plain
// read-modify-write.
#include "marex_cellwalk.hip.h"

// rows loaded together of the one-cell and of the four-cell layout
#ifndef CE_U1
#define CE_U1 8
#endif
#ifndef CE_U4
#define CE_U4 4
#endif
// the int32 planes of the carried state: four always, all ten with anomalies
enum { CE_RUN, CE_START1, CE_END, CE_CURSOR, CE_EMAX, CE_ETMAX, CE_EINV, CE_TMAX, CE_TTMAX, CE_TINV };


// Rows t0 .. t0 + Tb - 1: x and anom [Tb][C]; mask is the base of the whole [T][C] output.  V: cells per lane (4: C % 4 == 0
// and x and mask are 4-byte aligned -- the entry point checks, and launches it without anomalies only); ANOM: anom and the
// float planes are given.
template <int V, bool ANOM>
__global__ void __launch_bounds__(256)
k_cell_events(const unsigned char* __restrict__ x, const float* __restrict__ anom, long t0, long Tb, long C, int D, int Gap,
              int finish, const int* __restrict__ grp, int G, int* sti, double* stf, unsigned* events, unsigned* event_days,
              unsigned* dur_max, double* sum, unsigned* vmax, unsigned* invalid, unsigned char* mask,
              const long long* __restrict__ rec_off, int* rec_start, int* rec_end, unsigned* rec_vmax, int* rec_tmax,
              double* rec_sum, unsigned* rec_invalid, u64* status) {
    typedef typename cell_word<unsigned char, V>::type W;
    constexpr int U = V == 4 ? CE_U4 : CE_U1;
    const long c0 = ((long)blockIdx.x * 256 + threadIdx.x) * V;
    if (c0 >= C) return;  // V == 4: C % 4 == 0, so all four cells exist; no ballots, so a lane may leave
    const size_t Cs = (size_t)C;
    unsigned run[V], cur[V], emax[V], einv[V], tmx[V], tinv[V];
    int st1[V], end[V], etm[V], ttm[V];  // st1: start + 1 of the open event, 0 for none
    double es[V], ts[V];
    unsigned bad = 0, over = 0;
#pragma unroll
    for (int j = 0; j < V; ++j) {
        const size_t c = c0 + j;
        run[j] = (unsigned)sti[CE_RUN * Cs + c];
        st1[j] = sti[CE_START1 * Cs + c];
        end[j] = sti[CE_END * Cs + c];
        cur[j] = (unsigned)sti[CE_CURSOR * Cs + c];
        emax[j] = einv[j] = tmx[j] = tinv[j] = 0;
        etm[j] = ttm[j] = 0;
        es[j] = ts[j] = 0.0;
        if (ANOM) {
            emax[j] = (unsigned)sti[CE_EMAX * Cs + c];
            etm[j] = sti[CE_ETMAX * Cs + c];
            einv[j] = (unsigned)sti[CE_EINV * Cs + c];
            tmx[j] = (unsigned)sti[CE_TMAX * Cs + c];
            ttm[j] = sti[CE_TTMAX * Cs + c];
            tinv[j] = (unsigned)sti[CE_TINV * Cs + c];
            es[j] = stf[c];
            ts[j] = stf[Cs + c];
        }
    }
    auto emit = [&](int j) {  // the open event of sub-cell j closes: accumulators of its start's group, its record
        const int s = st1[j] - 1, e = end[j];
        st1[j] = 0;
        const int g = grp ? grp[s] : 0;
        if (g < 0 || g >= G) {  // addresses nothing
            ++bad;
            return;
        }
        const size_t c = c0 + j;
        if (events) {
            const size_t o = (size_t)g * Cs + c;
            const unsigned d = (unsigned)(e - s + 1);
            events[o] += 1;
            event_days[o] += d;
            if (d > dur_max[o]) dur_max[o] = d;
            if (ANOM) {
                sum[o] += es[j];
                if (emax[j] > vmax[o]) vmax[o] = emax[j];
                invalid[o] += einv[j];
            }
        }
        if (rec_start) {
            const long long o = rec_off[c] + (long long)cur[j];
            if (o < rec_off[c + 1]) {
                rec_start[o] = s;
                rec_end[o] = e;
                if (ANOM) {
                    rec_vmax[o] = emax[j];
                    rec_tmax[o] = etm[j];
                    rec_sum[o] = es[j];
                    rec_invalid[o] = einv[j];
                }
            } else {
                ++over;  // more events than the offsets leave room for: counted, not written
            }
            ++cur[j];
        }
    };
    for (long r = 0; r < Tb; r += U) {
        W w[U];
        float av[U][V];
#pragma unroll
        for (int k = 0; k < U; ++k) w[k] = (r + k < Tb) ? *(const W*)(x + (size_t)(r + k) * Cs + c0) : (W)0;
        if (ANOM) {  // the integer state machine runs ahead: a step matters when it is present or lies in an open event
#pragma unroll
            for (int j = 0; j < V; ++j) {
                unsigned pr = run[j];
                bool po = st1[j] != 0;
                int pe = end[j];
#pragma unroll
                for (int k = 0; k < U; ++k) {
                    const int t = (int)(t0 + r + k);
                    const bool p = cell_value<V>(w[k], j) > 0;
                    if (p) {
                        if (++pr >= (unsigned)D) {
                            po = true;
                            pe = t;
                        }
                    } else {
                        pr = 0;
                        if (po && t - pe > Gap) po = false;
                    }
                    av[k][j] = ((p || po) && r + k < Tb) ? anom[(size_t)(r + k) * Cs + c0 + j] : 0.f;
                }
            }
        }
#pragma unroll  // w[k], av[k] must stay in registers: no dynamic indexing
        for (int k = 0; k < U; ++k) {
            if (r + k < Tb) {  // uniform
                const int t = (int)(t0 + r + k);
                unsigned mw = 0;
#pragma unroll
                for (int j = 0; j < V; ++j) {
                    const bool p = cell_value<V>(w[k], j) > 0;
                    const float a = ANOM ? av[k][j] : 0.f;
                    const bool fin = ANOM && finite_bits(a);
                    const unsigned key = ANOM ? ordered_key(a) : 0u;
                    bool to_tail = false;
                    if (p) {
                        ++run[j];
                        if (run[j] <= (unsigned)D) {
                            if (run[j] == 1 && !st1[j]) {  // a run starts with no event open: the tail restarts
                                ts[j] = 0.0;
                                tmx[j] = tinv[j] = 0;
                                ttm[j] = 0;
                            }
                            to_tail = true;
                        } else {  // a step of a qualified run: straight to the event
                            if (ANOM) {
                                if (fin) {
                                    es[j] += (double)a;
                                    if (key > emax[j]) {
                                        emax[j] = key;
                                        etm[j] = t;
                                    }
                                } else {
                                    ++einv[j];
                                }
                            }
                            end[j] = t;
                        }
                    } else {
                        run[j] = 0;
                        if (st1[j]) {
                            if (t - end[j] > Gap)
                                emit(j);
                            else
                                to_tail = true;
                        }
                    }
                    if (ANOM && to_tail) {
                        if (fin) {
                            ts[j] += (double)a;
                            if (key > tmx[j]) {
                                tmx[j] = key;
                                ttm[j] = t;
                            }
                        } else {
                            ++tinv[j];
                        }
                    }
                    if (p && run[j] == (unsigned)D) {  // the run qualifies: it opens an event or joins the open one
                        if (mask) {  // the steps of the event not marked yet, up to t - 1: bytes of this lane's column
                            for (long s = st1[j] ? (long)end[j] + 1 : (long)t - D + 1; s < t; ++s) mask[(size_t)s * Cs + c0 + j] = 1;
                        }
                        if (!st1[j]) {
                            st1[j] = t - D + 2;
                            es[j] = 0.0;
                            emax[j] = einv[j] = 0;
                            etm[j] = 0;
                        }
                        if (ANOM) {  // the tail joins the event as one term
                            es[j] += ts[j];
                            if (tmx[j] > emax[j]) {
                                emax[j] = tmx[j];
                                etm[j] = ttm[j];
                            }
                            einv[j] += tinv[j];
                            ts[j] = 0.0;
                            tmx[j] = tinv[j] = 0;
                            ttm[j] = 0;
                        }
                        end[j] = t;
                    }
                    mw |= (unsigned)(p && run[j] >= (unsigned)D) << (8 * j);
                }
                if (mask) *(W*)(mask + (size_t)t * Cs + c0) = (W)mw;
            }
        }
    }
    size_t Cw = Cs;
    asm volatile("" : "+s"(Cw));  // an empty statement: the plane addresses are formed again here, not kept through the loop
#pragma unroll
    for (int j = 0; j < V; ++j) {
        if (finish && st1[j]) emit(j);  // the record ends: an open event ends at its last qualifying step
        const size_t c = c0 + j;
        sti[CE_RUN * Cw + c] = (int)run[j];
        sti[CE_START1 * Cw + c] = st1[j];
        sti[CE_END * Cw + c] = end[j];
        sti[CE_CURSOR * Cw + c] = (int)cur[j];
        if (ANOM) {
            sti[CE_EMAX * Cw + c] = (int)emax[j];
            sti[CE_ETMAX * Cw + c] = etm[j];
            sti[CE_EINV * Cw + c] = (int)einv[j];
            sti[CE_TMAX * Cw + c] = (int)tmx[j];
            sti[CE_TTMAX * Cw + c] = ttm[j];
            sti[CE_TINV * Cw + c] = (int)tinv[j];
            stf[c] = es[j];
            stf[Cw + c] = ts[j];
        }
    }
    if (bad) atomicAdd(status, (u64)bad);
    if (over) atomicAdd(status + 1, (u64)over);
}

static inline bool ce_misaligned(const void* p, uintptr_t a) { return ((uintptr_t)p & (a - 1)) != 0; }

extern "C" int marex_cell_events_u8(marex_ctx* ctx, const uint8_t* x, const float* anom, int64_t t0, int64_t Tb, int64_t C,
                                    int min_duration, int max_gap, int finish, const int32_t* grp, int G, int32_t* state_i32,
                                    double* state_f64, uint32_t* events, uint32_t* event_days, uint32_t* duration_max, double* sum,
                                    uint32_t* vmax, uint32_t* invalid, uint8_t* mask, const int64_t* rec_off, int32_t* rec_start,
                                    int32_t* rec_end, uint32_t* rec_vmax, int32_t* rec_tmax, double* rec_sum,
                                    uint32_t* rec_invalid, uint64_t* status) {
    const char* name = "marex_cell_events_u8";
    if (!ctx) return -1;
    const int nacc = (events != nullptr) + (event_days != nullptr) + (duration_max != nullptr);
    const int nacc_a = (sum != nullptr) + (vmax != nullptr) + (invalid != nullptr);
    const int nrec = (rec_off != nullptr) + (rec_start != nullptr) + (rec_end != nullptr);
    const int nrec_a = (rec_vmax != nullptr) + (rec_tmax != nullptr) + (rec_sum != nullptr) + (rec_invalid != nullptr);
    if (!x || !state_i32 || !status || (anom && !state_f64) || t0 < 0 || Tb < 0 || C <= 0 || min_duration < 1 || max_gap < 0 ||
        G <= 0 || (!grp && G != 1) || (nacc != 0 && nacc != 3) || nacc_a != (anom && nacc ? 3 : 0) || (nrec != 0 && nrec != 3) ||
        nrec_a != (anom && nrec ? 4 : 0))
        return fail(ctx, -1, "%s: null field, state or status, anomalies without their state, empty shape, t0 < 0, "
                             "min_duration < 1, max_gap < 0, no group, or accumulators or records given in part", name);
    if (ce_misaligned(anom, 4) || ce_misaligned(grp, 4) || ce_misaligned(state_i32, 4) || ce_misaligned(state_f64, 8) ||
        ce_misaligned(events, 4) || ce_misaligned(event_days, 4) || ce_misaligned(duration_max, 4) || ce_misaligned(sum, 8) ||
        ce_misaligned(vmax, 4) || ce_misaligned(invalid, 4) || ce_misaligned(rec_off, 8) || ce_misaligned(rec_start, 4) ||
        ce_misaligned(rec_end, 4) || ce_misaligned(rec_vmax, 4) || ce_misaligned(rec_tmax, 4) || ce_misaligned(rec_sum, 8) ||
        ce_misaligned(rec_invalid, 4) || ce_misaligned(status, 8))
        return fail(ctx, -1, "%s: a pointer is not aligned to its element", name);
    if (const int rc = cell_stream_limits(ctx, name, t0, Tb, C)) return rc;
    if (Tb == 0) return 0;  // nothing to walk
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    LaunchTimer lt(ctx, MAREX_K_MORPH);
    // four cells per lane without anomalies only: with them the four-cell build needs 239 VGPRs
    const bool quad = !anom && C % 4 == 0 && !ce_misaligned(x, 4) && !ce_misaligned(mask, 4);
    const dim3 grid = quad ? cell_grid<4>(C) : cell_grid<1>(C), block(256);
#define CE_GO(V, ANOM)                                                                                                          \
    hipLaunchKernelGGL((k_cell_events<V, ANOM>), grid, block, 0, ctx->stream, (const unsigned char*)x, anom, (long)t0, (long)Tb, \
                       (long)C, min_duration, max_gap, finish, grp, G, state_i32, state_f64, (unsigned*)events,                 \
                       (unsigned*)event_days, (unsigned*)duration_max, sum, (unsigned*)vmax, (unsigned*)invalid,                \
                       (unsigned char*)mask, (const long long*)rec_off, rec_start, rec_end, (unsigned*)rec_vmax, rec_tmax,      \
                       rec_sum, (unsigned*)rec_invalid, (u64*)status)
    if (quad)
        CE_GO(4, false);
    else if (anom)
        CE_GO(1, true);
    else
        CE_GO(1, false);
#undef CE_GO
    HIP_TRY(ctx, hipGetLastError());
    return 0;
}
