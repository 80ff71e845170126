#pragma once
// marex_cellwalk.hip.h -- what the per-cell streaming kernels (marex_occurrence.hip, marex_local_intensity.hip,
// marex_cell_events.hip, marex_compound.hip, marex_heat_stress.hip) share: a lane owns one cell, or four consecutive uint8
// cells through one 32-bit load, for the whole call and walks the rows.  The kernels, their unroll depths and what they keep per cell stay in their
// units (the register budgets differ).  The leaf helpers that the event kernels use too -- u64,
// finite_bits, severity_class, wave_sum, cell_stream_limits -- are in marex_common.hip.h.
#include "marex_common.hip.h"

// the word a lane loads per row: T int or unsigned char, V cells per lane
template <typename T, int V>
struct cell_word;
template <>
struct cell_word<int, 1> { typedef int type; };
template <>
struct cell_word<unsigned char, 1> { typedef unsigned char type; };
template <>
struct cell_word<unsigned char, 4> { typedef unsigned type; };

// the value of sub-cell j in the loaded word
template <int V, typename W>
__device__ __forceinline__ int cell_value(W w, int j) {
    return V == 4 ? (int)(((unsigned)w >> (8 * j)) & 255u) : (int)w;
}

__device__ __forceinline__ bool cell_present(int v, int match) { return match ? v == match : v > 0; }

// The wave's distinct classes among the lanes' cj (one sub-cell): the k-th goes to lane k, as the 64-bit mask of its lanes
// and its value; a class outside 0 .. R - 1 belongs to nobody.  Every lane of the wave must call it (ballots), lanes past
// the last cell with cj = -1.
__device__ __forceinline__ void wave_class_partition(int cj, int R, int lane, u64& smask, int& scls) {
    u64 todo = __ballot(cj >= 0 && cj < R);
    for (int n = 0; todo; ++n) {  // at most 64 rounds: each takes at least one lane
        const int cv = __shfl(cj, __ffsll((long long)todo) - 1, 64);
        const u64 same = __ballot(cj == cv) & todo;
        if (lane == n) {
            smask = same;
            scls = cv;
        }
        todo &= ~same;
    }
}

// blocks of 256 lanes with V cells each over a row of C cells
template <int V>
static inline dim3 cell_grid(long C) {
    const long lanes = (C + V - 1) / V;
    return dim3((unsigned)((lanes + 255) / 256));
}
