// marex_mesh_merge.hip -- the partition kernels of the tracker's split-and-merge stage on an unstructured mesh
// (split_and_merge_objects_parallel, marEx/track.py:3804-4814; partition_nn_unstructured_optimised, 5246-5353;
// partition_centroid_unstructured, 5357-5419).  The host (marex_amd/track_mesh.py) drives the chunk / timestep / child
// loop and reads only small tables; a slice of the ID field [C] is partitioned here, in place.
//
// Nearest centroid.  The reference compares float32 haversine distances under numba fastmath, which is not
// reproducible.  The contract here: the host builds float64 unit vectors of the cells, u [3][C], and of the parents'
// float32 centroids, pv [3][n]; a cell goes to the parent with the smallest chord ((dx dx + dy dy) + dz dz), float64,
// no FMA (-ffp-contract=off), parents scanned in order with a strict comparison (first minimum).  The chord is monotone
// in the great-circle distance; no transcendental function is evaluated on the device.
//
// Nearest neighbour.  The reference grows the parents' frontiers over the mesh edges: a hop is, for parent p ascending
// and direction i = 0, 1, 2, one substep in which every unclaimed cell that is the i-th listed neighbour of a cell owned
// by p at the start of that substep becomes p's.  One 32-bit word per cell holds (stamp << 8) | owner (owner 255 =
// unclaimed, stamp = the number of the substep that claimed it, 0 for seeds): "owned at the start of the substep" is
// owner == p && stamp < this substep's stamp, and a claim is one compare-and-swap of the unclaimed word, so both are
// decided from one word and exactly one claimer counts a cell.  One launch per substep: the launch boundary is the
// barrier between substeps; there is no grid-wide wait.  A control block carries the stopping rule, so that the host
// may queue several hops before it looks: substeps launched after "stopped" do nothing.
#include "marex_common.hip.h"

#define MMRG_UNCLAIMED 0xFFu
#define MMRG_MAX_PARENTS 10
// control block, int32 [8]
#define MMRG_CTL_UNCLAIMED 0  // child cells without an owner
#define MMRG_CTL_CLAIMED 1    // a child cell was claimed in the running hop
#define MMRG_CTL_STOPPED 2
#define MMRG_CTL_HOPS 3       // hops run
#define MMRG_CTL_LEFT 4       // child cells the finish kernel gave to the nearest centroid
#define MMRG_CTL_REASON 5     // 1: no child cell unclaimed, 2: a hop claimed no child cell, 3: the hop cap
#define MMRG_CTL_WORDS 8

// the entry j in [j0, j1) whose vector pv[.][j] is nearest to the unit vector of cell c (first minimum)
__device__ __forceinline__ int mmrg_nearest(const double* __restrict__ u, long C, long c, const double* __restrict__ pv, int n_ent,
                                            int j0, int j1) {
    const double x = u[c], y = u[C + c], z = u[2 * C + c];
    int best = j0;
    double bd = __builtin_huge_val();
    for (int j = j0; j < j1; ++j) {
        const double dx = x - pv[j], dy = y - pv[n_ent + j], dz = z - pv[2 * n_ent + j];
        const double d = (dx * dx + dy * dy) + dz * dz;
        if (d < bd) {
            bd = d;
            best = j;
        }
    }
    return best;
}

// Centroid partition of every merging child of one timestep in one launch: child k (child_keys[k], ascending) has the
// parent entries off[k] .. off[k + 1]; each of its cells takes lab[] of the nearest entry.  The children's cells are
// disjoint and the new labels are fresh IDs (or the child's own), so no cell is visited twice.
__global__ void __launch_bounds__(256)
k_mmrg_part_centroid(int* __restrict__ ids, long C, const int* __restrict__ child_keys, int n_child, const int* __restrict__ off,
                     const double* __restrict__ u, const double* __restrict__ pv, int n_ent, const int* __restrict__ lab) {
    for (long c = (long)blockIdx.x * 256 + threadIdx.x; c < C; c += (long)gridDim.x * 256) {
        const int v = ids[c];
        if (v <= 0) continue;
        const int k = sorted_find(child_keys, n_child, v);
        if (k < 0) continue;
        const int j0 = off[k], j1 = off[k + 1];
        if (j0 < 0 || j1 > n_ent || j0 >= j1) continue;
        ids[c] = lab[mmrg_nearest(u, C, c, pv, n_ent, j0, j1)];
    }
}

// word[c] = j for a cell of parent parents[j] in prev, else unclaimed; ctl[UNCLAIMED] = the child cells without an owner
__global__ void __launch_bounds__(256)
k_mmrg_nn_seed(const int* __restrict__ cur, const int* __restrict__ prev, long C, int child, const int* __restrict__ parents,
               int n_par, unsigned* __restrict__ word, int* __restrict__ ctl) {
    for (long base = (long)blockIdx.x * 256; base < C; base += (long)gridDim.x * 256) {  // uniform over the workgroup
        const long c = base + threadIdx.x;
        bool open = false;
        if (c < C) {
            const int pid = prev[c];
            unsigned o = MMRG_UNCLAIMED;
            if (pid > 0)
                for (int j = 0; j < n_par; ++j)
                    if (parents[j] == pid) {
                        o = (unsigned)j;
                        break;
                    }
            word[c] = o;
            open = o == MMRG_UNCLAIMED && cur[c] == child;
        }
        const int n = __popcll(__ballot(open));
        if ((threadIdx.x & 63) == 0 && n) atomicAdd(&ctl[MMRG_CTL_UNCLAIMED], n);
    }
}

// Before every hop, one thread: the reference's loop conditions (track.py:5292, 5322-5325) in their order.
__global__ void k_mmrg_nn_gate(int* __restrict__ ctl, int max_hops) {
    if (threadIdx.x || blockIdx.x || ctl[MMRG_CTL_STOPPED]) return;
    int reason = 0;
    if (ctl[MMRG_CTL_HOPS] > 0 && !ctl[MMRG_CTL_CLAIMED]) reason = 2;
    else if (ctl[MMRG_CTL_UNCLAIMED] <= 0) reason = 1;
    else if (ctl[MMRG_CTL_HOPS] >= max_hops) reason = 3;
    if (reason) {
        ctl[MMRG_CTL_REASON] = reason;
        ctl[MMRG_CTL_STOPPED] = 1;
    } else {
        ctl[MMRG_CTL_CLAIMED] = 0;
        ctl[MMRG_CTL_HOPS] += 1;
    }
}

// One substep: parent p, direction nbr_i = nbr[i], stamp > 0 unique and increasing over the substeps of this child.
__global__ void __launch_bounds__(256)
k_mmrg_nn_substep(const int* __restrict__ cur, const int* __restrict__ nbr_i, long C, int child, unsigned p, unsigned stamp,
                  unsigned* word, int* ctl) {
    if (ctl[MMRG_CTL_STOPPED]) return;  // written by the gate kernel only: the same for every thread of this launch
    const unsigned mine = (stamp << 8) | p;
    for (long c = (long)blockIdx.x * 256 + threadIdx.x; c < C; c += (long)gridDim.x * 256) {
        const unsigned w = word[c];
        if ((w & 0xFFu) != p || (w >> 8) >= stamp) continue;  // not p's, or claimed in this very substep
        const int n = nbr_i[c];
        if (n < 0 || (long)n >= C) continue;
        if (atomicCAS(&word[n], MMRG_UNCLAIMED, mine) != MMRG_UNCLAIMED) continue;
        if (cur[n] == child) {
            atomicSub(&ctl[MMRG_CTL_UNCLAIMED], 1);
            atomicOr(&ctl[MMRG_CTL_CLAIMED], 1);
        }
    }
}

// cur[c] = lab[owner] for every child cell; a cell that is still unclaimed takes the nearest centroid
__global__ void __launch_bounds__(256)
k_mmrg_nn_finish(int* __restrict__ cur, long C, int child, const double* __restrict__ u, const double* __restrict__ pv, int n_par,
                 const int* __restrict__ lab, const unsigned* __restrict__ word, int* __restrict__ ctl) {
    for (long base = (long)blockIdx.x * 256; base < C; base += (long)gridDim.x * 256) {  // uniform over the workgroup
        const long c = base + threadIdx.x;
        bool left = false;
        if (c < C && cur[c] == child) {
            unsigned o = word[c] & 0xFFu;
            if (o == MMRG_UNCLAIMED) {
                left = true;
                o = (unsigned)mmrg_nearest(u, C, c, pv, n_par, 0, n_par);
            }
            if (o < (unsigned)n_par) cur[c] = lab[o];
        }
        const int n = __popcll(__ballot(left));
        if ((threadIdx.x & 63) == 0 && n) atomicAdd(&ctl[MMRG_CTL_LEFT], n);
    }
}

extern "C" int marex_mesh_partition_centroid_i32(marex_ctx* ctx, int32_t* ids, int64_t C, const int32_t* child_keys, int n_child,
                                                 const int32_t* off, const double* u, const double* pv, int n_ent,
                                                 const int32_t* lab) {
    if (!ctx) return -1;
    if (!ids || !child_keys || !off || !u || !pv || !lab || C <= 0 || n_child <= 0 || n_ent <= 0)
        return fail(ctx, -1, "marex_mesh_partition_centroid_i32: null pointer, empty slice, no child or no parent");
    if (C >= 2147483647L) return fail(ctx, -4, "marex_mesh_partition_centroid_i32: a slice has 2^31 - 1 or more cells");
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    LaunchTimer lt(ctx, MAREX_K_MORPH);
    hipLaunchKernelGGL(k_mmrg_part_centroid, dim3(stride_grid(C)), dim3(256), 0, ctx->stream, ids, (long)C, child_keys, n_child, off, u,
                       pv, n_ent, lab);
    HIP_TRY(ctx, hipGetLastError());
    return 0;
}

extern "C" int marex_mesh_nn_seed_i32(marex_ctx* ctx, const int32_t* cur, const int32_t* prev, int64_t C, int child,
                                      const int32_t* parents, int n_par, uint32_t* word, int32_t* ctl) {
    if (!ctx) return -1;
    if (!cur || !prev || !parents || !word || !ctl || C <= 0 || child <= 0)
        return fail(ctx, -1, "marex_mesh_nn_seed_i32: null pointer, empty slice or no child");
    if (n_par < 1 || n_par > MMRG_MAX_PARENTS) return fail(ctx, -1, "marex_mesh_nn_seed_i32: n_par=%d is not in 1 .. %d", n_par, MMRG_MAX_PARENTS);
    if (C >= 2147483647L) return fail(ctx, -4, "marex_mesh_nn_seed_i32: a slice has 2^31 - 1 or more cells");
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    LaunchTimer lt(ctx, MAREX_K_MORPH);
    HIP_TRY(ctx, hipMemsetAsync(ctl, 0, MMRG_CTL_WORDS * sizeof(int), ctx->stream));
    hipLaunchKernelGGL(k_mmrg_nn_seed, dim3(stride_grid(C)), dim3(256), 0, ctx->stream, cur, prev, (long)C, child, parents, n_par,
                       (unsigned*)word, ctl);
    HIP_TRY(ctx, hipGetLastError());
    return 0;
}

extern "C" int marex_mesh_nn_hops_i32(marex_ctx* ctx, const int32_t* cur, const int32_t* nbr, int64_t C, int child, int n_par,
                                      int first_hop, int n_hops, int max_hops, uint32_t* word, int32_t* ctl) {
    if (!ctx) return -1;
    if (!cur || !nbr || !word || !ctl || C <= 0 || child <= 0)
        return fail(ctx, -1, "marex_mesh_nn_hops_i32: null pointer, empty slice or no child");
    if (n_par < 1 || n_par > MMRG_MAX_PARENTS) return fail(ctx, -1, "marex_mesh_nn_hops_i32: n_par=%d is not in 1 .. %d", n_par, MMRG_MAX_PARENTS);
    if (C >= 2147483647L) return fail(ctx, -4, "marex_mesh_nn_hops_i32: a slice has 2^31 - 1 or more cells");
    const long per_hop = 3L * n_par;
    if (first_hop < 0 || n_hops < 0 || max_hops < 0 || (long)first_hop + n_hops > max_hops || (long)max_hops * per_hop >= (1L << 24))
        return fail(ctx, -1, "marex_mesh_nn_hops_i32: hops %d .. +%d of at most %d with %d parents do not fit the 24-bit substep stamp",
                    first_hop, n_hops, max_hops, n_par);
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    LaunchTimer lt(ctx, MAREX_K_MORPH);
    const dim3 grid(stride_grid(C));
    for (int h = first_hop; h < first_hop + n_hops; ++h) {
        hipLaunchKernelGGL(k_mmrg_nn_gate, dim3(1), dim3(64), 0, ctx->stream, ctl, max_hops);
        for (int p = 0; p < n_par; ++p)
            for (int i = 0; i < 3; ++i)
                hipLaunchKernelGGL(k_mmrg_nn_substep, grid, dim3(256), 0, ctx->stream, cur, nbr + (size_t)i * C, (long)C, child,
                                   (unsigned)p, (unsigned)((long)h * per_hop + 3 * p + i + 1), (unsigned*)word, ctl);
    }
    HIP_TRY(ctx, hipGetLastError());
    return 0;
}

extern "C" int marex_mesh_nn_finish_i32(marex_ctx* ctx, int32_t* cur, int64_t C, int child, const double* u, const double* pv,
                                        int n_par, const int32_t* lab, const uint32_t* word, int32_t* ctl, int max_hops) {
    if (!ctx) return -1;
    if (!cur || !u || !pv || !lab || !word || !ctl || C <= 0 || child <= 0)
        return fail(ctx, -1, "marex_mesh_nn_finish_i32: null pointer, empty slice or no child");
    if (n_par < 1 || n_par > MMRG_MAX_PARENTS) return fail(ctx, -1, "marex_mesh_nn_finish_i32: n_par=%d is not in 1 .. %d", n_par, MMRG_MAX_PARENTS);
    if (C >= 2147483647L) return fail(ctx, -4, "marex_mesh_nn_finish_i32: a slice has 2^31 - 1 or more cells");
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    LaunchTimer lt(ctx, MAREX_K_MORPH);
    hipLaunchKernelGGL(k_mmrg_nn_gate, dim3(1), dim3(64), 0, ctx->stream, ctl, max_hops);  // names the reason of the stop
    hipLaunchKernelGGL(k_mmrg_nn_finish, dim3(stride_grid(C)), dim3(256), 0, ctx->stream, cur, (long)C, child, u, pv, n_par, lab,
                       (const unsigned*)word, ctl);
    HIP_TRY(ctx, hipGetLastError());
    return 0;
}
