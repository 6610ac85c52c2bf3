// Maximum-weight one-to-one assignment of quantised IoUs, shared by the SAM3D fusion matching (fusion.hip) and the Waymo
// detection metrics (waymo_metrics.hip): the pair -> weight plumbing of their weight kernels and the one wave-level solver.
#pragma once
#include "bev_iou.h"

#define ASSIGN_KMAX 1000000        // IoU quantisation: weight = (int)(iou * ASSIGN_KMAX); a pair's cost is ASSIGN_KMAX - weight

static __device__ __forceinline__ int assign_weight(double iou, double thr)
{
    return iou >= thr ? (int)(iou * (double)ASSIGN_KMAX) : 0;
}

// workspace of a call over total_pairs pairs: the int32 weights + the first group of every 256-pair block
static inline int64_t assign_workspace_bytes(int64_t total_pairs)
{
    const int64_t n = total_pairs > 0 ? total_pairs : 1;
    return (n + (n + 255) / 256) * (int64_t)sizeof(int32_t);
}

// first group (sample, or frame x type) of every 256-pair block of a weight kernel: one binary search per block instead of
// one per pair
static __global__ __launch_bounds__(256) void k_assign_block_owner(const int64_t *__restrict__ pair_off, int n_groups, int64_t n_blocks,
                                                                   int32_t *__restrict__ blk_owner)
{
    const int64_t b = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (b >= n_blocks) return;
    const int64_t t = b * 256;
    int lo = 0, hi = n_groups;              // last g with pair_off[g] <= t
    while (hi - lo > 1) {
        const int mid = (lo + hi) >> 1;
        if (pair_off[mid] <= t) lo = mid; else hi = mid;
    }
    blk_owner[b] = lo;
}

// pair t of a weight kernel (block = 256 pairs): its group, prediction p and ground truth g within the group
struct AssignPair { int group, p, g; };
static __device__ __forceinline__ AssignPair assign_locate(int64_t t, const int32_t *__restrict__ blk_owner,
                                                           const int64_t *__restrict__ pair_off, const int32_t *__restrict__ gt_off,
                                                           int n_groups)
{
    int f = blk_owner[blockIdx.x];
    while (f + 1 < n_groups && pair_off[f + 1] <= t) ++f;      // a block spans few groups
    const int G = gt_off[f + 1] - gt_off[f];
    const int64_t r = t - pair_off[f];
    const int p = (int)(r / G);
    return {f, p, (int)(r - (int64_t)p * G)};
}

static __device__ __forceinline__ long long assign_wave_min(long long v)
{
    return cm3d_wave_reduce_t(v, [](long long a, long long b) { return b < a ? b : a; });
}

static __device__ __forceinline__ long long assign_wave_sum(long long v)
{
    return cm3d_wave_reduce_t(v, [](long long a, long long b) { return a + b; });
}

// element idx (wave-uniform) of a state array: slot idx / 64 of lane idx % 64
template <int CPL>
static __device__ __forceinline__ int assign_get(const int (&a)[CPL], int idx)
{
    int r = __builtin_amdgcn_readlane(a[0], idx & 63);
#pragma unroll
    for (int k = 1; k < CPL; ++k) {
        const int t = __builtin_amdgcn_readlane(a[k], idx & 63);
        r = (idx >> 6) == k ? t : r;
    }
    return r;
}

// The solver is instantiated for 64, 128, 256 and 1024 columns; instance CPL takes the groups whose larger side is above
// the next smaller instance's capacity.
template <int CPL>
static __device__ __forceinline__ bool assign_instance_takes(int big)
{
    static_assert(CPL == 1 || CPL == 2 || CPL == 4 || CPL == 16, "launched instances");
    static_assert(64 * 16 == CM3D_MAX_MATCH_BOXES, "the widest instance holds the documented capacity");
    return big > (CPL == 1 ? 0 : CPL == 2 ? 64 : CPL == 4 ? 128 : 256) && big <= 64 * CPL;
}

// Hungarian method with potentials (u on rows, v on columns) by one wave of 64 lanes, all state in registers: column j
// (1-based) lives in lane (j - 1) % 64, slot (j - 1) / 64 -- potential v, reduced cost, predecessor `way`, assigned row p --
// and row r's potential u likewise.  No barrier inside the search.  rows n <= columns m <= 64 * CPL; every row gets a column.
// Cost = ASSIGN_KMAX - weight >= 0, so the assignment has maximum weight.  One row is added per phase and the assignment
// after phase i is optimal for rows 1..i.  Ties: an unassigned column wins a step (the search ends there: most costs are the
// same "no overlap" value), then the lowest column.  The CPU oracle runs the same steps sequentially.
// 32-bit state: a free column has v = 0, so 0 <= u <= ASSIGN_KMAX and -ASSIGN_KMAX <= v <= 0 by dual feasibility; reduced
// costs stay below 2 * ASSIGN_KMAX < 2^21 (far inside the coarser n * 10^6 <= 1024 * 10^6 < 2^30).
template <int CPL>
struct AssignSolver {
    int u[CPL], v[CPL], p[CPL], way[CPL];        // slot k: row / column k * 64 + lane + 1

    // wgt(i, j): weight of row i, column j (1-based); after_row(i): called (wave-uniformly) once row i has its column
    template <typename Wgt, typename AfterRow>
    __device__ __forceinline__ void solve(int n, int m, Wgt wgt, AfterRow after_row)
    {
        const int lane = threadIdx.x;
        const int INF = 1 << 30;
#pragma unroll
        for (int k = 0; k < CPL; ++k) { u[k] = 0; v[k] = 0; p[k] = 0; way[k] = 0; }
        for (int i = 1; i <= n; ++i) {
            int minv[CPL];
            bool used[CPL], row_in_tree[CPL];
#pragma unroll
            for (int k = 0; k < CPL; ++k) { minv[k] = INF; used[k] = false; row_in_tree[k] = false; }
            int j0 = 0;
            while (true) {
                // column j0 joins the tree, with it the row assigned to it
                const int i0 = j0 == 0 ? i : assign_get<CPL>(p, j0 - 1);
                const int ui0 = assign_get<CPL>(u, i0 - 1);
                long long key = (long long)INF << 12;
#pragma unroll
                for (int k = 0; k < CPL; ++k) {
                    const int col = k * 64 + lane + 1;
                    if (col == j0) used[k] = true;
                    if (col == i0) row_in_tree[k] = true;
                    if (col <= m && !used[k]) {
                        const int cur = (ASSIGN_KMAX - wgt(i0, col)) - ui0 - v[k];
                        if (cur < minv[k]) { minv[k] = cur; way[k] = j0; }
                        const long long kk = (long long)minv[k] * 4096 + (p[k] != 0 ? 2048 : 0) + col;   // the tie rule
                        key = kk < key ? kk : key;
                    }
                }
                key = assign_wave_min(key);
                const int delta = (int)(key >> 12);
                const int j1 = __builtin_amdgcn_readfirstlane((int)(key & 2047));
#pragma unroll
                for (int k = 0; k < CPL; ++k) {
                    if (row_in_tree[k]) u[k] += delta;
                    if (used[k]) v[k] -= delta; else minv[k] -= delta;
                }
                j0 = j1;
                if (assign_get<CPL>(p, j0 - 1) == 0) break;
            }
            do {                                 // augment along the predecessor chain (uniform pointer chasing through lane reads)
                const int j1 = assign_get<CPL>(way, j0 - 1);
                const int pr = j1 == 0 ? i : assign_get<CPL>(p, (j1 == 0 ? 1 : j1) - 1);
#pragma unroll
                for (int k = 0; k < CPL; ++k)
                    if (k * 64 + lane + 1 == j0) p[k] = pr;
                j0 = j1;
            } while (j0);
            after_row(i);
        }
    }
};
