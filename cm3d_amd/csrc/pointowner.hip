// One owner per contested point, exclusive in-mask lists (opt-in): cm3d_point_owner of include/cm3d_hip.h, which states the rule;
// cm3d_amd/pointowner.py is the host statement, to the bit.
//   k_owner_rank     one thread per mask: its frame by a search of mask_off, then its rank in the frame -- the number of the frame's
//                    masks it beats under the rule (a loop over the frame's masks, at most CM3D_MAX_MASKS_PER_FRAME in a real batch) --
//                    and the inverse, by_rank[first mask of the frame + rank] = mask.  The order is strict and total, so the ranks of
//                    a frame are a permutation.
//   k_owner_claim<0> one workgroup per mask: 0 into the table entry of every listed point (only entries that are read later are
//                    cleared: the table is 4 F P bytes, the lists a small part of it).
//   k_owner_claim<1> one workgroup per mask: an integer maximum of rank + 1 on the entry of every listed point.  A maximum does not
//                    depend on the order of arrival, so every run leaves the same table.
//   k_owner_resolve  one workgroup per mask: entry -> by_rank -> the owner of every position (ow_owner), one keep byte per position,
//                    the kept count behind a workgroup sum, the MIN_KEEP rule, ow_status and ow_lost.
//   k_list_compact_scan / _scatter (csrc/list_compact.h, shared with cm3d_depth_cluster and cm3d_ground_strip).
// Every offset read from device memory is clamped first: list positions into [0, idx_cap], mask numbers into [0, n_masks]; a point
// index outside [0, P) touches no table entry.  Integer atomics only, no allocation, no read-back.
#include "common.h"
#include "list_compact.h"

#define PO_THREADS 256

static __device__ __forceinline__ int po_clamp(int v, int lo, int hi) { return v < lo ? lo : (v > hi ? hi : v); }

// a beats b (a != b): the rule of the header.  A NaN score is lower than every number and equal to another NaN.
static __device__ __forceinline__ bool po_beats(int rule, double sa, int na, int a, double sb, int nb, int b)
{
    const bool gt = sa == sa && (sb != sb || sa > sb);
    const bool eq = (sa != sa && sb != sb) || sa == sb;
    if (rule == 0) return gt || (eq && (na < nb || (na == nb && a < b)));
    return na < nb || (na == nb && (gt || (eq && a < b)));
}

__global__ __launch_bounds__(PO_THREADS) void k_owner_rank(const int32_t *__restrict__ hit_off, const int32_t *__restrict__ mask_off,
                                                           int n_frames, int n_masks, int idx_cap, const double *__restrict__ score,
                                                           int rule, int32_t *__restrict__ rank, int32_t *__restrict__ frame,
                                                           int32_t *__restrict__ by_rank)
{
    const int m = blockIdx.x * PO_THREADS + threadIdx.x;
    if (m >= n_masks) return;
    int f = -1, m0 = 0, m1 = 0;
    if (n_frames > 0) {                                     // the last frame whose first mask is not behind m (mask_off ascends)
        int a = 0, b = n_frames;
        while (b - a > 1) {
            const int mid = (a + b) >> 1;
            if (po_clamp(mask_off[mid], 0, n_masks) <= m) a = mid; else b = mid;
        }
        m0 = po_clamp(mask_off[a], 0, n_masks), m1 = po_clamp(mask_off[a + 1], m0, n_masks);
        if (m0 <= m && m < m1) f = a;
    }
    int r = 0;
    if (f >= 0) {
        const double sa = score[m];
        const int na = lc_range(hit_off, m, idx_cap).n;
        for (int j = m0; j < m1; ++j)
            if (j != m && po_beats(rule, sa, na, m, score[j], lc_range(hit_off, j, idx_cap).n, j)) ++r;
        by_rank[m0 + r] = m;                                // (r < m1 - m0)
    }
    rank[m] = r;
    frame[m] = f;
}

// CLAIM 0: clear the listed entries; 1: the maximum of rank + 1
template <int CLAIM>
__global__ __launch_bounds__(LC_THREADS) void k_owner_claim(const int32_t *__restrict__ hit_idx, const int32_t *__restrict__ hit_off,
                                                            int idx_cap, int P, const int32_t *__restrict__ rank,
                                                            const int32_t *__restrict__ frame, int32_t *__restrict__ table)
{
    const int m = blockIdx.x;
    const int f = frame[m];
    if (f < 0) return;
    const LcRange r = lc_range(hit_off, m, idx_cap);
    int32_t *const tab = table + (size_t)f * (size_t)P;
    const int v = rank[m] + 1;
    for (long long i = threadIdx.x; i < r.n; i += LC_THREADS) {
        const int p = hit_idx[r.lo + i];
        if (p < 0 || p >= P) continue;
        if (CLAIM) atomicMax(&tab[p], v); else tab[p] = 0;
    }
}

__global__ __launch_bounds__(LC_THREADS) void k_owner_resolve(const int32_t *__restrict__ hit_idx, const int32_t *__restrict__ hit_off,
                                                              const int32_t *__restrict__ mask_off, int n_masks, int idx_cap, int P,
                                                              const int32_t *__restrict__ frame, const int32_t *__restrict__ by_rank,
                                                              const int32_t *__restrict__ table, int min_keep,
                                                              int32_t *__restrict__ ow_owner, uint8_t *__restrict__ keep,
                                                              int32_t *__restrict__ count, int32_t *__restrict__ ow_status,
                                                              int32_t *__restrict__ ow_lost)
{
    __shared__ int s_cnt[LC_WAVES];
    const int m = blockIdx.x, lane = cm3d_lane(), wave = threadIdx.x >> 6;
    const LcRange r = lc_range(hit_off, m, idx_cap);
    if (r.n == 0) {
        if (threadIdx.x == 0) count[m] = 0, ow_status[m] = 2, ow_lost[m] = 0;
        return;
    }
    const int f = frame[m];
    const int m0 = f >= 0 ? po_clamp(mask_off[f], 0, n_masks) : 0;
    const int32_t *const tab = table + (size_t)(f >= 0 ? f : 0) * (size_t)P;
    int kept = 0;
    for (long long i = threadIdx.x; i < r.n; i += LC_THREADS) {
        const int p = hit_idx[r.lo + i];
        int owner = m;
        if (f >= 0 && p >= 0 && p < P) owner = by_rank[po_clamp(m0 + tab[p] - 1, 0, n_masks - 1)];      // (the entry is in [1, masks of f])
        ow_owner[r.lo + i] = owner;
        keep[r.lo + i] = owner == m ? 1 : 0;
        kept += owner == m ? 1 : 0;
    }
    kept = cm3d_wave_sum(kept);
    if (lane == 0) s_cnt[wave] = kept;
    __syncthreads();
    kept = 0;
#pragma unroll
    for (int w = 0; w < LC_WAVES; ++w) kept += s_cnt[w];
    const bool whole = kept < min_keep;
    if (whole)                  // the list is kept whole (every thread sets the bytes it wrote itself)
        for (long long i = threadIdx.x; i < r.n; i += LC_THREADS) keep[r.lo + i] = 1;
    if (threadIdx.x == 0) {
        count[m] = whole ? r.n : kept;
        ow_status[m] = whole ? 1 : 0;
        ow_lost[m] = whole ? 0 : r.n - kept;
    }
}

extern "C" int cm3d_point_owner_check(int32_t rule, int32_t min_keep)
{
    return (rule == 0 || rule == 1) && min_keep >= 1 ? CM3D_OK : CM3D_ERR_ARG;
}

extern "C" int64_t cm3d_point_owner_workspace_bytes(int32_t n_frames, int32_t max_pts_per_frame, int32_t n_masks, int32_t idx_cap)
{
    if (n_frames < 0 || max_pts_per_frame < 0 || n_masks <= 0 || idx_cap <= 0) return 0;
    return 16 * (int64_t)n_masks + 4 * (int64_t)n_frames * (int64_t)max_pts_per_frame + (int64_t)idx_cap;
}

extern "C" int cm3d_point_owner(const float *hit_xyz, const int32_t *hit_idx, const int32_t *hit_off, const int32_t *mask_off,
                                int32_t n_frames, int32_t n_masks, int32_t idx_cap, int32_t max_pts_per_frame, const double *score,
                                int32_t rule, int32_t min_keep, int32_t *ow_owner, int32_t *ow_off, int32_t *ow_tile_off, int32_t *ow_idx,
                                float *ow_xyz, int32_t *ow_status, int32_t *ow_lost, void *workspace, int64_t workspace_bytes,
                                cm3d_stream_t stream)
{
    if (cm3d_point_owner_check(rule, min_keep) != CM3D_OK) return CM3D_ERR_ARG;
    if (n_masks < 0 || idx_cap <= 0 || n_frames < 0 || max_pts_per_frame < 0) return CM3D_ERR_ARG;
    if (!hit_idx) return CM3D_ERR_ARG;                      // the stage cannot do without the point indices
    if (n_masks == 0) return CM3D_OK;
    if (!hit_xyz || !hit_off || !mask_off || !score || !ow_owner || !ow_off || !ow_tile_off || !ow_idx || !ow_xyz || !ow_status || !ow_lost ||
        !workspace)
        return CM3D_ERR_ARG;
    if (((uintptr_t)hit_xyz & 15) || ((uintptr_t)ow_xyz & 15) || ((uintptr_t)workspace & 3)) return CM3D_ERR_ARG;
    if (workspace_bytes < cm3d_point_owner_workspace_bytes(n_frames, max_pts_per_frame, n_masks, idx_cap)) return CM3D_ERR_WORKSPACE;
    hipStream_t st = (hipStream_t)stream;
    // count i32[M] | rank i32[M] | frame i32[M] | by_rank i32[M] | table i32[F][P] | keep u8[idx_cap]
    int32_t *count = (int32_t *)workspace, *rank = count + n_masks, *frame = rank + n_masks, *by_rank = frame + n_masks;
    int32_t *table = by_rank + n_masks;
    uint8_t *keep = (uint8_t *)(table + (size_t)n_frames * (size_t)max_pts_per_frame);
    const int P = max_pts_per_frame;
    hipLaunchKernelGGL(k_owner_rank, dim3((n_masks + PO_THREADS - 1) / PO_THREADS), dim3(PO_THREADS), 0, st, hit_off, mask_off, n_frames,
                       n_masks, idx_cap, score, rule, rank, frame, by_rank);
    CM3D_CHECK_LAUNCH();
    hipLaunchKernelGGL(k_owner_claim<0>, dim3(n_masks), dim3(LC_THREADS), 0, st, hit_idx, hit_off, idx_cap, P, rank, frame, table);
    CM3D_CHECK_LAUNCH();
    hipLaunchKernelGGL(k_owner_claim<1>, dim3(n_masks), dim3(LC_THREADS), 0, st, hit_idx, hit_off, idx_cap, P, rank, frame, table);
    CM3D_CHECK_LAUNCH();
    hipLaunchKernelGGL(k_owner_resolve, dim3(n_masks), dim3(LC_THREADS), 0, st, hit_idx, hit_off, mask_off, n_masks, idx_cap, P, frame,
                       by_rank, table, min_keep, ow_owner, keep, count, ow_status, ow_lost);
    CM3D_CHECK_LAUNCH();
    hipLaunchKernelGGL(k_list_compact_scan, dim3(1), dim3(1024), 0, st, count, n_masks, ow_off, ow_tile_off);
    CM3D_CHECK_LAUNCH();
    hipLaunchKernelGGL(k_list_compact_scatter, dim3(n_masks), dim3(LC_THREADS), 0, st, (const float4 *)hit_xyz, hit_idx, hit_off, idx_cap,
                       keep, ow_off, ow_idx, (float4 *)ow_xyz);
    CM3D_CHECK_LAUNCH();
    return CM3D_OK;
}
