// Waymo 3D detection metrics (the counting part of waymo-open-dataset's compute_detection_metrics_main; host side and
// the rules: cm3d_amd/waymo_eval.py).
//
// Input: "groups" = (frame, type, shard) with their predictions (descending score) and ground truth.  Per group and per
// score cutoff c (101 of them, float32(c * 0.01)) the predictions with score >= cutoff are matched one to one with the
// group's ground truth: maximum-weight assignment on weight = int(3D IoU x 1e6), pairs below the type's IoU threshold
// never match.  Counted per (breakdown, cutoff): TP, FP, FN at LEVEL_1, FN at LEVEL_2 and the heading-accuracy sum of
// the matches (int64, 2^-32 units), all with integer atomics: the result does not depend on the order in which waves run.
//
// Launches:
//   k_wm_weights   one thread per (prediction, ground truth) pair of a group: float64 polygon clipping x z overlap
//   k_wm_match<C>  one wave per group of at most 64 C columns (C = 1, 2, 4, 16): assign.h's AssignSolver.  Rows are
//                  predictions in score order, columns the ground truth padded with empty columns to max(P, G).
//                  The method adds one row per phase and the assignment after phase k is optimal for the first k rows,
//                  so ONE solve gives the matching of every cutoff: the counts are taken after the phases that end a
//                  cutoff's prediction subset (at most P + 1 distinct subsets).  per_cutoff != 0 solves every cutoff
//                  afresh instead (a check of that deduplication).
#include "assign.h"

#define WM_BREAKDOWNS 16
#define WM_CUTOFFS 101
#define WM_LDS 4096                 // weights of a group up to this many pairs sit in LDS, larger ones are read from L2

static __device__ __forceinline__ float wm_cutoff(int c) { return (float)(c * 0.01); }

static __device__ __forceinline__ double wm_thr(int bd) { return bd < 4 ? 0.7 : 0.5; }     // vehicle 0.7, the other types 0.5

// Box record (CM3D_WM_BOX_STRIDE doubles): cx, cy, length, width, cos(heading), sin(heading), cz, height.
static __device__ double wm_iou3d(const double *__restrict__ a, const double *__restrict__ b)
{
    const double va = a[2] * a[3] * a[7], vb = b[2] * b[3] * b[7];
    if (!(a[2] * a[3] > 0.0) || !(b[2] * b[3] > 0.0) || !(a[7] > 0.0) || !(b[7] > 0.0)) return 0.0;
    double inter = bev_inter_area(a, b);
    const double zlo = fmax(a[6] - 0.5 * a[7], b[6] - 0.5 * b[7]);
    const double zhi = fmin(a[6] + 0.5 * a[7], b[6] + 0.5 * b[7]);
    inter = inter * fmax(zhi - zlo, 0.0);
    const double uni = (va + vb) - inter;
    if (!(uni > 0.0)) return 0.0;
    const double iou = inter / uni;
    return iou > 1.0 ? 1.0 : iou;
}

// heading accuracy of a match in 2^-32 units: 1 - |d| / pi, d = float32 heading difference wrapped to [-pi, pi]
static __device__ long long wm_heading_fx(float pd, float gt)
{
    const double pi = 3.141592653589793, two_pi = 6.283185307179586;
    const float d32 = gt - pd;
    double t = fmod((double)d32 + pi, two_pi);
    if (t < 0.0) t += two_pi;
    double d = (double)(float)fabs(t - pi);
    if (d > pi) d = (double)(float)(two_pi - d);
    double acc = 1.0 - d / pi;
    acc = acc < 0.0 ? 0.0 : (acc > 1.0 ? 1.0 : acc);
    return llrint((double)(float)acc * 4294967296.0);
}

__global__ __launch_bounds__(256) void k_wm_zero(long long *__restrict__ counts, long long *__restrict__ heading)
{
    const int t = blockIdx.x * 256 + threadIdx.x;
    if (t < WM_BREAKDOWNS * WM_CUTOFFS * 4) counts[t] = 0;
    if (t < WM_BREAKDOWNS * WM_CUTOFFS) heading[t] = 0;
}

__global__ __launch_bounds__(256) void k_wm_weights(const double *__restrict__ pred, const int32_t *__restrict__ pred_off,
                                                    const double *__restrict__ gt, const int32_t *__restrict__ gt_off,
                                                    const int32_t *__restrict__ group_bd, const int64_t *__restrict__ pair_off,
                                                    const int32_t *__restrict__ blk_group, int n_groups, int64_t total_pairs,
                                                    int32_t *__restrict__ weight)
{
    const int64_t t = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (t >= total_pairs) return;
    const AssignPair q = assign_locate(t, blk_group, pair_off, gt_off, n_groups);
    const double iou = wm_iou3d(pred + (int64_t)(pred_off[q.group] + q.p) * CM3D_WM_BOX_STRIDE,
                                gt + (int64_t)(gt_off[q.group] + q.g) * CM3D_WM_BOX_STRIDE);
    weight[t] = assign_weight(iou, wm_thr(group_bd[q.group]));
}

// The counting of one group, shared by k_wm_match and k_wm_sweep_match: P rows in descending score order (score_at(r), r = 0..P-1,
// heading head_at(i) and weights wgt(i, j) of row i = 1..P), G ground-truth columns from g0, level1() of them at LEVEL_1.  Finds every
// cutoff's prefix of rows, solves once (per_cutoff: every cutoff afresh), takes the counts at the prefix boundaries and adds them
// to breakdown bd of counts / heading with integer atomics.
template <int CPL, typename Wgt, typename ScoreAt, typename HeadAt, typename Level1>
static __device__ __forceinline__ void wm_count_group(int P, int G, int g0, int bd, Wgt wgt, ScoreAt score_at, HeadAt head_at, Level1 level1,
                                                      const float *__restrict__ gt_head, const int32_t *__restrict__ gt_level,
                                                      int per_cutoff, unsigned long long *__restrict__ counts,
                                                      unsigned long long *__restrict__ heading)
{
    const int lane = threadIdx.x;
    const int big = P > G ? P : G;
    // prediction subset size of this lane's cutoffs (lane, lane + 64): predictions with score >= cutoff
    int kc[2];
#pragma unroll
    for (int s = 0; s < 2; ++s) {
        const int c = lane + 64 * s;
        const float cut = wm_cutoff(c < WM_CUTOFFS ? c : 0);
        int lo = 0, hi = P;
        while (lo < hi) {
            const int mid = (lo + hi) >> 1;
            if (score_at(mid) >= cut) lo = mid + 1; else hi = mid;
        }
        kc[s] = c < WM_CUTOFFS ? lo : -1;
    }
    const int n_l1 = level1();
    long long r_tp[2] = {0, 0}, r_fn1[2] = {n_l1, n_l1}, r_fn2[2] = {G, G}, r_h[2] = {0, 0};      // the empty subset's counts

    AssignSolver<CPL> S;
    // counts of the current assignment, taken by the lanes whose cutoff subset has `rows` predictions
    // TP, FN at LEVEL_1 and the heading sum of the current assignment (pairs of zero weight are no match)
    auto count = [&](long long &tp, long long &fn1, long long &h) {
#pragma unroll
        for (int k = 0; k < CPL; ++k) {
            const int col = k * 64 + lane + 1;
            if (col <= G) {
                const int i = S.p[k];
                const bool matched = i != 0 && wgt(i, col) > 0;
                tp += matched;
                if (!matched && gt_level[g0 + col - 1] == 1) ++fn1;
                if (matched) h += wm_heading_fx(head_at(i), gt_head[g0 + col - 1]);
            }
        }
        tp = assign_wave_sum(tp);
        fn1 = assign_wave_sum(fn1);
        h = assign_wave_sum(h);
    };
    auto record = [&](int rows) {
        long long tp = 0, fn1 = 0, h = 0;
        count(tp, fn1, h);
#pragma unroll
        for (int s = 0; s < 2; ++s)
            if (kc[s] == rows) { r_tp[s] = tp; r_fn1[s] = fn1; r_fn2[s] = G - tp; r_h[s] = h; }
    };
    auto record_boundary = [&](int i) {          // after row i: record(i) when some lane's cutoff ends there
        const bool here = kc[0] == i || kc[1] == i;
        if (__builtin_amdgcn_ballot_w64(here) != 0ull) record(i);
    };
    if (!per_cutoff) {
        if (P > 0 && G > 0) S.solve(P, big, wgt, record_boundary);
    } else {
        // every cutoff on its own: a fresh solve over its subset, columns padded to max(k, G)
        for (int c = 0; c < WM_CUTOFFS; ++c) {
            const int k = __shfl(c < 64 ? kc[0] : kc[1], c & 63, 64);
            if (k > 0 && G > 0) {
                S.solve(k, k > G ? k : G, wgt, [](int) {});
                long long tp = 0, fn1 = 0, h = 0;
                count(tp, fn1, h);
                if (lane == (c & 63) && c < 64) { r_tp[0] = tp; r_fn1[0] = fn1; r_fn2[0] = G - tp; r_h[0] = h; }
                if (lane == (c & 63) && c >= 64) { r_tp[1] = tp; r_fn1[1] = fn1; r_fn2[1] = G - tp; r_h[1] = h; }
            }
        }
    }
    // this group's contribution to its breakdown: one lane per cutoff, zero terms skipped
#pragma unroll
    for (int s = 0; s < 2; ++s) {
        const int c = lane + 64 * s;
        if (c >= WM_CUTOFFS) continue;
        unsigned long long *dst = counts + ((int64_t)bd * WM_CUTOFFS + c) * 4;
        const long long fp = (long long)kc[s] - r_tp[s];
        if (r_tp[s]) atomicAdd(dst + 0, (unsigned long long)r_tp[s]);
        if (fp) atomicAdd(dst + 1, (unsigned long long)fp);
        if (r_fn1[s]) atomicAdd(dst + 2, (unsigned long long)r_fn1[s]);
        if (r_fn2[s]) atomicAdd(dst + 3, (unsigned long long)r_fn2[s]);
        if (r_h[s]) atomicAdd(heading + (int64_t)bd * WM_CUTOFFS + c, (unsigned long long)r_h[s]);
    }
}

static __device__ __forceinline__ void wm_wave_sync()        // LDS written by some lanes of the wave is read by others
{
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}

template <int CPL>
__global__ __launch_bounds__(64) void k_wm_match(const float *__restrict__ pred_head, const float *__restrict__ pred_score,
                                                 const int32_t *__restrict__ pred_off, const float *__restrict__ gt_head,
                                                 const int32_t *__restrict__ gt_level, const int32_t *__restrict__ gt_off,
                                                 const int32_t *__restrict__ group_bd, const int64_t *__restrict__ pair_off,
                                                 const int32_t *__restrict__ weight, int per_cutoff,
                                                 unsigned long long *__restrict__ counts, unsigned long long *__restrict__ heading,
                                                 int32_t *__restrict__ status)
{
    __shared__ int s_w[WM_LDS];
    const int g = blockIdx.x, lane = threadIdx.x;
    const int p0 = pred_off[g], g0 = gt_off[g];
    const int P = pred_off[g + 1] - p0, G = gt_off[g + 1] - g0;
    const int bd = group_bd[g];
    const int big = P > G ? P : G;
    if (CPL == 1) {                              // capacity and type checks, once per group
        if (bd < 0 || bd >= WM_BREAKDOWNS) { if (lane == 0) atomicOr(status, 2); return; }
        if (big > CM3D_MAX_MATCH_BOXES) { if (lane == 0) atomicOr(status, 1); return; }
    }
    if (bd < 0 || bd >= WM_BREAKDOWNS || !assign_instance_takes<CPL>(big)) return;       // another instance's group
    const int32_t *__restrict__ Wm = weight + pair_off[g];
    const bool in_lds = P * G <= WM_LDS;
    if (in_lds) {
        for (int q = lane; q < P * G; q += 64) s_w[q] = Wm[q];
        wm_wave_sync();
    }
    auto wgt = [&](int i, int j) -> int {        // row i (prediction), column j (ground truth or empty), 1-based
        if (j > G) return 0;
        return in_lds ? s_w[(i - 1) * G + (j - 1)] : Wm[(int64_t)(i - 1) * G + (j - 1)];
    };
    auto level1 = [&]() {
        int n_l1 = 0;
        for (int j = lane; j < G; j += 64) n_l1 += gt_level[g0 + j] == 1;
        return cm3d_wave_sum(n_l1);
    };
    wm_count_group<CPL>(P, G, g0, bd, wgt, [&](int r) { return pred_score[p0 + r]; }, [&](int i) { return pred_head[p0 + i - 1]; },
                        level1, gt_head, gt_level, per_cutoff, counts, heading);
}

// ---- the alpha sweep of the SAM3D fusion grid search (host side: cm3d_amd/fusion.py, waymo_eval.pack_candidates) ----
// A group's rows are a candidate superset in candidate order; per alpha a candidate is active or not and has a score:
//   kind 0 unmatched prediction: score p           kind 1 unmatched SAM3D box: score clip(s * alpha)
//   kind 2 prediction of a pair: score p, active iff !(s * alpha > p)     kind 3 its SAM3D box: clip(s * alpha), iff s * alpha > p
// (p, s and s * alpha in double, one rounding to float).  The weights of all candidates x ground truth are computed once.
#define WM_SWEEP_TARGET_WAVES 4096       // the alphas of a call are cut into slices until about this many waves run

static __device__ __forceinline__ unsigned wm_score_key(float score)       // ascending key = descending score; -0 == +0
{
    const unsigned b = __float_as_uint(score + 0.0f);
    return ~(b ^ ((b >> 31) ? 0xffffffffu : 0x80000000u));
}

// One wave per (group, slice of alphas); the wave walks its alphas.  Per alpha: keys of the active candidates into LDS, rank
// sort (rank = number of smaller keys; key = descending score, then candidate order -- pack_arrays' lexsort), the ranked
// scores and the permutation into LDS, then wm_count_group with rows read through the permutation, into the alpha's slice.
// A static group (kind 0 only) is counted once, by slice 0, into the static slice that k_wm_sweep_add_static adds to every alpha.
template <int CPL>
__global__ __launch_bounds__(64) void k_wm_sweep_match(const float *__restrict__ cand_head, const int32_t *__restrict__ cand_kind,
                                                       const double *__restrict__ cand_p, const double *__restrict__ cand_s,
                                                       const int32_t *__restrict__ cand_off, const float *__restrict__ gt_head,
                                                       const int32_t *__restrict__ gt_level, const int32_t *__restrict__ gt_off,
                                                       const int32_t *__restrict__ group_bd, const int64_t *__restrict__ pair_off,
                                                       const int32_t *__restrict__ weight, const int32_t *__restrict__ group_static,
                                                       const double *__restrict__ alphas, int n_alphas, int per_slice,
                                                       unsigned long long *__restrict__ counts, unsigned long long *__restrict__ heading,
                                                       unsigned long long *__restrict__ static_counts,
                                                       unsigned long long *__restrict__ static_heading, int32_t *__restrict__ status)
{
    __shared__ int s_w[WM_LDS];
    __shared__ unsigned long long s_key[64 * CPL];
    __shared__ float s_score[64 * CPL];
    __shared__ int s_perm[64 * CPL];
    const int g = blockIdx.x, slice = blockIdx.y, lane = threadIdx.x;
    const int c0 = cand_off[g], g0 = gt_off[g];
    const int C = cand_off[g + 1] - c0, G = gt_off[g + 1] - g0;
    const int bd = group_bd[g];
    const int big = C > G ? C : G;
    if (CPL == 1 && slice == 0) {                // capacity and type checks, once per group
        if (bd < 0 || bd >= WM_BREAKDOWNS) { if (lane == 0) atomicOr(status, 2); return; }
        if (big > CM3D_MAX_MATCH_BOXES) { if (lane == 0) atomicOr(status, 1); return; }
    }
    if (bd < 0 || bd >= WM_BREAKDOWNS || big > CM3D_MAX_MATCH_BOXES || !assign_instance_takes<CPL>(big)) return;
    const bool is_static = group_static[g] != 0;
    if (is_static && slice != 0) return;
    const int a_lo = is_static ? 0 : slice * per_slice;
    const int a_hi = is_static ? 1 : (a_lo + per_slice < n_alphas ? a_lo + per_slice : n_alphas);
    if (a_lo >= a_hi) return;
    const int32_t *__restrict__ Wm = weight + pair_off[g];
    const bool in_lds = C * G <= WM_LDS;
    if (in_lds)
        for (int q = lane; q < C * G; q += 64) s_w[q] = Wm[q];
    auto wgt = [&](int i, int j) -> int {        // row i in rank order (candidate s_perm[i - 1]), column j, 1-based
        if (j > G) return 0;
        const int c = s_perm[i - 1];
        return in_lds ? s_w[c * G + (j - 1)] : Wm[(int64_t)c * G + (j - 1)];
    };
    int n_l1 = 0;
    for (int j = lane; j < G; j += 64) n_l1 += gt_level[g0 + j] == 1;
    n_l1 = cm3d_wave_sum(n_l1);
    for (int a = a_lo; a < a_hi; ++a) {
        const double alpha = is_static ? 0.0 : alphas[a];
        unsigned long long key[CPL];
        float score[CPL];
        int n_active = 0;
#pragma unroll
        for (int k = 0; k < CPL; ++k) {
            const int c = k * 64 + lane;
            key[k] = ~0ull;
            score[k] = 0.0f;
            if (c < C) {
                const int kind = cand_kind[c0 + c];
                const double p = cand_p[c0 + c], prod = cand_s[c0 + c] * alpha;
                const bool sam = prod > p;
                const bool active = kind == 0 || kind == 1 || (kind == 2 && !sam) || (kind == 3 && sam);
                const double clipped = prod < 0.0 ? 0.0 : (prod > 1.0 ? 1.0 : prod);
                score[k] = (float)((kind == 0 || kind == 2) ? p : clipped);
                if (active) key[k] = ((unsigned long long)wm_score_key(score[k]) << 32) | (unsigned)c;
                n_active += active;
                s_key[c] = key[k];
            }
        }
        n_active = cm3d_wave_sum(n_active);
        wm_wave_sync();
        int rank[CPL];
#pragma unroll
        for (int k = 0; k < CPL; ++k) rank[k] = 0;
        for (int j = 0; j < C; ++j) {
            const unsigned long long kj = s_key[j];
#pragma unroll
            for (int k = 0; k < CPL; ++k) rank[k] += kj < key[k];
        }
#pragma unroll
        for (int k = 0; k < CPL; ++k)
            if (key[k] != ~0ull) {               // an active candidate: its rank is below n_active <= C
                s_perm[rank[k]] = k * 64 + lane;
                s_score[rank[k]] = score[k];
            }
        wm_wave_sync();
        wm_count_group<CPL>(n_active, G, g0, bd, wgt, [&](int r) { return s_score[r]; },
                            [&](int i) { return cand_head[c0 + s_perm[i - 1]]; }, [&]() { return n_l1; }, gt_head, gt_level, 0,
                            is_static ? static_counts : counts + (int64_t)a * (WM_BREAKDOWNS * WM_CUTOFFS * 4),
                            is_static ? static_heading : heading + (int64_t)a * (WM_BREAKDOWNS * WM_CUTOFFS));
        wm_wave_sync();                          // the next alpha overwrites the permutation
    }
}

__global__ __launch_bounds__(256) void k_wm_sweep_zero(long long *__restrict__ a, int64_t na, long long *__restrict__ b, int64_t nb)
{
    const int64_t t = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (t < na) a[t] = 0;
    if (t < nb) b[t] = 0;
}

// every alpha's slice += the static groups' counts (slice layout: counts [16][101][4], then heading [16][101])
__global__ __launch_bounds__(256) void k_wm_sweep_add_static(long long *__restrict__ counts, long long *__restrict__ heading,
                                                             const long long *__restrict__ static_slice, int n_alphas)
{
    const int NC = WM_BREAKDOWNS * WM_CUTOFFS * 4, NH = WM_BREAKDOWNS * WM_CUTOFFS;
    const int64_t t = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (t >= (int64_t)n_alphas * (NC + NH)) return;
    const int a = (int)(t / (NC + NH)), r = (int)(t - (int64_t)a * (NC + NH));
    if (r < NC) counts[(int64_t)a * NC + r] += static_slice[r];
    else heading[(int64_t)a * NH + (r - NC)] += static_slice[r];
}

extern "C" int64_t cm3d_waymo_metrics_workspace_bytes(int64_t total_pairs)
{
    return assign_workspace_bytes(total_pairs);
}

extern "C" int cm3d_waymo_metrics(const double *pred_box, const float *pred_heading, const float *pred_score,
                                  const int32_t *pred_off, const double *gt_box, const float *gt_heading, const int32_t *gt_level,
                                  const int32_t *gt_off, const int32_t *group_bd, const int64_t *pair_off, int32_t n_groups,
                                  int64_t total_pairs, int32_t per_cutoff, int64_t *counts, int64_t *heading_sum, int32_t *status,
                                  void *workspace, int64_t workspace_bytes, cm3d_stream_t stream)
{
    if (!pred_off || !gt_off || !group_bd || !pair_off || !counts || !heading_sum || !status || n_groups < 0 || total_pairs < 0)
        return CM3D_ERR_ARG;
    if (total_pairs >= ((int64_t)1 << 31) * 256) return CM3D_ERR_ARG;
    if (total_pairs > 0 && (!pred_box || !gt_box || !workspace || workspace_bytes < cm3d_waymo_metrics_workspace_bytes(total_pairs)))
        return total_pairs > 0 && (!pred_box || !gt_box) ? CM3D_ERR_ARG : CM3D_ERR_WORKSPACE;
    hipStream_t st = (hipStream_t)stream;
    hipLaunchKernelGGL(k_wm_zero, dim3((WM_BREAKDOWNS * WM_CUTOFFS * 4 + 255) / 256), dim3(256), 0, st, (long long *)counts,
                       (long long *)heading_sum);
    CM3D_CHECK_LAUNCH();
    if (n_groups == 0) return CM3D_OK;
    int32_t *weight = (int32_t *)workspace;
    if (total_pairs > 0) {
        int32_t *blk_group = weight + total_pairs;
        const int64_t n_blocks = (total_pairs + 255) / 256;
        hipLaunchKernelGGL(k_assign_block_owner, dim3((unsigned)((n_blocks + 255) / 256)), dim3(256), 0, st, pair_off, n_groups, n_blocks,
                           blk_group);
        CM3D_CHECK_LAUNCH();
        hipLaunchKernelGGL(k_wm_weights, dim3((unsigned)n_blocks), dim3(256), 0, st, pred_box, pred_off, gt_box, gt_off, group_bd,
                           pair_off, blk_group, n_groups, total_pairs, weight);
        CM3D_CHECK_LAUNCH();
    }
    unsigned long long *c = (unsigned long long *)counts, *h = (unsigned long long *)heading_sum;
    hipLaunchKernelGGL(k_wm_match<1>, dim3(n_groups), dim3(64), 0, st, pred_heading, pred_score, pred_off, gt_heading, gt_level, gt_off,
                       group_bd, pair_off, weight, per_cutoff, c, h, status);
    CM3D_CHECK_LAUNCH();
    hipLaunchKernelGGL(k_wm_match<2>, dim3(n_groups), dim3(64), 0, st, pred_heading, pred_score, pred_off, gt_heading, gt_level, gt_off,
                       group_bd, pair_off, weight, per_cutoff, c, h, status);
    CM3D_CHECK_LAUNCH();
    hipLaunchKernelGGL(k_wm_match<4>, dim3(n_groups), dim3(64), 0, st, pred_heading, pred_score, pred_off, gt_heading, gt_level, gt_off,
                       group_bd, pair_off, weight, per_cutoff, c, h, status);
    CM3D_CHECK_LAUNCH();
    hipLaunchKernelGGL(k_wm_match<16>, dim3(n_groups), dim3(64), 0, st, pred_heading, pred_score, pred_off, gt_heading, gt_level, gt_off,
                       group_bd, pair_off, weight, per_cutoff, c, h, status);
    CM3D_CHECK_LAUNCH();
    return CM3D_OK;
}

#define WM_SWEEP_STATIC_WORDS (WM_BREAKDOWNS * WM_CUTOFFS * 5)      // the static slice: counts, then heading sums

extern "C" int64_t cm3d_waymo_metrics_sweep_workspace_bytes(int64_t total_pairs)
{
    return (int64_t)WM_SWEEP_STATIC_WORDS * (int64_t)sizeof(int64_t) + assign_workspace_bytes(total_pairs);
}

extern "C" int cm3d_waymo_metrics_sweep(const double *cand_box, const float *cand_heading, const int32_t *cand_kind, const double *cand_p,
                                        const double *cand_s, const int32_t *cand_off, const double *gt_box, const float *gt_heading,
                                        const int32_t *gt_level, const int32_t *gt_off, const int32_t *group_bd, const int64_t *pair_off,
                                        const int32_t *group_static, int32_t n_groups, int64_t total_pairs, const double *alphas,
                                        int32_t n_alphas, int64_t *counts, int64_t *heading_sum, int32_t *status, void *workspace,
                                        int64_t workspace_bytes, cm3d_stream_t stream)
{
    if (!cand_off || !gt_off || !group_bd || !pair_off || !group_static || !alphas || !counts || !heading_sum || !status || n_groups < 0 ||
        total_pairs < 0 || n_alphas < 1 || n_alphas > CM3D_WM_SWEEP_MAX_ALPHAS)
        return CM3D_ERR_ARG;
    if (total_pairs >= ((int64_t)1 << 31) * 256) return CM3D_ERR_ARG;
    if (total_pairs > 0 && (!cand_box || !gt_box)) return CM3D_ERR_ARG;
    if (!workspace || workspace_bytes < cm3d_waymo_metrics_sweep_workspace_bytes(total_pairs)) return CM3D_ERR_WORKSPACE;
    hipStream_t st = (hipStream_t)stream;
    long long *stat = (long long *)workspace;
    const int64_t n_out = (int64_t)n_alphas * WM_BREAKDOWNS * WM_CUTOFFS * 4;
    hipLaunchKernelGGL(k_wm_sweep_zero, dim3((unsigned)((n_out + 255) / 256)), dim3(256), 0, st, (long long *)counts, n_out,
                       (long long *)heading_sum, n_out / 4);
    CM3D_CHECK_LAUNCH();
    hipLaunchKernelGGL(k_wm_sweep_zero, dim3((WM_SWEEP_STATIC_WORDS + 255) / 256), dim3(256), 0, st, stat, (int64_t)WM_SWEEP_STATIC_WORDS,
                       stat, (int64_t)0);
    CM3D_CHECK_LAUNCH();
    if (n_groups == 0) return CM3D_OK;
    int32_t *weight = (int32_t *)(stat + WM_SWEEP_STATIC_WORDS);
    if (total_pairs > 0) {
        int32_t *blk_group = weight + total_pairs;
        const int64_t n_blocks = (total_pairs + 255) / 256;
        hipLaunchKernelGGL(k_assign_block_owner, dim3((unsigned)((n_blocks + 255) / 256)), dim3(256), 0, st, pair_off, n_groups, n_blocks,
                           blk_group);
        CM3D_CHECK_LAUNCH();
        hipLaunchKernelGGL(k_wm_weights, dim3((unsigned)n_blocks), dim3(256), 0, st, cand_box, cand_off, gt_box, gt_off, group_bd,
                           pair_off, blk_group, n_groups, total_pairs, weight);
        CM3D_CHECK_LAUNCH();
    }
    // few groups: more slices of fewer alphas, so that the device fills; many groups: one wave walks all alphas of its group
    int slices = WM_SWEEP_TARGET_WAVES / n_groups;
    slices = slices < 1 ? 1 : (slices > n_alphas ? n_alphas : slices);
    const int per_slice = (n_alphas + slices - 1) / slices;
    slices = (n_alphas + per_slice - 1) / per_slice;
    unsigned long long *c = (unsigned long long *)counts, *h = (unsigned long long *)heading_sum, *sc = (unsigned long long *)stat;
    unsigned long long *sh = sc + WM_BREAKDOWNS * WM_CUTOFFS * 4;
    const dim3 grid(n_groups, slices);
#define WM_SWEEP_LAUNCH(CPL)                                                                                                          \
    hipLaunchKernelGGL(k_wm_sweep_match<CPL>, grid, dim3(64), 0, st, cand_heading, cand_kind, cand_p, cand_s, cand_off, gt_heading,   \
                       gt_level, gt_off, group_bd, pair_off, weight, group_static, alphas, n_alphas, per_slice, c, h, sc, sh, status); \
    CM3D_CHECK_LAUNCH();
    WM_SWEEP_LAUNCH(1)
    WM_SWEEP_LAUNCH(2)
    WM_SWEEP_LAUNCH(4)
    WM_SWEEP_LAUNCH(16)
#undef WM_SWEEP_LAUNCH
    const int64_t n_add = (int64_t)n_alphas * WM_SWEEP_STATIC_WORDS;
    hipLaunchKernelGGL(k_wm_sweep_add_static, dim3((unsigned)((n_add + 255) / 256)), dim3(256), 0, st, (long long *)counts,
                       (long long *)heading_sum, stat, n_alphas);
    CM3D_CHECK_LAUNCH();
    return CM3D_OK;
}
