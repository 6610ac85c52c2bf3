// the box matching of the SAM3D fusion step.
// Reference: src/nuscenes/linear_matching.py:53-121,231-259 (and the same block of
// src/waymo/linear_matching.py): per sample, `match(pred_boxes, sam3d_boxes, 0.2, Type.TYPE_2D)` =
// waymo_open_dataset's py_metrics_ops.match with TYPE_HUNGARIAN -- bird's-eye-view IoU of rotated
// rectangles, quantised to integers, maximum-weight bipartite assignment, pairs below the IoU
// threshold dropped.  (The op's C++ is not in the reference checkout: parity unpinned)
//
// Launches for all samples of a result file:
//   k_bev_weights    one thread per (prediction, sam3d) pair of a sample: float64 polygon clipping ->
//                    int32 weight matrix (the matrices sit in L2 for the solver)
//   k_bev_assign<C>  one wave per sample of at most 64 C boxes on its larger side (C = 1, 2, 4, 16): assign.h's
//                    AssignSolver with rows = the smaller side, then the matches written out
// Latency / integer bound; no HBM roofline applies (a sample's matrix is a few KB).
#include "assign.h"

#define BM_MAX_SIDE CM3D_MAX_MATCH_BOXES
#define BM_LDS 8192               // weights of a sample up to this many pairs sit in LDS, larger ones are read from L2

__global__ __launch_bounds__(256) void k_bev_init(int32_t *__restrict__ pred_match, double *__restrict__ match_iou, int n_pred,
                                                  int32_t *__restrict__ gt_match, int n_gt)
{
    const int t = blockIdx.x * 256 + threadIdx.x;
    if (t < n_pred) { pred_match[t] = -1; match_iou[t] = 0.0; }
    if (t < n_gt) gt_match[t] = -1;
}

__global__ __launch_bounds__(256) void k_bev_weights(const double *__restrict__ pred, const int32_t *__restrict__ pred_off,
                                                     const double *__restrict__ gt, const int32_t *__restrict__ gt_off,
                                                     const int64_t *__restrict__ pair_off, const int32_t *__restrict__ blk_frame,
                                                     int n_frames, int64_t total_pairs, double thr, int32_t *__restrict__ weight)
{
    const int64_t t = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (t >= total_pairs) return;
    const AssignPair q = assign_locate(t, blk_frame, pair_off, gt_off, n_frames);
    const double iou = bev_iou(pred + (int64_t)(pred_off[q.group] + q.p) * 6, gt + (int64_t)(gt_off[q.group] + q.g) * 6);
    weight[t] = assign_weight(iou, thr);
}

template <int CPL>
__global__ __launch_bounds__(64) void k_bev_assign(const double *__restrict__ pred, const int32_t *__restrict__ pred_off,
                                                   const double *__restrict__ gt, const int32_t *__restrict__ gt_off,
                                                   const int64_t *__restrict__ pair_off, const int32_t *__restrict__ weight,
                                                   int32_t *__restrict__ pred_match, int32_t *__restrict__ gt_match,
                                                   double *__restrict__ match_iou, int32_t *__restrict__ status)
{
    __shared__ int s_w[BM_LDS];
    const int f = blockIdx.x, lane = threadIdx.x;
    const int p0 = pred_off[f], g0 = gt_off[f];
    const int P = pred_off[f + 1] - p0, G = gt_off[f + 1] - g0;
    const int big = P > G ? P : G;
    if (P <= 0 || G <= 0) return;
    if (CPL == 1 && big > BM_MAX_SIDE) {         // capacity check, once per sample
        if (lane == 0) atomicOr(status, 1);
        return;
    }
    if (!assign_instance_takes<CPL>(big)) return;                 // another instance's sample
    const int32_t *__restrict__ Wm = weight + pair_off[f];
    const bool tr = P > G;                       // rows = the smaller side
    const int n = tr ? G : P, m = tr ? P : G;
    const bool in_lds = n * m <= BM_LDS;
    if (in_lds) {                                // LDS image: row-major [n][m] in (row, column) order of the search
        for (int q = lane; q < n * m; q += 64) {
            const int i = q / m, j = q - i * m;
            s_w[q] = tr ? Wm[(int64_t)j * G + i] : Wm[(int64_t)i * G + j];
        }
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
        __builtin_amdgcn_wave_barrier();
        __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
    }
    auto wgt = [&](int i, int j) -> int {        // weight of row i, column j (1-based)
        if (in_lds) return s_w[(i - 1) * m + (j - 1)];
        return tr ? Wm[(int64_t)(j - 1) * G + (i - 1)] : Wm[(int64_t)(i - 1) * G + (j - 1)];
    };
    AssignSolver<CPL> S;
    S.solve(n, m, wgt, [](int) {});
#pragma unroll
    for (int k = 0; k < CPL; ++k) {
        const int col = k * 64 + lane + 1;
        if (col <= m && S.p[k] != 0) {
            const int i = S.p[k];
            if (wgt(i, col) > 0) {               // below the IoU threshold: not a match
                const int pi = tr ? col - 1 : i - 1, gi = tr ? i - 1 : col - 1;
                pred_match[p0 + pi] = gi;
                gt_match[g0 + gi] = pi;
                match_iou[p0 + pi] = bev_iou(pred + (int64_t)(p0 + pi) * 6, gt + (int64_t)(g0 + gi) * 6);
            }
        }
    }
}

extern "C" int64_t cm3d_bev_match_workspace_bytes(int64_t total_pairs)
{
    return assign_workspace_bytes(total_pairs);
}

extern "C" int cm3d_bev_match(const double *pred, const int32_t *pred_off, int32_t n_pred, const double *gt,
                              const int32_t *gt_off, int32_t n_gt, const int64_t *pair_off, int32_t n_frames,
                              int64_t total_pairs, double iou_thr, int32_t *pred_match, int32_t *gt_match, double *match_iou,
                              int32_t *status, void *workspace, int64_t workspace_bytes, cm3d_stream_t stream)
{
    if (!pred_off || !gt_off || !pair_off || !status || n_frames <= 0 || n_pred < 0 || n_gt < 0 || total_pairs < 0)
        return CM3D_ERR_ARG;
    if ((n_pred > 0 && (!pred || !pred_match || !match_iou)) || (n_gt > 0 && (!gt || !gt_match))) return CM3D_ERR_ARG;
    if (total_pairs >= ((int64_t)1 << 31) * 256) return CM3D_ERR_ARG;
    if (total_pairs > 0 && (!workspace || workspace_bytes < cm3d_bev_match_workspace_bytes(total_pairs))) return CM3D_ERR_WORKSPACE;
    hipStream_t st = (hipStream_t)stream;
    const int n_init = n_pred > n_gt ? n_pred : n_gt;
    if (n_init > 0) {
        hipLaunchKernelGGL(k_bev_init, dim3((n_init + 255) / 256), dim3(256), 0, st, pred_match, match_iou, n_pred, gt_match, n_gt);
        CM3D_CHECK_LAUNCH();
    }
    if (total_pairs == 0) return CM3D_OK;
    int32_t *weight = (int32_t *)workspace;
    int32_t *blk_frame = weight + total_pairs;
    const int64_t n_blocks = (total_pairs + 255) / 256;
    hipLaunchKernelGGL(k_assign_block_owner, dim3((unsigned)((n_blocks + 255) / 256)), dim3(256), 0, st, pair_off, n_frames, n_blocks,
                       blk_frame);
    CM3D_CHECK_LAUNCH();
    hipLaunchKernelGGL(k_bev_weights, dim3((unsigned)n_blocks), dim3(256), 0, st, pred, pred_off, gt, gt_off, pair_off, blk_frame,
                       n_frames, total_pairs, iou_thr, weight);
    CM3D_CHECK_LAUNCH();
    hipLaunchKernelGGL(k_bev_assign<1>, dim3(n_frames), dim3(64), 0, st, pred, pred_off, gt, gt_off, pair_off, weight, pred_match,
                       gt_match, match_iou, status);
    CM3D_CHECK_LAUNCH();
    hipLaunchKernelGGL(k_bev_assign<2>, dim3(n_frames), dim3(64), 0, st, pred, pred_off, gt, gt_off, pair_off, weight, pred_match,
                       gt_match, match_iou, status);
    CM3D_CHECK_LAUNCH();
    hipLaunchKernelGGL(k_bev_assign<4>, dim3(n_frames), dim3(64), 0, st, pred, pred_off, gt, gt_off, pair_off, weight, pred_match,
                       gt_match, match_iou, status);
    CM3D_CHECK_LAUNCH();
    hipLaunchKernelGGL(k_bev_assign<16>, dim3(n_frames), dim3(64), 0, st, pred, pred_off, gt, gt_off, pair_off, weight, pred_match,
                       gt_match, match_iou, status);
    CM3D_CHECK_LAUNCH();
    return CM3D_OK;
}
