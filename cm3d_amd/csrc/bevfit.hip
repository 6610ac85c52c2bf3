// Yaw fit of every mask's in-mask list (cm3d_bev_fit, cm3d_yaw_select; include/cm3d_hip.h states the semantics, cm3d_amd/bevfit.py is
// the host statement): search-based L-shape fitting with the closeness criterion on the bird's-eye view of the list.
//   k_bev_fit     one workgroup of K threads per mask: LANES ARE ANGLES, a wave owns 64 of them.  The list is staged through LDS in
//                 chunks of CM3D_BEV_FIT_CHUNK points, already widened and shifted to the list's first point; every lane reads the
//                 same LDS address (a broadcast, no bank conflict) and walks the list twice -- bounds, then the sum of 1/d in list
//                 order, which is the rule's order because it is the lane's own loop.  The K/64 waves of a mask share the staged
//                 chunk and nothing else; the choice of k* is one wave reduction and a look at K/64 candidates.  float64 throughout,
//                 no atomics, no allocation.
//   k_yaw_select  one thread per mask: fitted axis or lane yaw (the lane resolves the axis modulo pi), into a table k_box_nms reads
//                 in place of the lane tables.
// Every offset read from hit_off is clamped into [0, idx_cap] first (bf_range): nothing at or beyond idx_cap is read whatever the
// offsets hold.  Table, frame and lane indices of k_yaw_select are clamped into their arrays alike.
#include "common.h"

#define BF_CHUNK CM3D_BEV_FIT_CHUNK
#define BF_MAX_WAVES 4

struct BfRange { int lo, n; };
static __device__ __forceinline__ BfRange bf_range(const int32_t *hit_off, int m, int idx_cap)
{
    int lo = hit_off[m], hi = hit_off[m + 1];
    lo = lo < 0 ? 0 : (lo > idx_cap ? idx_cap : lo);
    hi = hi < lo ? lo : (hi > idx_cap ? idx_cap : hi);
    return BfRange{lo, hi - lo};
}

static __device__ __forceinline__ bool bf_finite(float v) { return fabsf(v) <= 3.402823466e38f; }      // (false for NaN)

// the list's points [base, base + cnt) as float64 offsets from its first point, into LDS; a barrier on either side
static __device__ __forceinline__ void bf_stage(const float4 *__restrict__ p, int cnt, double x0, double y0, double2 *s_p)
{
    __syncthreads();                             // the chunk before this one has been walked by every wave
    for (int i = threadIdx.x; i < cnt; i += blockDim.x) {
        const float4 v = p[i];
        s_p[i] = make_double2((double)v.x - x0, (double)v.y - y0);
    }
    __syncthreads();
}

__global__ __launch_bounds__(64 * BF_MAX_WAVES) void k_bev_fit(const float4 *__restrict__ hit_xyz, const int32_t *__restrict__ hit_off,
                                                               int idx_cap, const double2 *__restrict__ angle_cs, double d0, int min_points,
                                                               double min_length, int32_t *__restrict__ fit_k,
                                                               double *__restrict__ fit_rect, int32_t *__restrict__ fit_status)
{
    __shared__ double2 s_p[BF_CHUNK];
    __shared__ double s_q[BF_MAX_WAVES];
    __shared__ int s_k[BF_MAX_WAVES];
    const int m = blockIdx.x, t = threadIdx.x, K = blockDim.x;
    const BfRange r = bf_range(hit_off, m, idx_cap);
    const float4 *const list = hit_xyz + r.lo;
    const int n = r.n;
    double *const rect = fit_rect + (size_t)m * CM3D_MATCH_BOX_STRIDE;

    // (n is the same in every thread of the workgroup: the early ends are taken by all of them, in front of the first barrier)
    int status = n == 0 ? 2 : n < min_points ? 1 : 0;
    if (status == 0) {
        int bad = 0;
        for (int i = t; i < n; i += K) {
            const float4 v = list[i];
            bad |= !(bf_finite(v.x) && bf_finite(v.y));
        }
        if (__syncthreads_or(bad)) status = 4;
    }
    if (status != 0) {
        if (t == 0) {
            fit_k[m] = -1, fit_status[m] = status;
            for (int q = 0; q < CM3D_MATCH_BOX_STRIDE; ++q) rect[q] = 0.0;
        }
        return;
    }

    const double x0 = (double)list[0].x, y0 = (double)list[0].y;
    const double2 cs = angle_cs[t];
    const double c = cs.x, s = cs.y;

    // walk 1: the bounds of the list along (c, s) and across it.  (Minima and maxima are single instructions here, and they give the
    // bits of the statement's comparisons: every value is finite, and none is -0.0 -- x and y are differences in round-to-nearest, so
    // +0.0 where they vanish, c > 0 and s >= 0, so a product is -0.0 only beside a +0.0 one, and a difference of equals is +0.0.)
    double lo1 = INFINITY, hi1 = -INFINITY, lo2 = INFINITY, hi2 = -INFINITY;
    for (int base = 0; base < n; base += BF_CHUNK) {
        const int cnt = min(BF_CHUNK, n - base);
        bf_stage(list + base, cnt, x0, y0, s_p);
        for (int i = 0; i < cnt; ++i) {
            const double2 p = s_p[i];
            const double c1 = (p.x * c) + (p.y * s), c2 = (p.y * c) - (p.x * s);
            lo1 = fmin(lo1, c1), hi1 = fmax(hi1, c1);
            lo2 = fmin(lo2, c2), hi2 = fmax(hi2, c2);
        }
    }
    // walk 2: the closeness criterion, summed in list order
    double q = 0.0;
    for (int base = 0; base < n; base += BF_CHUNK) {
        const int cnt = min(BF_CHUNK, n - base);
        if (n > BF_CHUNK) bf_stage(list + base, cnt, x0, y0, s_p);       // (a list of one chunk is still staged)
        for (int i = 0; i < cnt; ++i) {
            const double2 p = s_p[i];
            const double c1 = (p.x * c) + (p.y * s), c2 = (p.y * c) - (p.x * s);
            const double d = fmax(fmin(fmin(hi1 - c1, c1 - lo1), fmin(hi2 - c2, c2 - lo2)), d0);
            q = q + 1.0 / d;
        }
    }

    // k*: the greatest q, the smallest k on a tie -- inside each wave, then over the K/64 waves
    const Cm3dDistIdx w = cm3d_wave_reduce_t(Cm3dDistIdx{q, t, 0},
                                             [](Cm3dDistIdx a, Cm3dDistIdx b) { return (b.s > a.s || (b.s == a.s && b.j < a.j)) ? b : a; });
    if (cm3d_lane() == 0) s_q[t >> 6] = w.s, s_k[t >> 6] = w.j;
    __syncthreads();
    double bq = s_q[0];
    int bk = s_k[0];
    for (int v = 1; v < (K >> 6); ++v)            // (ascending k: a later wave wins only with a strictly greater q)
        if (s_q[v] > bq) bq = s_q[v], bk = s_k[v];
    if (t != bk) return;

    const double a = hi1 - lo1, b = hi2 - lo2;
    const bool along = a >= b;
    const double length = along ? a : b, width = along ? b : a;
    if (length < min_length) {
        fit_k[m] = -1, fit_status[m] = 3;
        for (int v = 0; v < CM3D_MATCH_BOX_STRIDE; ++v) rect[v] = 0.0;
        return;
    }
    const double m1 = (lo1 + hi1) * 0.5, m2 = (lo2 + hi2) * 0.5;
    rect[0] = ((m1 * c) - (m2 * s)) + x0;
    rect[1] = ((m1 * s) + (m2 * c)) + y0;
    rect[2] = length, rect[3] = width;
    rect[4] = along ? c : -s, rect[5] = along ? s : c;
    fit_k[m] = t, fit_status[m] = 0;
}

static __device__ __forceinline__ int bf_clamp(int v, int n) { return v < 0 ? 0 : (v >= n ? n - 1 : v); }

__global__ __launch_bounds__(256) void k_yaw_select(const double *__restrict__ fit_rect, const int32_t *__restrict__ fit_status,
                                                    const int32_t *__restrict__ medoid_pos, const int32_t *__restrict__ mask_frame,
                                                    const int32_t *__restrict__ class_id, const int32_t *__restrict__ is_vehicle,
                                                    int n_classes, const double *__restrict__ lane_dist, double lane_min_dist,
                                                    const float *__restrict__ lane, const int32_t *__restrict__ lane_off,
                                                    const int32_t *__restrict__ frame_lane, const int32_t *__restrict__ lane_idx,
                                                    int n_tables, int n_lane_points, const float *__restrict__ pose_rt, int n_masks,
                                                    int n_frames, float *__restrict__ yaw_tab, int32_t *__restrict__ yaw_idx,
                                                    int32_t *__restrict__ yaw_src)
{
    const int m = blockIdx.x * blockDim.x + threadIdx.x;
    if (m >= n_masks) return;
    float yaw = 0.0f;
    int src = 0;
    if (medoid_pos[m] >= 0) {
        const int f = bf_clamp(mask_frame[m], n_frames);
        // the lane point k_box_nms reads for this mask (boxes.hip: lane[max(ltab + li, 0)]), kept inside the array
        const int ltab = lane_off[bf_clamp(frame_lane[f], n_tables)];
        const float yaw_l = lane[(size_t)bf_clamp(ltab + lane_idx[m], n_lane_points) * 3 + 2];
        yaw = yaw_l;
        int cls = class_id[m];
        if (cls < 0 || cls >= n_classes) cls = 0;
        if (fit_status[m] == 0 && is_vehicle[cls] && lane_dist[m] >= lane_min_dist) {
            double cg = fit_rect[(size_t)m * CM3D_MATCH_BOX_STRIDE + 4], sg = fit_rect[(size_t)m * CM3D_MATCH_BOX_STRIDE + 5];
            if (pose_rt) {                       // Waymo: the lists are in the vehicle frame, the lanes in the global one
                const float *R = pose_rt + (size_t)f * 12;
                const double c = cg, s = sg;
                cg = ((double)R[0] * c) + ((double)R[1] * s);
                sg = ((double)R[3] * c) + ((double)R[4] * s);
            }
            const double yl = (double)yaw_l;
            const double dot = (cg * cos(yl)) + (sg * sin(yl));
            if (dot < 0) cg = -cg, sg = -sg;     // the fit gives the axis, the map which way along it
            yaw = (float)atan2(sg, cg);
            src = 1;
        }
    }
    yaw_tab[3 * (size_t)m] = 0.0f, yaw_tab[3 * (size_t)m + 1] = 0.0f, yaw_tab[3 * (size_t)m + 2] = yaw;
    yaw_idx[m] = m;
    yaw_src[m] = src;
}

static bool bf_finite_host(double v) { return v - v == 0.0; }

extern "C" int cm3d_bev_fit(const float *hit_xyz, const int32_t *hit_off, int32_t n_masks, int32_t idx_cap, const double *angle_cs, int32_t K,
                            double d0, int32_t min_points, double min_length, int32_t *fit_k, double *fit_rect, int32_t *fit_status,
                            cm3d_stream_t stream)
{
    if (!hit_xyz || !hit_off || !angle_cs || !fit_k || !fit_rect || !fit_status) return CM3D_ERR_ARG;
    if (n_masks <= 0 || idx_cap <= 0) return CM3D_ERR_ARG;
    if (K < 64 || K > 64 * BF_MAX_WAVES || K % 64 != 0) return CM3D_ERR_ARG;
    if (!bf_finite_host(d0) || !(d0 > 0.0) || min_points < 2 || !bf_finite_host(min_length) || !(min_length >= 0.0)) return CM3D_ERR_ARG;
    if (((uintptr_t)hit_xyz & 15) != 0 || ((uintptr_t)angle_cs & 15) != 0) return CM3D_ERR_ARG;
    hipLaunchKernelGGL(k_bev_fit, dim3(n_masks), dim3(K), 0, (hipStream_t)stream, (const float4 *)hit_xyz, hit_off, idx_cap,
                       (const double2 *)angle_cs, d0, min_points, min_length, fit_k, fit_rect, fit_status);
    CM3D_CHECK_LAUNCH();
    return CM3D_OK;
}

extern "C" int cm3d_yaw_select(const double *fit_rect, const int32_t *fit_status, const int32_t *medoid_pos, const int32_t *mask_frame,
                               const int32_t *class_id, const int32_t *is_vehicle, int32_t n_classes, const double *lane_dist,
                               double lane_min_dist, const float *lane, const int32_t *lane_off, const int32_t *frame_lane,
                               const int32_t *lane_idx, int32_t n_tables, int32_t n_lane_points, const float *pose_rt, int32_t n_masks,
                               int32_t n_frames, float *yaw_tab, int32_t *yaw_idx, int32_t *yaw_src, cm3d_stream_t stream)
{
    if (!fit_rect || !fit_status || !medoid_pos || !mask_frame || !class_id || !is_vehicle || !lane_dist || !lane || !lane_off || !frame_lane ||
        !lane_idx || !yaw_tab || !yaw_idx || !yaw_src)
        return CM3D_ERR_ARG;
    if (n_masks <= 0 || n_frames <= 0 || n_classes <= 0 || n_tables <= 0 || n_lane_points <= 0) return CM3D_ERR_ARG;
    if (!(lane_min_dist >= 0.0)) return CM3D_ERR_ARG;                                              // (a NaN fails the comparison)
    hipLaunchKernelGGL(k_yaw_select, dim3((n_masks + 255) / 256), dim3(256), 0, (hipStream_t)stream, fit_rect, fit_status, medoid_pos,
                       mask_frame, class_id, is_vehicle, n_classes, lane_dist, lane_min_dist, lane, lane_off, frame_lane, lane_idx, n_tables,
                       n_lane_points, pose_rt, n_masks, n_frames, yaw_tab, yaw_idx, yaw_src);
    CM3D_CHECK_LAUNCH();
    return CM3D_OK;
}
