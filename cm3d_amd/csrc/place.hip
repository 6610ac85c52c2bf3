// Box centre from the fitted rectangle (opt-in, behind the yaw fit): cm3d_box_place of include/cm3d_hip.h.  k_box_nms puts a vehicle's
// centre at the medoid pushed along the view ray (push_centroid, src/nuscenes/2d_to_3d.py:164-198); here the sensor-side corner and
// faces of cm3d_bev_fit's rectangle carry the class's length and width instead, and the circle NMS is decided again on the new centres.
// All float64, every product, sum and difference rounded on its own (-ffp-contract=off); no library call: the host statement
// (cm3d_amd.boxplace.box_place_host) gives the same bits.  One wave per frame, latency-bound like k_box_nms; no HBM roofline applies.
#include "common.h"
#include "circle_nms.h"

static __device__ __forceinline__ bool bp_finite(double v) { return fabs(v) < INFINITY; }      // (NaN fails the comparison)

// WAYMO: lists, rectangles and boxes live in the vehicle frame, the sensor is its origin; else nuScenes: all global, the sensor is the
// frame's ego position.  cap: as in k_box_nms -- the launch's LDS is sized by it, the masks of a frame beyond it take no part.
template <bool WAYMO>
__global__ __launch_bounds__(64) void k_box_place(double *__restrict__ box, int32_t *__restrict__ flags, const int32_t *__restrict__ mask_off,
                                                  int n_masks, const double *__restrict__ fit_rect, const int32_t *__restrict__ yaw_src,
                                                  const double *__restrict__ prior_wlh, const int32_t *__restrict__ nms_group,
                                                  const double *__restrict__ nms_thr, int n_classes, const double *__restrict__ ego_xyz,
                                                  double thin, int cap, int32_t *__restrict__ place_src, double *__restrict__ place_pushed)
{
    extern __shared__ __align__(8) double s_bp[];
    const int cap8 = (cap + 7) & ~7;
    double *const s_x = s_bp, *const s_y = s_x + cap8, *const s_s = s_y + cap8;
    int *const s_lab = reinterpret_cast<int *>(s_s + cap8), *const s_order = s_lab + cap8;
    unsigned char *const s_valid = reinterpret_cast<unsigned char *>(s_order + cap8), *const s_sup = s_valid + cap8, *const s_keep = s_sup + cap8;
    const int f = blockIdx.x;
    // (a frame's range is clamped into the batch: no mask outside [0, n_masks) is addressed whatever mask_off holds)
    const int m0 = min(max(mask_off[f], 0), n_masks);
    const int n_all = min(max(mask_off[f + 1], m0), n_masks) - m0;
    const int nm = min(min(n_all, BN_MAX), cap);
    const int lane_id = threadIdx.x;
    const bool in_regs = nm <= 64;
    const double sx = WAYMO ? 0.0 : ego_xyz[3 * f], sy = WAYMO ? 0.0 : ego_xyz[3 * f + 1];
    const bool sensor_ok = bp_finite(sx) && bp_finite(sy);
    double r_x = 0.0, r_y = 0.0, r_s = 0.0, r_thr = 0.0;
    int r_lab = 0, r_fl = 0;
    bool r_valid = false;

    for (int k = lane_id; k < nm; k += 64) {
        const int m = m0 + k;
        double *b = box + (size_t)m * CM3D_BOX_STRIDE;
        const double *fr = fit_rect + (size_t)m * CM3D_MATCH_BOX_STRIDE;
        // (as in k_box_nms: everything indexed by the mask is requested before the first branch, the class's tables one round trip later)
        const int fl_in = flags[m], ys = yaw_src[m];
        const double bx = b[0], by = b[1], score_m = b[7], b8 = b[8];
        const double cx = fr[0], cy = fr[1], ra = fr[2], rb = fr[3], hc = fr[4], hs = fr[5];
        const int cls = b8 >= 0.0 && b8 < (double)n_classes ? (int)b8 : 0;              // what cm3d_box_rotated_nms reads of the record
        const double len = prior_wlh[3 * cls + 1], wid = prior_wlh[3 * cls + 0];      // the [w, l, h] table: length along the heading
        const int grp = nms_group[cls];
        const bool valid = (fl_in & 1) != 0;
        if (in_regs && valid) r_thr = nms_thr[grp];
        double x = bx, y = by;
        int src = 0;
        if (valid && ys == 1 && sensor_ok && bp_finite(cx) && bp_finite(cy) && bp_finite(ra) && bp_finite(rb) && bp_finite(hc) && bp_finite(hs)) {
            const double ex = sx - cx, ey = sy - cy;
            const double pu = (ex * hc) + (ey * hs), pv = (ey * hc) - (ex * hs);      // the sensor in the rectangle's axes
            const double su = pu >= 0.0 ? 1.0 : -1.0, sv = pv >= 0.0 ? 1.0 : -1.0;
            const bool au = rb >= thin, av = ra >= thin;                               // an axis is anchored at the corner when the face across it was seen
            const double du = au ? su * ((ra - len) * 0.5) : 0.0;
            const double dv = av ? sv * ((rb - wid) * 0.5) : 0.0;
            x = ((du * hc) - (dv * hs)) + cx;
            y = ((du * hs) + (dv * hc)) + cy;
            src = au && av ? 1 : (au || av ? 2 : 3);
            b[0] = x; b[1] = y;
        }
        place_src[m] = src;
        place_pushed[2 * (size_t)m] = bx; place_pushed[2 * (size_t)m + 1] = by;
        if (in_regs) {
            r_x = x; r_y = y; r_s = score_m; r_lab = grp; r_valid = valid; r_fl = fl_in;
        } else {
            s_x[k] = x; s_y[k] = y; s_s[k] = score_m; s_lab[k] = grp;
            s_valid[k] = valid; s_sup[k] = 0; s_keep[k] = 0;
        }
    }
    if (in_regs) {
        const uint64_t keep = nms_regs(nm, lane_id, r_valid, r_x, r_y, r_s, r_lab, r_thr);
        if (lane_id < nm) {
            const int fl = (r_fl & ~2) | ((keep >> lane_id) & 1 ? 2 : 0);
            flags[m0 + lane_id] = fl;
            box[(size_t)(m0 + lane_id) * CM3D_BOX_STRIDE + 9] = (double)fl;
        }
    } else {
        nms_phase(nm, lane_id, nms_thr, s_x, s_y, s_s, s_lab, s_order, s_valid, s_sup, s_keep);
        for (int k = lane_id; k < nm; k += 64) {
            const int fl = (flags[m0 + k] & ~2) | (s_keep[k] ? 2 : 0);
            flags[m0 + k] = fl;
            box[(size_t)(m0 + k) * CM3D_BOX_STRIDE + 9] = (double)fl;
        }
    }
    // masks beyond the launch's bound (the box launch gave them flags 0): not placed, not kept
    for (int k = nm + lane_id; k < n_all; k += 64) {
        const int m = m0 + k;
        double *b = box + (size_t)m * CM3D_BOX_STRIDE;
        const int fl = flags[m] & ~2;
        const double bx = b[0], by = b[1];
        place_src[m] = 0;
        place_pushed[2 * (size_t)m] = bx; place_pushed[2 * (size_t)m + 1] = by;
        flags[m] = fl;
        b[9] = (double)fl;
    }
}

extern "C" int cm3d_box_place(double *box, int32_t *flags, const int32_t *mask_off, int32_t n_frames, int32_t n_masks, const double *fit_rect,
                              const int32_t *yaw_src, const double *prior_wlh, const int32_t *nms_group, const double *nms_thr,
                              int32_t n_classes, const double *ego_xyz, int32_t waymo, double thin, int32_t max_masks_per_frame,
                              int32_t *place_src, double *place_pushed, cm3d_stream_t stream)
{
    if (!box || !flags || !mask_off || !fit_rect || !yaw_src || !prior_wlh || !nms_group || !nms_thr || (!waymo && !ego_xyz) || !place_src ||
        !place_pushed)
        return CM3D_ERR_ARG;
    if (n_frames <= 0 || n_masks <= 0 || n_classes <= 0 || max_masks_per_frame <= 0) return CM3D_ERR_ARG;
    if (!(thin >= 0.0) || !(thin < INFINITY)) return CM3D_ERR_ARG;                  // (NaN fails the first comparison)
    const int cap = max_masks_per_frame < BN_MAX ? max_masks_per_frame : BN_MAX;
    const size_t lds = bn_lds_bytes(cap);                                          // (at most 35 KiB: below the default limit)
    if (waymo)
        hipLaunchKernelGGL(k_box_place<true>, dim3(n_frames), dim3(64), lds, (hipStream_t)stream, box, flags, mask_off, n_masks, fit_rect, yaw_src,
                           prior_wlh, nms_group, nms_thr, n_classes, ego_xyz, thin, cap, place_src, place_pushed);
    else
        hipLaunchKernelGGL(k_box_place<false>, dim3(n_frames), dim3(64), lds, (hipStream_t)stream, box, flags, mask_off, n_masks, fit_rect, yaw_src,
                           prior_wlh, nms_group, nms_thr, n_classes, ego_xyz, thin, cap, place_src, place_pushed);
    CM3D_CHECK_LAUNCH();
    return CM3D_OK;
}
