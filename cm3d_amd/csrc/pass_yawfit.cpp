// Host side of the opt-in yaw-fitted pass (cm3d_lift_pass_yaw_fitted, cm3d_yaw_fit_boxes; include/cm3d_hip.h): the plain pass, the
// L-shape fit of every in-mask list, the choice between the fitted axis and the lane's yaw, and the box launch once more with the
// chosen yaws standing where the lane tables stood.  No kernel lives here, k_box_nms is what it was, and csrc/pipeline.cpp knows
// nothing of this file: the plain pass and cm3d_pipe_submit stay what they are.
#include <hip/hip_runtime_api.h>

#include "../../include/cm3d_hip.h"

static int record(void *ev, cm3d_stream_t st)
{
    return !ev || hipEventRecord((hipEvent_t)ev, (hipStream_t)st) == hipSuccess ? CM3D_OK : CM3D_ERR_LAUNCH;
}

static bool usable(const cm3d_lift_pass_desc *d, const cm3d_yaw_fit_desc *y)
{
    if (!d || !y || d->size != (int64_t)sizeof(cm3d_lift_pass_desc) || y->size != (int64_t)sizeof(cm3d_yaw_fit_desc)) return false;
    return y->angle_cs && y->fit_k && y->fit_rect && y->fit_status && y->yaw_tab && y->yaw_idx && y->yaw_src && y->tab_off && y->tab_frame;
}

extern "C" int cm3d_yaw_fit_boxes(const cm3d_lift_pass_desc *d, const cm3d_yaw_fit_desc *y, cm3d_stream_t st)
{
    if (!usable(d, y)) return CM3D_ERR_ARG;
    const float *xyz = y->hit_xyz ? y->hit_xyz : d->hit_xyz;
    const int32_t *off = y->hit_off ? y->hit_off : d->hit_off;
    const int32_t *pos = y->medoid_pos ? y->medoid_pos : d->medoid_pos;
    int rc;
    if ((rc = record(y->ev[0], st)) != CM3D_OK) return rc;
    rc = cm3d_bev_fit(xyz, off, d->n_masks, d->idx_cap, y->angle_cs, y->K, y->d0, y->min_points, y->min_length, y->fit_k, y->fit_rect,
                      y->fit_status, st);
    if (rc != CM3D_OK) return rc;
    rc = cm3d_yaw_select(y->fit_rect, y->fit_status, pos, d->mask_frame, d->class_id, d->is_vehicle, d->n_classes, d->lane_dist,
                         y->lane_min_dist, d->lane, d->lane_off, d->frame_lane, d->lane_idx, d->n_tables, d->n_lane_points, d->pose_rt,
                         d->n_masks, d->n_frames, y->yaw_tab, y->yaw_idx, y->yaw_src, st);
    if (rc != CM3D_OK || (rc = record(y->ev[1], st)) != CM3D_OK) return rc;
    // the boxes again: k_box_nms takes a mask's yaw from lane[lane_off[frame_lane[f]] + lane_idx[m]] and reads nothing else of a lane
    // point, so one table of M rows, every frame on table 0 and lane_idx[m] = m hand it the chosen yaws; `box` and `flags` are
    // written whole, so nothing of the first launch remains
    return cm3d_box_nms_bounded(d->centroid_g, pos, d->mask_off, d->n_frames, d->n_masks, d->class_id, d->score, y->yaw_tab, y->tab_off,
                                y->tab_frame, y->yaw_idx, d->lane_dist, d->prior_wlh, d->is_vehicle, d->nms_group, d->nms_thr, d->n_classes,
                                d->ego_xyz, d->pose_inv,
                                d->planes > 0 && d->planes < CM3D_MAX_MASKS_PER_FRAME / 32 ? 32 * d->planes : CM3D_MAX_MASKS_PER_FRAME,
                                d->box, d->flags, st);
}

extern "C" int cm3d_lift_pass_yaw_fitted(const cm3d_lift_pass_desc *d, const cm3d_yaw_fit_desc *y, cm3d_stream_t st)
{
    if (!usable(d, y)) return CM3D_ERR_ARG;
    const int rc = cm3d_lift_pass(d, st);
    return rc != CM3D_OK ? rc : cm3d_yaw_fit_boxes(d, y, st);
}
