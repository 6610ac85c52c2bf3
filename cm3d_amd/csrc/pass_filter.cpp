// Host side of the opt-in filtered pass (cm3d_lift_pass_filtered, include/cm3d_hip.h): the plain pass, the stage-2 filter on what it
// left in device memory, and the box launch once more on the filtered medoid positions.  No kernel lives here, and csrc/pipeline.cpp
// knows nothing of this file: the plain pass and cm3d_pipe_submit stay what they are.
#include <hip/hip_runtime_api.h>

#include "../../include/cm3d_hip.h"

static int record(void *ev, cm3d_stream_t st)
{
    return !ev || hipEventRecord((hipEvent_t)ev, (hipStream_t)st) == hipSuccess ? CM3D_OK : CM3D_ERR_LAUNCH;
}

extern "C" int cm3d_lift_pass_filtered(const cm3d_lift_pass_desc *d, const cm3d_stage2_filter_desc *f, cm3d_stream_t st)
{
    if (!d || !f || f->size != (int64_t)sizeof(cm3d_stage2_filter_desc)) return CM3D_ERR_ARG;
    if (!f->medoid_pos_kept || !f->on_road) return CM3D_ERR_ARG;
    int rc;
    if ((rc = cm3d_lift_pass(d, st)) != CM3D_OK || (rc = record(f->ev[0], st)) != CM3D_OK) return rc;
    rc = cm3d_stage2_filter(d->centroid_g, d->medoid_pos, d->mask_frame, d->frame_lane, d->class_id, d->lane_dist, d->n_masks, d->n_frames,
                            f->tab_y, f->tab_slab, f->slab_off, f->ent_edge, f->ent_ring, f->edge, f->ring_info, f->n_poly_tables,
                            f->needs_road, d->is_vehicle, d->n_classes, f->lane_max_dist, f->vehicle_lane_max_dist, f->medoid_pos_kept,
                            f->on_road, st);
    if (rc != CM3D_OK || (rc = record(f->ev[1], st)) != CM3D_OK) return rc;
    // the boxes again, on the positions the filter kept: `box` and `flags` are written whole, so nothing of the first launch remains
    return cm3d_box_nms_bounded(d->centroid_g, f->medoid_pos_kept, d->mask_off, d->n_frames, d->n_masks, d->class_id, d->score, d->lane,
                                d->lane_off, d->frame_lane, d->lane_idx, d->lane_dist, d->prior_wlh, d->is_vehicle, d->nms_group, d->nms_thr,
                                d->n_classes, d->ego_xyz, d->pose_inv,
                                d->planes > 0 && d->planes < CM3D_MAX_MASKS_PER_FRAME / 32 ? 32 * d->planes : CM3D_MAX_MASKS_PER_FRAME,
                                d->box, d->flags, st);
}
