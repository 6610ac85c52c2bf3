// Host side of the placed pass (cm3d_lift_pass_placed, include/cm3d_hip.h): the composed pass of csrc/pass_options.cpp without its rotated
// NMS, cm3d_box_place on the rectangles the yaw fit left, then the rotated NMS.  No kernel lives here, and pass_options.cpp knows nothing
// of this file: cm3d_lift_pass_opt and cm3d_lift_pass_options stay what they are.
#include <hip/hip_runtime_api.h>

#include "../../include/cm3d_hip.h"

static int record(void *ev, cm3d_stream_t st)
{
    return !ev || hipEventRecord((hipEvent_t)ev, (hipStream_t)st) == hipSuccess ? CM3D_OK : CM3D_ERR_LAUNCH;
}

static int32_t bound(const cm3d_lift_pass_desc *d)          // no frame has more than 32 * planes masks (as the box launch's)
{
    return d->planes > 0 && d->planes < CM3D_MAX_MASKS_PER_FRAME / 32 ? 32 * d->planes : CM3D_MAX_MASKS_PER_FRAME;
}

extern "C" int cm3d_lift_pass_placed(const cm3d_lift_pass_desc *d, const cm3d_lift_pass_options *o, const cm3d_box_place_desc *p,
                                     cm3d_stream_t st)
{
    if (!d || d->size != (int64_t)sizeof *d || !o || o->size != (int64_t)sizeof *o || !p || p->size != (int64_t)sizeof *p) return CM3D_ERR_ARG;
    const cm3d_yaw_fit_desc *y = o->yaw;
    const cm3d_rotated_nms_desc *n = o->nms;
    if (!y || y->size != (int64_t)sizeof *y || !y->fit_rect || !y->yaw_src) return CM3D_ERR_ARG;
    if (!p->place_src || !p->place_pushed || !(p->thin >= 0.0) || !(p->thin <= 1.7976931348623157e308)) return CM3D_ERR_ARG;
    if (n && (n->size != (int64_t)sizeof *n || !n->thr)) return CM3D_ERR_ARG;
    // the pass in front, without the rotated NMS: it belongs behind the placement (cm3d_lift_pass_opt checks the other members first
    // and makes no call when one is bad)
    cm3d_lift_pass_options front = *o;
    front.nms = nullptr;
    int rc;
    if ((rc = cm3d_lift_pass_opt(d, &front, st)) != CM3D_OK || (rc = record(p->ev[0], st)) != CM3D_OK) return rc;
    rc = cm3d_box_place(d->box, d->flags, d->mask_off, d->n_frames, d->n_masks, y->fit_rect, y->yaw_src, d->prior_wlh, d->nms_group, d->nms_thr,
                        d->n_classes, d->ego_xyz, d->pose_inv != nullptr, p->thin, bound(d), p->place_src, p->place_pushed, st);
    if (rc != CM3D_OK || (rc = record(p->ev[1], st)) != CM3D_OK) return rc;
    if (n)
        rc = cm3d_box_rotated_nms(d->box, d->flags, d->mask_off, d->n_frames, d->n_masks, d->class_id, d->prior_wlh, d->nms_group,
                                  d->n_classes, n->thr, n->n_thr, n->measure, n->class_agnostic, d->pose_inv != nullptr, bound(d), st);
    return rc;
}
