// Host side of the owned pass (cm3d_lift_pass_owned, include/cm3d_hip.h): the head of the plain pass, the point ownership on the raw
// in-mask lists, the ground grid and the strip on the exclusive lists where there is a strip, then the composed pass of
// csrc/pass_options.cpp behind its seam on the lists that are left -- without its rotated NMS where there is a placement, which stands
// in front of it as in csrc/pass_strip.cpp.  No kernel lives here, and pass_options.cpp, pass_strip.cpp and pass_place.cpp know nothing
// of the ownership: cm3d_lift_pass_opt, cm3d_lift_pass_placed and cm3d_lift_pass_stripped stay what they are.
#include <hip/hip_runtime_api.h>

#include "../../include/cm3d_hip.h"
#include "pass_seam.h"

static int record(void *ev, cm3d_stream_t st)
{
    return !ev || hipEventRecord((hipEvent_t)ev, (hipStream_t)st) == hipSuccess ? CM3D_OK : CM3D_ERR_LAUNCH;
}

static int32_t bound(const cm3d_lift_pass_desc *d)          // no frame has more than 32 * planes masks (as the box launch's)
{
    return d->planes > 0 && d->planes < CM3D_MAX_MASKS_PER_FRAME / 32 ? 32 * d->planes : CM3D_MAX_MASKS_PER_FRAME;
}

static bool usable(const cm3d_ground_strip_desc *s)
{
    return s->size == (int64_t)sizeof *s && s->origin && s->grid_z && s->grid_n && s->gs_off && s->gs_tile_off && s->gs_xyz && s->gs_status &&
           s->gs_dropped && s->gs_idx && s->ws &&
           cm3d_ground_strip_check(s->cell, s->down, s->up, s->quantile, s->min_points, s->margin, s->min_keep) == CM3D_OK;
}

static bool usable(const cm3d_point_owner_desc *w)
{
    return w->size == (int64_t)sizeof *w && w->ow_owner && w->ow_off && w->ow_tile_off && w->ow_idx && w->ow_xyz && w->ow_status && w->ow_lost &&
           w->ws && cm3d_point_owner_check(w->rule, w->min_keep) == CM3D_OK;
}

extern "C" int cm3d_lift_pass_owned(const cm3d_lift_pass_desc *d, const cm3d_lift_pass_options *o, const cm3d_box_place_desc *p,
                                    const cm3d_ground_strip_desc *s, const cm3d_point_owner_desc *w, cm3d_stream_t st)
{
    if (!d || d->size != (int64_t)sizeof *d || !d->hit_idx || !w || !usable(w) || (s && !usable(s))) return CM3D_ERR_ARG;
    // the lists behind the ownership and the strip: their work list is built by the medoid stage (tile_work belongs to the raw lists)
    cm3d_lift_pass_desc g = *d;
    g.hit_off = w->ow_off, g.tile_off = w->ow_tile_off, g.hit_idx = w->ow_idx, g.hit_xyz = w->ow_xyz, g.tile_work = nullptr;
    const cm3d_lift_pass_desc owned = g;
    if (s) g.hit_off = s->gs_off, g.tile_off = s->gs_tile_off, g.hit_idx = s->gs_idx, g.hit_xyz = s->gs_xyz;
    if (cm3d_pass_seam_check(d, &g, o) != CM3D_OK) return CM3D_ERR_ARG;
    const cm3d_yaw_fit_desc *y = o ? o->yaw : nullptr;
    const cm3d_rotated_nms_desc *n = o ? o->nms : nullptr;
    if (p && (p->size != (int64_t)sizeof *p || !y || !y->fit_rect || !y->yaw_src || !p->place_src || !p->place_pushed || !(p->thin >= 0.0) ||
              !(p->thin <= 1.7976931348623157e308)))
        return CM3D_ERR_ARG;
    int rc;
    if ((rc = cm3d_lift_pass_head(d, st)) != CM3D_OK || (rc = record(w->ev[0], st)) != CM3D_OK) return rc;
    rc = cm3d_point_owner(d->hit_xyz, d->hit_idx, d->hit_off, d->mask_off, d->n_frames, d->n_masks, d->idx_cap, d->max_pts_per_frame, d->score,
                          w->rule, w->min_keep, w->ow_owner, w->ow_off, w->ow_tile_off, w->ow_idx, w->ow_xyz, w->ow_status, w->ow_lost, w->ws,
                          w->ws_bytes, st);
    if (rc != CM3D_OK || (rc = record(w->ev[1], st)) != CM3D_OK) return rc;
    if (s) {
        if ((rc = record(s->ev[0], st)) != CM3D_OK) return rc;
        // the sweep rows: the cloud where the pass has materialised it, the raw rows otherwise
        rc = cm3d_ground_grid(d->points, d->points ? d->pt_off : nullptr, d->raw, d->raw_stride, d->sweep_xf, d->sweep_row_off,
                              d->frame_sweep_off, d->n_sweeps, d->halfw, d->pt_cap, s->origin, d->n_frames, s->cell, s->down, s->up, s->quantile,
                              s->min_points, s->grid_z, s->grid_n, st);
        if (rc != CM3D_OK) return rc;
        rc = cm3d_ground_strip(owned.hit_xyz, owned.hit_idx, owned.hit_off, d->mask_frame, d->n_masks, d->idx_cap, s->origin, s->grid_z,
                               d->n_frames, s->cell, s->margin, s->min_keep, s->gs_off, s->gs_tile_off, s->gs_idx, s->gs_xyz, s->gs_status,
                               s->gs_dropped, s->ws, s->ws_bytes, st);
        if (rc != CM3D_OK || (rc = record(s->ev[1], st)) != CM3D_OK) return rc;
    }
    if (!p) return cm3d_pass_seam_run(d, &g, o, st);
    // with a placement the rotated NMS belongs behind it
    cm3d_lift_pass_options front = *o;
    front.nms = nullptr;
    if ((rc = cm3d_pass_seam_run(d, &g, &front, st)) != CM3D_OK || (rc = record(p->ev[0], st)) != CM3D_OK) return rc;
    rc = cm3d_box_place(d->box, d->flags, d->mask_off, d->n_frames, d->n_masks, y->fit_rect, y->yaw_src, d->prior_wlh, d->nms_group, d->nms_thr,
                        d->n_classes, d->ego_xyz, d->pose_inv != nullptr, p->thin, bound(d), p->place_src, p->place_pushed, st);
    if (rc != CM3D_OK || (rc = record(p->ev[1], st)) != CM3D_OK) return rc;
    if (n)
        rc = cm3d_box_rotated_nms(d->box, d->flags, d->mask_off, d->n_frames, d->n_masks, d->class_id, d->prior_wlh, d->nms_group,
                                  d->n_classes, n->thr, n->n_thr, n->measure, n->class_agnostic, d->pose_inv != nullptr, bound(d), st);
    return rc;
}
