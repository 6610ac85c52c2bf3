// Host side of every pass with a stage that cm3d_lift_pass_options has no member for (cm3d_lift_pass_composed, include/cm3d_hip.h): the
// point ownership and the ground strip in front of the clustering, the box placement in front of the rotated NMS, and between them the
// composed pass of csrc/pass_options.cpp behind its seam (csrc/pass_seam.h).  cm3d_lift_pass_placed, _stripped and _owned are this
// function with one argument required.  No kernel lives here, and pass_options.cpp knows nothing of this file.
#include <cfloat>

#include "../../include/cm3d_hip.h"
#include "pass_seam.h"

static bool usable(const cm3d_point_owner_desc *w)
{
    return w->size == (int64_t)sizeof *w && w->ow_owner && w->ow_off && w->ow_tile_off && w->ow_idx && w->ow_xyz && w->ow_status && w->ow_lost &&
           w->ws && cm3d_point_owner_check(w->rule, w->min_keep) == CM3D_OK;
}

static bool usable(const cm3d_ground_strip_desc *s, bool idx)
{
    return s->size == (int64_t)sizeof *s && s->origin && s->grid_z && s->grid_n && s->gs_off && s->gs_tile_off && s->gs_xyz && s->gs_status &&
           s->gs_dropped && (!idx || s->gs_idx) && s->ws &&
           cm3d_ground_strip_check(s->cell, s->down, s->up, s->quantile, s->min_points, s->margin, s->min_keep) == CM3D_OK;
}

static bool usable(const cm3d_box_place_desc *p, const cm3d_yaw_fit_desc *y)
{
    return p->size == (int64_t)sizeof *p && y && y->fit_rect && y->yaw_src && p->place_src && p->place_pushed && p->thin >= 0.0 && p->thin <= DBL_MAX;
}

extern "C" int cm3d_lift_pass_composed(const cm3d_lift_pass_desc *d, const cm3d_lift_pass_options *o, const cm3d_box_place_desc *p,
                                       const cm3d_ground_strip_desc *s, const cm3d_point_owner_desc *w, cm3d_stream_t st)
{
    if (!d || d->size != (int64_t)sizeof *d || (w && (!d->hit_idx || !usable(w))) || (s && !usable(s, d->hit_idx))) return CM3D_ERR_ARG;
    // the lists behind the ownership and the strip: their work list is built by the medoid stage (tile_work belongs to the raw lists)
    cm3d_lift_pass_desc owned = *d, g = *d;
    if (w) owned.hit_off = w->ow_off, owned.tile_off = w->ow_tile_off, owned.hit_idx = w->ow_idx, owned.hit_xyz = w->ow_xyz, g = owned;
    if (s) g.hit_off = s->gs_off, g.tile_off = s->gs_tile_off, g.hit_idx = d->hit_idx ? s->gs_idx : nullptr, g.hit_xyz = s->gs_xyz;
    g.tile_work = nullptr;
    const cm3d_lift_pass_desc *lists = w || s ? &g : d;          // d itself: the seam runs the head, or the plain pass
    if (cm3d_pass_seam_check(d, lists, o) != CM3D_OK || (p && !usable(p, o ? o->yaw : nullptr))) return CM3D_ERR_ARG;
    int rc;
    if (lists != d && (rc = cm3d_lift_pass_head(d, st)) != CM3D_OK) return rc;
    if (w) {
        if ((rc = record(w->ev[0], st)) != CM3D_OK) return rc;
        rc = cm3d_point_owner(d->hit_xyz, d->hit_idx, d->hit_off, d->mask_off, d->n_frames, d->n_masks, d->idx_cap, d->max_pts_per_frame, d->score,
                              w->rule, w->min_keep, w->ow_owner, w->ow_off, w->ow_tile_off, w->ow_idx, w->ow_xyz, w->ow_status, w->ow_lost, w->ws,
                              w->ws_bytes, st);
        if (rc != CM3D_OK || (rc = record(w->ev[1], st)) != CM3D_OK) return rc;
    }
    if (s) {
        if ((rc = record(s->ev[0], st)) != CM3D_OK) return rc;
        // the sweep rows: the cloud where the pass has materialised it, the raw rows otherwise (the strip never makes a pass materialise it)
        rc = cm3d_ground_grid(d->points, d->points ? d->pt_off : nullptr, d->raw, d->raw_stride, d->sweep_xf, d->sweep_row_off,
                              d->frame_sweep_off, d->n_sweeps, d->halfw, d->pt_cap, s->origin, d->n_frames, s->cell, s->down, s->up, s->quantile,
                              s->min_points, s->grid_z, s->grid_n, st);
        if (rc != CM3D_OK) return rc;
        rc = cm3d_ground_strip(owned.hit_xyz, owned.hit_idx, owned.hit_off, d->mask_frame, d->n_masks, d->idx_cap, s->origin, s->grid_z,
                               d->n_frames, s->cell, s->margin, s->min_keep, s->gs_off, s->gs_tile_off, g.hit_idx, s->gs_xyz, s->gs_status,
                               s->gs_dropped, s->ws, s->ws_bytes, st);
        if (rc != CM3D_OK || (rc = record(s->ev[1], st)) != CM3D_OK) return rc;
    }
    // with a placement the rotated NMS belongs behind it
    cm3d_lift_pass_options front;
    if (p) front = *o, front.nms = nullptr;
    if ((rc = cm3d_pass_seam_run(d, lists, p ? &front : o, st)) != CM3D_OK || !p) return rc;
    const cm3d_yaw_fit_desc *y = o->yaw;
    const cm3d_rotated_nms_desc *n = o->nms;
    if ((rc = record(p->ev[0], st)) != CM3D_OK) return rc;
    rc = cm3d_box_place(d->box, d->flags, d->mask_off, d->n_frames, d->n_masks, y->fit_rect, y->yaw_src, d->prior_wlh, d->nms_group, d->nms_thr,
                        d->n_classes, d->ego_xyz, d->pose_inv != nullptr, p->thin, bound(d), p->place_src, p->place_pushed, st);
    if (rc != CM3D_OK || (rc = record(p->ev[1], st)) != CM3D_OK) return rc;
    if (n)
        rc = cm3d_box_rotated_nms(d->box, d->flags, d->mask_off, d->n_frames, d->n_masks, d->class_id, d->prior_wlh, d->nms_group,
                                  d->n_classes, n->thr, n->n_thr, n->measure, n->class_agnostic, d->pose_inv != nullptr, bound(d), st);
    return rc;
}

extern "C" {
int cm3d_lift_pass_placed(const cm3d_lift_pass_desc *d, const cm3d_lift_pass_options *o, const cm3d_box_place_desc *p, cm3d_stream_t st)
{
    return o && p ? cm3d_lift_pass_composed(d, o, p, nullptr, nullptr, st) : CM3D_ERR_ARG;
}
int cm3d_lift_pass_stripped(const cm3d_lift_pass_desc *d, const cm3d_lift_pass_options *o, const cm3d_box_place_desc *p,
                            const cm3d_ground_strip_desc *s, cm3d_stream_t st)
{
    return s ? cm3d_lift_pass_composed(d, o, p, s, nullptr, st) : CM3D_ERR_ARG;
}
int cm3d_lift_pass_owned(const cm3d_lift_pass_desc *d, const cm3d_lift_pass_options *o, const cm3d_box_place_desc *p,
                         const cm3d_ground_strip_desc *s, const cm3d_point_owner_desc *w, cm3d_stream_t st)
{
    return w ? cm3d_lift_pass_composed(d, o, p, s, w, st) : CM3D_ERR_ARG;
}
}
