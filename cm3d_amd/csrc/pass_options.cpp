// Host side of the opt-in stages of a pass (cm3d_lift_pass_opt, include/cm3d_hip.h): the depth clustering between the halves of the
// plain pass, and behind it the stage-2 filter, the yaw fit and the rotated-box NMS.  The only statement of a composed pass's order
// (the composer of the stages in front of the clustering enters it behind the seam, on the lists those leave, through cm3d_pass_seam_run
// below; record() and bound() come from csrc/pass_seam.h).  No
// kernel lives here, and csrc/pipeline.cpp knows nothing of this file: the plain pass and cm3d_pipe_submit stay what they are.
#include "../../include/cm3d_hip.h"
#include "pass_seam.h"

// the box launch of the plain pass once more, on other positions or other lane tables: `box` and `flags` are written whole, so nothing
// of an earlier launch remains
static int boxes(const cm3d_lift_pass_desc *d, const int32_t *pos, const float *lane, const int32_t *lane_off, const int32_t *frame_lane,
                 const int32_t *lane_idx, cm3d_stream_t st)
{
    return cm3d_box_nms_bounded(d->centroid_g, pos, d->mask_off, d->n_frames, d->n_masks, d->class_id, d->score, lane, lane_off, frame_lane,
                                lane_idx, d->lane_dist, d->prior_wlh, d->is_vehicle, d->nms_group, d->nms_thr, d->n_classes, d->ego_xyz,
                                d->pose_inv, bound(d), d->box, d->flags, st);
}

static bool usable(const cm3d_lift_pass_desc *d) { return d && d->size == (int64_t)sizeof *d; }
static bool usable(const cm3d_depth_cluster_desc *c, bool idx)
{
    return c->size == (int64_t)sizeof *c && c->cl_off && c->cl_tile_off && c->cl_xyz && c->cl_status && (!idx || c->cl_idx);
}
static bool usable(const cm3d_stage2_filter_desc *f) { return f->size == (int64_t)sizeof *f && f->medoid_pos_kept && f->on_road; }
static bool usable(const cm3d_yaw_fit_desc *y)
{
    return y->size == (int64_t)sizeof *y && y->angle_cs && y->fit_k && y->fit_rect && y->fit_status && y->yaw_tab && y->yaw_idx && y->yaw_src &&
           y->tab_off && y->tab_frame;
}
static bool usable(const cm3d_rotated_nms_desc *n) { return n->size == (int64_t)sizeof *n && n->thr; }

// the fit, the choice, and the boxes with yaw_tab as every frame's lane table: k_box_nms reads nothing of a lane point but its yaw
static int yaw_fit(const cm3d_lift_pass_desc *d, const cm3d_yaw_fit_desc *y, const float *xyz, const int32_t *off, const int32_t *pos,
                   cm3d_stream_t st)
{
    int rc;
    if ((rc = record(y->ev[0], st)) != CM3D_OK) return rc;
    rc = cm3d_bev_fit(xyz, off, d->n_masks, d->idx_cap, y->angle_cs, y->K, y->d0, y->min_points, y->min_length, y->fit_k, y->fit_rect,
                      y->fit_status, st);
    if (rc != CM3D_OK) return rc;
    rc = cm3d_yaw_select(y->fit_rect, y->fit_status, pos, d->mask_frame, d->class_id, d->is_vehicle, d->n_classes, d->lane_dist,
                         y->lane_min_dist, d->lane, d->lane_off, d->frame_lane, d->lane_idx, d->n_tables, d->n_lane_points, d->pose_rt,
                         d->n_masks, d->n_frames, y->yaw_tab, y->yaw_idx, y->yaw_src, st);
    if (rc != CM3D_OK || (rc = record(y->ev[1], st)) != CM3D_OK) return rc;
    return boxes(d, pos, y->yaw_tab, y->tab_off, y->tab_frame, y->yaw_idx, st);
}

extern "C" int cm3d_yaw_fit_boxes(const cm3d_lift_pass_desc *d, const cm3d_yaw_fit_desc *y, cm3d_stream_t st)
{
    if (!usable(d) || !y || !usable(y)) return CM3D_ERR_ARG;
    return yaw_fit(d, y, y->hit_xyz ? y->hit_xyz : d->hit_xyz, y->hit_off ? y->hit_off : d->hit_off,
                   y->medoid_pos ? y->medoid_pos : d->medoid_pos, st);
}

// A composed pass behind the seam, on the lists of `l`: `d` itself (nothing has been enqueued yet: the head runs here), or a copy of `d`
// with other lists in hit_off, tile_off, hit_idx, hit_xyz and no tile_work (the head has run and something stands between it and the
// clustering).  Every descriptor has been checked.
static int behind(const cm3d_lift_pass_desc *d, const cm3d_lift_pass_desc *l, const cm3d_depth_cluster_desc *c, const cm3d_stage2_filter_desc *f,
                  const cm3d_yaw_fit_desc *y, const cm3d_rotated_nms_desc *n, cm3d_stream_t st)
{
    // what the later stages read: the clustered lists when there are any, the positions the filter kept when there is one
    const float *xyz = c ? c->cl_xyz : l->hit_xyz;
    const int32_t *off = c ? c->cl_off : l->hit_off;
    const int32_t *pos = f ? f->medoid_pos_kept : d->medoid_pos;
    int rc;
    if (c) {
        if ((l == d && (rc = cm3d_lift_pass_head(d, st)) != CM3D_OK) || (rc = record(c->ev[0], st)) != CM3D_OK) return rc;
        rc = cm3d_depth_cluster(l->hit_xyz, l->hit_idx, l->hit_off, d->mask_frame, d->n_masks, d->idx_cap, c->origin, d->n_frames, c->eps,
                                c->min_points, c->pick, c->cl_off, c->cl_tile_off, l->hit_idx ? c->cl_idx : nullptr, c->cl_xyz, c->cl_status,
                                c->ws, c->ws_bytes, st);
        if (rc != CM3D_OK || (rc = record(c->ev[1], st)) != CM3D_OK) return rc;
        // the rest of the pass on the clustered lists; their work list is built by the medoid stage (tile_work belongs to the raw lists)
        cm3d_lift_pass_desc t = *d;
        t.hit_off = c->cl_off, t.tile_off = c->cl_tile_off, t.hit_idx = c->cl_idx, t.hit_xyz = c->cl_xyz, t.tile_work = nullptr;
        rc = cm3d_lift_pass_tail(&t, st);
    } else
        rc = l == d ? cm3d_lift_pass(d, st) : cm3d_lift_pass_tail(l, st);
    if (rc != CM3D_OK) return rc;
    if (f) {
        if ((rc = record(f->ev[0], st)) != CM3D_OK) return rc;
        rc = cm3d_stage2_filter(d->centroid_g, d->medoid_pos, d->mask_frame, d->frame_lane, d->class_id, d->lane_dist, d->n_masks, d->n_frames,
                                f->tab_y, f->tab_slab, f->slab_off, f->ent_edge, f->ent_ring, f->edge, f->ring_info, f->n_poly_tables,
                                f->needs_road, d->is_vehicle, d->n_classes, f->lane_max_dist, f->vehicle_lane_max_dist, f->medoid_pos_kept,
                                f->on_road, st);
        if (rc != CM3D_OK || (rc = record(f->ev[1], st)) != CM3D_OK) return rc;
        if ((rc = boxes(d, pos, d->lane, d->lane_off, d->frame_lane, d->lane_idx, st)) != CM3D_OK) return rc;
    }
    if (y && (rc = yaw_fit(d, y, xyz, off, pos, st)) != CM3D_OK) return rc;
    if (n)
        rc = cm3d_box_rotated_nms(d->box, d->flags, d->mask_off, d->n_frames, d->n_masks, d->class_id, d->prior_wlh, d->nms_group,
                                  d->n_classes, n->thr, n->n_thr, n->measure, n->class_agnostic, d->pose_inv != nullptr, bound(d), st);
    return rc;
}

// every present descriptor, and yaw's own statement of its lists and positions: each NULL or what `behind` derives for the lists of `l`
static bool checked(const cm3d_lift_pass_desc *d, const cm3d_lift_pass_desc *l, const cm3d_lift_pass_options *o)
{
    if (!usable(d) || !l || (o && o->size != (int64_t)sizeof *o)) return false;
    if (!o) return true;
    const auto *c = o->cluster;
    const auto *f = o->filter;
    const auto *y = o->yaw;
    const auto *n = o->nms;
    if ((c && !usable(c, l->hit_idx)) || (f && !usable(f)) || (y && !usable(y)) || (n && !usable(n))) return false;
    const float *xyz = c ? c->cl_xyz : l->hit_xyz;
    const int32_t *off = c ? c->cl_off : l->hit_off;
    const int32_t *pos = f ? f->medoid_pos_kept : d->medoid_pos;
    return !(y && ((y->hit_xyz && y->hit_xyz != xyz) || (y->hit_off && y->hit_off != off) || (y->medoid_pos && y->medoid_pos != pos)));
}

extern "C" int cm3d_lift_pass_opt(const cm3d_lift_pass_desc *d, const cm3d_lift_pass_options *o, cm3d_stream_t st)
{
    if (o && o->size != (int64_t)sizeof *o) return CM3D_ERR_ARG;
    if (!o || (!o->cluster && !o->filter && !o->yaw && !o->nms)) return cm3d_lift_pass(d, st);
    if (!checked(d, d, o)) return CM3D_ERR_ARG;
    return behind(d, d, o->cluster, o->filter, o->yaw, o->nms, st);
}

// The seam for the composer (declared in csrc/pass_seam.h, no part of include/cm3d_hip.h): the check of a composed pass's
// descriptors for the lists of `l`, and the pass behind the seam on them (opt may be NULL: the tail alone).
extern "C" int cm3d_pass_seam_check(const cm3d_lift_pass_desc *d, const cm3d_lift_pass_desc *l, const cm3d_lift_pass_options *o)
{
    return checked(d, l, o) ? CM3D_OK : CM3D_ERR_ARG;
}

extern "C" int cm3d_pass_seam_run(const cm3d_lift_pass_desc *d, const cm3d_lift_pass_desc *l, const cm3d_lift_pass_options *o, cm3d_stream_t st)
{
    if (!checked(d, l, o)) return CM3D_ERR_ARG;
    return behind(d, l, o ? o->cluster : nullptr, o ? o->filter : nullptr, o ? o->yaw : nullptr, o ? o->nms : nullptr, st);
}

// the single-option passes: cm3d_lift_pass_opt with that member set (a null member is an error here, not the plain pass)
static int only(const cm3d_lift_pass_desc *d, const cm3d_depth_cluster_desc *c, const cm3d_stage2_filter_desc *f, const cm3d_yaw_fit_desc *y,
                cm3d_stream_t st)
{
    const cm3d_lift_pass_options o = {(int64_t)sizeof o, c, f, y, nullptr};
    return c || f || y ? cm3d_lift_pass_opt(d, &o, st) : CM3D_ERR_ARG;
}

extern "C" {
int cm3d_lift_pass_clustered(const cm3d_lift_pass_desc *d, const cm3d_depth_cluster_desc *c, cm3d_stream_t st) { return only(d, c, nullptr, nullptr, st); }
int cm3d_lift_pass_filtered(const cm3d_lift_pass_desc *d, const cm3d_stage2_filter_desc *f, cm3d_stream_t st) { return only(d, nullptr, f, nullptr, st); }
int cm3d_lift_pass_yaw_fitted(const cm3d_lift_pass_desc *d, const cm3d_yaw_fit_desc *y, cm3d_stream_t st) { return only(d, nullptr, nullptr, y, st); }
}
