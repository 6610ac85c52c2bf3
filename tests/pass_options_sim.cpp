// Stand-alone trace of cm3d_lift_pass_opt, the three single-option passes and cm3d_yaw_fit_boxes (cm3d_amd/csrc/pass_options.cpp) over
// stubs of the nine entry points they call and of hipEventRecord (tests/pass_options_trace.py builds it with the address and
// undefined-behaviour sanitizers; the host tests compare the output with the sequence include/cm3d_hip.h states).  Per case: the calls
// of a clean pass, one line each with the arguments that matter, then `rc`; then, for every call k of that pass, `fail k rc calls`: the
// pass again with call k answering an error.
#include <hip/hip_runtime_api.h>

#include <cstdint>
#include <cstdio>
#include <cstring>
#include <functional>

#include "../include/cm3d_hip.h"

static int g_calls = 0, g_fail_at = -1;
static bool g_trace = true;

static bool fails() { return g_calls++ == g_fail_at; }
#define CALLED(bad, ok, ...)            \
    do {                                \
        if (g_trace) {                  \
            std::printf(__VA_ARGS__);   \
            std::printf("\n");          \
        }                               \
        return fails() ? bad : ok;      \
    } while (0)
static unsigned id(const void *p) { return (unsigned)(uintptr_t)p; }
static const char *set(const void *p) { return p ? "set" : "null"; }

// what the pass owns and what each stage owns: the stubs say whose array they were handed
static int32_t g_hit_off[4], g_tile_off[4], g_hit_idx[4], g_tile_work[4], g_cl_off[4], g_cl_tile_off[4], g_cl_idx[4], g_cl_status[4],
    g_medoid_pos[4], g_kept[4], g_lane_off[4], g_frame_lane[4], g_lane_idx[4], g_mask_frame[4], g_class[4], g_veh[4], g_fit_k[4],
    g_fit_status[4], g_yaw_idx[4], g_yaw_src[4], g_tab_off[2], g_tab_frame[4], g_mask_off[4], g_flags[4], g_group[4], g_poly_i[4];
static float g_hit_xyz[4], g_cl_xyz[4], g_lane[4], g_yaw_tab[4], g_centroid[4], g_pose_rt[12], g_pose_inv[16];
static double g_cs[4], g_rect[8], g_lane_dist[4], g_score[4], g_prior[4], g_thr[4], g_rot_thr[4], g_ego[4], g_box[4], g_origin[4], g_poly_d[4];
static uint8_t g_ws[16], g_on_road[4];

struct Name { const void *p; const char *n; };
static const char *who(const void *p)
{
    const Name names[] = {{g_hit_off, "hit_off"}, {g_tile_off, "tile_off"}, {g_hit_idx, "hit_idx"}, {g_tile_work, "tile_work"}, {g_cl_off, "cl_off"},
                          {g_cl_tile_off, "cl_tile_off"}, {g_cl_idx, "cl_idx"}, {g_medoid_pos, "medoid_pos"}, {g_kept, "kept"},
                          {g_lane_off, "lane_off"}, {g_frame_lane, "frame_lane"}, {g_lane_idx, "lane_idx"}, {g_yaw_idx, "yaw_idx"},
                          {g_tab_off, "tab_off"}, {g_tab_frame, "tab_frame"}, {g_hit_xyz, "hit_xyz"}, {g_cl_xyz, "cl_xyz"}, {g_lane, "lane"},
                          {g_yaw_tab, "yaw_tab"}, {g_pose_rt, "pose_rt"}, {g_pose_inv, "pose_inv"}, {g_lane_dist, "lane_dist"}, {g_box, "box"},
                          {g_flags, "flags"}, {g_centroid, "centroid"}, {g_on_road, "on_road"}, {g_mask_off, "mask_off"}, {g_rot_thr, "rot_thr"}};
    if (!p) return "null";
    for (const Name &e : names)
        if (e.p == p) return e.n;
    return "other";
}

extern "C" {
hipError_t hipEventRecord(hipEvent_t ev, hipStream_t) { CALLED(hipErrorInvalidValue, hipSuccess, "record %#x", id(ev)); }

static int part(const char *name, const cm3d_lift_pass_desc *d)
{
    CALLED(CM3D_ERR_LAUNCH, CM3D_OK, "%s size=%s hit_off=%s tile_off=%s hit_idx=%s hit_xyz=%s tile_work=%s n_masks=%d", name,
           d->size == (int64_t)sizeof *d ? "ok" : "bad", who(d->hit_off), who(d->tile_off), who(d->hit_idx), who(d->hit_xyz), who(d->tile_work),
           d->n_masks);
}
int cm3d_lift_pass(const cm3d_lift_pass_desc *d, cm3d_stream_t) { return part("cm3d_lift_pass", d); }
int cm3d_lift_pass_head(const cm3d_lift_pass_desc *d, cm3d_stream_t) { return part("cm3d_lift_pass_head", d); }
int cm3d_lift_pass_tail(const cm3d_lift_pass_desc *d, cm3d_stream_t) { return part("cm3d_lift_pass_tail", d); }
int cm3d_depth_cluster(const float *hit_xyz, const int32_t *hit_idx, const int32_t *hit_off, const int32_t *mask_frame, int32_t n_masks,
                       int32_t idx_cap, const double *origin, int32_t n_frames, double eps, int32_t min_points, int32_t pick, int32_t *cl_off,
                       int32_t *cl_tile_off, int32_t *cl_idx, float *cl_xyz, int32_t *cl_status, void *workspace, int64_t workspace_bytes,
                       cm3d_stream_t)
{
    CALLED(CM3D_ERR_WORKSPACE, CM3D_OK,
           "cm3d_depth_cluster in=%s,%s,%s frame=%s n=%d,%d,%d origin=%s eps=%g min=%d pick=%d out=%s,%s,%s,%s status=%s ws=%s,%lld",
           who(hit_xyz), who(hit_idx), who(hit_off), mask_frame == g_mask_frame ? "set" : "other", n_masks, idx_cap, n_frames,
           origin == g_origin ? "set" : "other", eps, min_points, pick, who(cl_off), who(cl_tile_off), who(cl_idx), who(cl_xyz),
           cl_status == g_cl_status ? "set" : "other", workspace == g_ws ? "set" : "other", (long long)workspace_bytes);
}
int cm3d_stage2_filter(const float *centroid_g, const int32_t *medoid_pos, const int32_t *mask_frame, const int32_t *frame_lane,
                       const int32_t *class_id, const double *lane_dist, int32_t n_masks, int32_t n_frames, const double *tab_y,
                       const int32_t *, const int32_t *, const int32_t *, const int32_t *, const double *, const int32_t *, int32_t n_tables,
                       const int32_t *needs_road, const int32_t *is_vehicle, int32_t n_classes, double lane_max_dist,
                       double vehicle_lane_max_dist, int32_t *medoid_pos_kept, uint8_t *on_road, cm3d_stream_t)
{
    const bool rest = mask_frame == g_mask_frame && frame_lane == g_frame_lane && class_id == g_class && is_vehicle == g_veh;
    CALLED(CM3D_ERR_LAUNCH, CM3D_OK, "cm3d_stage2_filter in=%s,%s,%s rest=%s n=%d,%d,%d polygons=%s tables=%d needs_road=%s thr=%g,%g out=%s,%s",
           who(centroid_g), who(medoid_pos), who(lane_dist), rest ? "set" : "other", n_masks, n_frames, n_classes, set(tab_y), n_tables,
           set(needs_road), lane_max_dist, vehicle_lane_max_dist, who(medoid_pos_kept), who(on_road));
}
int cm3d_bev_fit(const float *hit_xyz, const int32_t *hit_off, int32_t n_masks, int32_t idx_cap, const double *angle_cs, int32_t K, double d0,
                 int32_t min_points, double min_length, int32_t *fit_k, double *fit_rect, int32_t *fit_status, cm3d_stream_t)
{
    CALLED(CM3D_ERR_ARG, CM3D_OK, "cm3d_bev_fit in=%s,%s n=%d,%d cs=%s K=%d d0=%g min=%d,%g out=%s,%s,%s", who(hit_xyz), who(hit_off), n_masks,
           idx_cap, angle_cs == g_cs ? "set" : "other", K, d0, min_points, min_length, fit_k == g_fit_k ? "set" : "other",
           fit_rect == g_rect ? "set" : "other", fit_status == g_fit_status ? "set" : "other");
}
int cm3d_yaw_select(const double *fit_rect, const int32_t *fit_status, const int32_t *medoid_pos, const int32_t *mask_frame,
                    const int32_t *class_id, const int32_t *is_vehicle, int32_t n_classes, const double *lane_dist, double lane_min_dist,
                    const float *lane, const int32_t *lane_off, const int32_t *frame_lane, const int32_t *lane_idx, int32_t n_tables,
                    int32_t n_lane_points, const float *pose_rt, int32_t n_masks, int32_t n_frames, float *yaw_tab, int32_t *yaw_idx,
                    int32_t *yaw_src, cm3d_stream_t)
{
    const bool rest = fit_rect == g_rect && fit_status == g_fit_status && mask_frame == g_mask_frame && class_id == g_class && is_vehicle == g_veh;
    CALLED(CM3D_ERR_WORKSPACE, CM3D_OK, "cm3d_yaw_select pos=%s rest=%s classes=%d dist=%s,%g lane=%s,%s,%s,%s n=%d,%d pose=%s n=%d,%d out=%s,%s,%s",
           who(medoid_pos), rest ? "set" : "other", n_classes, who(lane_dist), lane_min_dist, who(lane), who(lane_off), who(frame_lane),
           who(lane_idx), n_tables, n_lane_points, who(pose_rt), n_masks, n_frames, who(yaw_tab), who(yaw_idx), yaw_src == g_yaw_src ? "set" : "other");
}
int cm3d_box_nms_bounded(const float *centroid, const int32_t *medoid_pos, const int32_t *mask_off, int32_t n_frames, int32_t n_masks,
                         const int32_t *class_id, const double *score, const float *lane, const int32_t *lane_off, const int32_t *frame_lane,
                         const int32_t *lane_idx, const double *lane_dist, const double *prior_wlh, const int32_t *is_vehicle,
                         const int32_t *nms_group, const double *nms_thr, int32_t n_classes, const double *ego_xyz, const float *pose_inv,
                         int32_t max_masks_per_frame, double *box, int32_t *flags, cm3d_stream_t)
{
    const bool rest = centroid == g_centroid && mask_off == g_mask_off && class_id == g_class && score == g_score && prior_wlh == g_prior &&
                      is_vehicle == g_veh && nms_group == g_group && nms_thr == g_thr && ego_xyz == g_ego;
    CALLED(CM3D_ERR_LAUNCH, CM3D_OK, "cm3d_box_nms_bounded pos=%s lane=%s,%s,%s,%s dist=%s rest=%s n=%d,%d,%d pose_inv=%s bound=%d out=%s,%s",
           who(medoid_pos), who(lane), who(lane_off), who(frame_lane), who(lane_idx), who(lane_dist), rest ? "set" : "other", n_frames, n_masks,
           n_classes, who(pose_inv), max_masks_per_frame, who(box), who(flags));
}
int cm3d_box_rotated_nms(double *box, int32_t *flags, const int32_t *mask_off, int32_t n_frames, int32_t n_masks, const int32_t *class_id,
                         const double *prior_wlh, const int32_t *nms_group, int32_t n_classes, const double *thr, int32_t n_groups,
                         int32_t measure, int32_t class_agnostic, int32_t waymo, int32_t max_masks_per_frame, cm3d_stream_t)
{
    const bool rest = class_id == g_class && prior_wlh == g_prior && nms_group == g_group;
    CALLED(CM3D_ERR_WORKSPACE, CM3D_OK, "cm3d_box_rotated_nms io=%s,%s off=%s rest=%s n=%d,%d,%d thr=%s,%d measure=%d agnostic=%d waymo=%d bound=%d",
           who(box), who(flags), who(mask_off), rest ? "set" : "other", n_frames, n_masks, n_classes, who(thr), n_groups, measure, class_agnostic,
           waymo, max_masks_per_frame);
}
}

// the descriptors of a case: copied in, so that a case can be checked for having been left alone
struct Case {
    cm3d_lift_pass_desc p;
    cm3d_depth_cluster_desc c;
    cm3d_stage2_filter_desc f;
    cm3d_yaw_fit_desc y;
    cm3d_rotated_nms_desc n;
    cm3d_lift_pass_options o;
};

static void run_case(const char *name, const Case &k, const std::function<int(const Case &)> &fn)
{
    std::printf("case %s\n", name);
    g_trace = true, g_calls = 0, g_fail_at = -1;
    Case before;
    std::memcpy(&before, &k, sizeof k);
    const int rc = fn(k);
    const int n = g_calls;
    std::printf("rc %d\n", rc);
    if (std::memcmp(&before, &k, sizeof k) != 0) std::printf("a caller's descriptor was changed\n");
    g_trace = false;
    for (int i = 0; i < n; ++i) {
        g_calls = 0, g_fail_at = i;
        const int ri = fn(k);
        std::printf("fail %d %d %d\n", i, ri, g_calls);
    }
}

// cm3d_lift_pass_opt with the members `which` names (c, f, y, n) pointing at the case's descriptors
static void run_opt(const char *name, Case k, const char *which)
{
    k.o.cluster = std::strchr(which, 'c') ? &k.c : nullptr, k.o.filter = std::strchr(which, 'f') ? &k.f : nullptr;
    k.o.yaw = std::strchr(which, 'y') ? &k.y : nullptr, k.o.nms = std::strchr(which, 'n') ? &k.n : nullptr;
    // (k is this function's copy: the pointers must be taken from the object the pass will see)
    run_case(name, k, [](const Case &q) { return cm3d_lift_pass_opt(&q.p, &q.o, nullptr); });
}
static void run_clustered(const char *name, const Case &k) { run_case(name, k, [](const Case &q) { return cm3d_lift_pass_clustered(&q.p, &q.c, nullptr); }); }
static void run_filtered(const char *name, const Case &k) { run_case(name, k, [](const Case &q) { return cm3d_lift_pass_filtered(&q.p, &q.f, nullptr); }); }
static void run_yaw_fitted(const char *name, const Case &k) { run_case(name, k, [](const Case &q) { return cm3d_lift_pass_yaw_fitted(&q.p, &q.y, nullptr); }); }
static void run_yaw_boxes(const char *name, const Case &k) { run_case(name, k, [](const Case &q) { return cm3d_yaw_fit_boxes(&q.p, &q.y, nullptr); }); }

static Case with_events(Case k)
{
    k.c.ev[0] = (void *)0x50, k.c.ev[1] = (void *)0x51, k.f.ev[0] = (void *)0x40, k.f.ev[1] = (void *)0x41;
    k.y.ev[0] = (void *)0x60, k.y.ev[1] = (void *)0x61;
    return k;
}

int main()
{
    Case q;
    std::memset(&q, 0, sizeof q);
    cm3d_lift_pass_desc &p = q.p;
    p.size = (int64_t)sizeof p;
    p.hit_off = g_hit_off, p.tile_off = g_tile_off, p.hit_idx = g_hit_idx, p.hit_xyz = g_hit_xyz, p.tile_work = g_tile_work;
    p.medoid_pos = g_medoid_pos, p.centroid_g = g_centroid, p.mask_frame = g_mask_frame;
    p.lane = g_lane, p.lane_off = g_lane_off, p.frame_lane = g_frame_lane, p.lane_idx = g_lane_idx, p.lane_dist = g_lane_dist;
    p.class_id = g_class, p.score = g_score, p.prior_wlh = g_prior, p.is_vehicle = g_veh, p.nms_group = g_group, p.nms_thr = g_thr;
    p.ego_xyz = g_ego, p.box = g_box, p.flags = g_flags, p.mask_off = g_mask_off;
    p.n_masks = 7, p.n_frames = 3, p.idx_cap = 4096, p.n_tables = 2, p.n_lane_points = 900, p.n_classes = 10, p.planes = 3;
    q.c.size = (int64_t)sizeof q.c;
    q.c.origin = g_origin, q.c.cl_off = g_cl_off, q.c.cl_tile_off = g_cl_tile_off, q.c.cl_idx = g_cl_idx, q.c.cl_xyz = g_cl_xyz;
    q.c.cl_status = g_cl_status, q.c.ws = g_ws, q.c.ws_bytes = 16, q.c.eps = 1.0, q.c.min_points = 20, q.c.pick = 0;
    q.f.size = (int64_t)sizeof q.f;
    q.f.medoid_pos_kept = g_kept, q.f.on_road = g_on_road, q.f.lane_max_dist = 20.0, q.f.vehicle_lane_max_dist = 4.0;
    q.y.size = (int64_t)sizeof q.y;
    q.y.angle_cs = g_cs, q.y.fit_k = g_fit_k, q.y.fit_rect = g_rect, q.y.fit_status = g_fit_status, q.y.yaw_tab = g_yaw_tab, q.y.yaw_idx = g_yaw_idx;
    q.y.yaw_src = g_yaw_src, q.y.tab_off = g_tab_off, q.y.tab_frame = g_tab_frame;
    q.y.K = 128, q.y.min_points = 20, q.y.d0 = 0.05, q.y.min_length = 1.0, q.y.lane_min_dist = 0.0;
    q.n.size = (int64_t)sizeof q.n;
    q.n.thr = g_rot_thr, q.n.n_thr = 10, q.n.measure = 1, q.n.class_agnostic = 1;
    q.o.size = (int64_t)sizeof q.o;
    Case k;

    // ---- the filtered pass
    k = q, k.p.planes = 1;
    run_filtered("filter.lanes_only", k);
    k.f.tab_y = g_poly_d, k.f.tab_slab = g_poly_i, k.f.slab_off = g_poly_i, k.f.ent_edge = g_poly_i, k.f.ent_ring = g_poly_i, k.f.edge = g_poly_d;
    k.f.ring_info = g_poly_i, k.f.needs_road = g_poly_i, k.f.n_poly_tables = 2;
    run_filtered("filter.polygons", k);
    k = q, k.p.planes = 1, k.f.ev[0] = (void *)0x40, k.f.ev[1] = (void *)0x41;
    run_filtered("filter.events", k);
    k = q, k.p.pose_inv = g_pose_inv;
    run_filtered("filter.pose_planes", k);
    k.p.planes = 32;
    run_filtered("filter.planes_32", k);
    k = q, k.f.size -= 8;
    run_filtered("filter.wrong_size", k);
    k = q, k.f.medoid_pos_kept = nullptr;
    run_filtered("filter.no_output", k);
    k = q, k.f.on_road = nullptr;
    run_filtered("filter.no_on_road", k);
    run_case("filter.null_pass", q, [](const Case &c) { return cm3d_lift_pass_filtered(nullptr, &c.f, nullptr); });
    run_case("filter.null_filter", q, [](const Case &c) { return cm3d_lift_pass_filtered(&c.p, nullptr, nullptr); });

    // ---- the clustered pass
    run_clustered("cluster.plain", q);
    k = q, k.c.ev[0] = (void *)0x50, k.c.ev[1] = (void *)0x51, k.c.eps = 0.5, k.c.min_points = 3, k.c.pick = 1;
    run_clustered("cluster.events", k);
    k = q, k.c.size -= 8;
    run_clustered("cluster.wrong_size", k);
    const char *couts[] = {"cluster.no_cl_off", "cluster.no_cl_tile_off", "cluster.no_cl_idx", "cluster.no_cl_xyz", "cluster.no_cl_status"};
    for (int i = 0; i < 5; ++i) {
        k = q;
        if (i == 0) k.c.cl_off = nullptr;
        if (i == 1) k.c.cl_tile_off = nullptr;
        if (i == 2) k.c.cl_idx = nullptr;
        if (i == 3) k.c.cl_xyz = nullptr;
        if (i == 4) k.c.cl_status = nullptr;
        run_clustered(couts[i], k);
    }
    run_case("cluster.null_pass", q, [](const Case &c) { return cm3d_lift_pass_clustered(nullptr, &c.c, nullptr); });
    run_case("cluster.null_cluster", q, [](const Case &c) { return cm3d_lift_pass_clustered(&c.p, nullptr, nullptr); });

    // ---- the yaw-fitted pass and the fit's launches alone
    run_yaw_fitted("yaw.plain", q);
    run_yaw_boxes("yaw.boxes_alone", q);
    Case w = q;
    w.y.ev[0] = (void *)0x50, w.y.ev[1] = (void *)0x51, w.y.K = 64, w.y.min_points = 5, w.y.d0 = 0.1, w.y.min_length = 2.5, w.y.lane_min_dist = 1.5;
    w.p.pose_rt = g_pose_rt, w.p.pose_inv = g_pose_inv, w.p.planes = 40;
    run_yaw_fitted("yaw.waymo_events", w);
    w.y.hit_xyz = g_cl_xyz, w.y.hit_off = g_cl_off, w.y.medoid_pos = g_kept;
    run_yaw_boxes("yaw.waymo_events_own_lists", w);
    run_yaw_fitted("yaw.own_lists_in_a_pass", w);              // the yaw rule: a pass fits the lists it derives and no others
    k = q, k.y.size -= 8;
    run_yaw_fitted("yaw.wrong_size", k);
    run_yaw_boxes("yaw.wrong_size_boxes", k);
    k = q, k.p.size += 8;
    run_yaw_fitted("yaw.wrong_pass_size", k);
    run_yaw_boxes("yaw.wrong_pass_size_boxes", k);
    const char *youts[] = {"yaw.no_angle_cs", "yaw.no_fit_k", "yaw.no_fit_rect", "yaw.no_fit_status", "yaw.no_yaw_tab", "yaw.no_yaw_idx",
                           "yaw.no_yaw_src", "yaw.no_tab_off", "yaw.no_tab_frame"};
    for (int i = 0; i < 9; ++i) {
        k = q;
        if (i == 0) k.y.angle_cs = nullptr;
        if (i == 1) k.y.fit_k = nullptr;
        if (i == 2) k.y.fit_rect = nullptr;
        if (i == 3) k.y.fit_status = nullptr;
        if (i == 4) k.y.yaw_tab = nullptr;
        if (i == 5) k.y.yaw_idx = nullptr;
        if (i == 6) k.y.yaw_src = nullptr;
        if (i == 7) k.y.tab_off = nullptr;
        if (i == 8) k.y.tab_frame = nullptr;
        if (i & 1)
            run_yaw_boxes(youts[i], k);
        else
            run_yaw_fitted(youts[i], k);
    }
    run_case("yaw.null_pass", q, [](const Case &c) { return cm3d_lift_pass_yaw_fitted(nullptr, &c.y, nullptr); });
    run_case("yaw.null_fit", q, [](const Case &c) { return cm3d_yaw_fit_boxes(&c.p, nullptr, nullptr); });
    run_case("yaw.null_fit_pass", q, [](const Case &c) { return cm3d_lift_pass_yaw_fitted(&c.p, nullptr, nullptr); });

    // ---- the composed pass: every presence combination, every event set; nuScenes and Waymo descriptors
    const Case e = with_events(q);
    Case ew = e;
    ew.p.pose_rt = g_pose_rt, ew.p.pose_inv = g_pose_inv, ew.p.planes = 40;
    for (int m = 0; m < 16; ++m) {
        char which[5] = "----", name[32];
        if (m & 1) which[0] = 'c';
        if (m & 2) which[1] = 'f';
        if (m & 4) which[2] = 'y';
        if (m & 8) which[3] = 'n';
        std::snprintf(name, sizeof name, "combo.%s", which);
        run_opt(name, e, which);
        std::snprintf(name, sizeof name, "combo_waymo.%s", which);
        run_opt(name, ew, which);
    }
    run_case("opt.null", e, [](const Case &c) { return cm3d_lift_pass_opt(&c.p, nullptr, nullptr); });
    // the single-option passes with their events set: the trace of the composed call with that member alone
    run_clustered("legacy.c---", e);
    run_filtered("legacy.-f--", e);
    run_yaw_fitted("legacy.--y-", e);

    // ---- a bad descriptor makes no call, wherever it stands and whatever stands beside it
    k = e, k.o.size += 8;
    run_opt("bad.opt_size", k, "cfyn");
    run_opt("bad.opt_size_no_member", k, "----");
    k = e, k.p.size -= 8;
    run_opt("bad.pass_size", k, "cfyn");
    run_case("bad.null_pass", e, [](const Case &c) {
        const cm3d_lift_pass_options o = {(int64_t)sizeof o, &c.c, &c.f, &c.y, &c.n};
        return cm3d_lift_pass_opt(nullptr, &o, nullptr);
    });
    k = e, k.c.size -= 8;
    run_opt("bad.cluster_size", k, "cfyn");
    k = e, k.f.size -= 8;
    run_opt("bad.filter_size", k, "cfyn");
    k = e, k.y.size -= 8;
    run_opt("bad.yaw_size", k, "cfyn");
    k = e, k.n.size -= 8;
    run_opt("bad.nms_size", k, "cfyn");
    run_opt("bad.nms_size_behind_cluster", k, "c--n");
    run_opt("bad.nms_size_alone", k, "---n");
    k = e, k.n.thr = nullptr;
    run_opt("bad.nms_no_thr", k, "cfyn");
    k = e, k.y.tab_off = nullptr;
    run_opt("bad.yaw_no_tab_off_behind_filter", k, "-fy-");
    k = e, k.f.on_road = nullptr;
    run_opt("bad.filter_no_on_road_behind_cluster", k, "cf--");
    k = e, k.c.cl_idx = nullptr;
    run_opt("bad.cluster_no_cl_idx", k, "c-yn");
    k.p.hit_idx = nullptr;                                   // a pass without index lists clusters without them
    run_opt("ok.cluster_without_idx", k, "c---");

    // ---- the yaw rule: inside a pass the fit's lists and positions are NULL or what the composition derives
    k = e, k.y.hit_xyz = g_hit_xyz;
    run_opt("rule.raw_xyz_behind_cluster", k, "c-y-");
    k = e, k.y.hit_off = g_hit_off;
    run_opt("rule.raw_off_behind_cluster", k, "c-y-");
    k = e, k.y.medoid_pos = g_medoid_pos;
    run_opt("rule.raw_pos_behind_filter", k, "-fy-");
    k = e, k.y.hit_xyz = g_cl_xyz, k.y.hit_off = g_cl_off;
    run_opt("rule.cl_lists_without_cluster", k, "-fy-");
    k.y.medoid_pos = g_kept;
    run_opt("rule.equal_cfyn", k, "cfyn");
    k = e, k.y.hit_xyz = g_hit_xyz, k.y.hit_off = g_hit_off, k.y.medoid_pos = g_medoid_pos;
    run_opt("rule.equal_--yn", k, "--yn");
    std::printf("pass_options_sim done\n");
    return 0;
}
