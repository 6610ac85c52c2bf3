// Stand-alone trace of cm3d_lift_pass_stripped, cm3d_lift_pass_owned and cm3d_lift_pass_composed (cm3d_amd/csrc/pass_compose.cpp over the
// seam of csrc/pass_options.cpp) over stubs of the entry points they call and of hipEventRecord, in the manner of
// tests/pass_options_sim.cpp (whose stubs do not know the gs_* and ow_* arrays, so this program has its own: each says whose arrays it
// was handed).  tests/test_ground_strip_host.py builds it with the address and undefined-behaviour sanitizers and compares the output
// with the sequence include/cm3d_hip.h states; tests/test_owned_pass_host.py does so for the owned.* cases, and holds the composer's
// trace against that of the entry point with the same arguments (the equiv.* cases).  Per case: the calls of a clean pass, `rc`, then
// for every call k of that pass `fail k rc calls`: the pass again with call k answering an error.
#include <hip/hip_runtime_api.h>

#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstring>

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

static int32_t g_hit_off[4], g_tile_off[4], g_hit_idx[4], g_tile_work[4], g_cl_off[4], g_cl_tile_off[4], g_cl_idx[4], g_cl_status[4], g_gs_off[4],
    g_gs_tile_off[4], g_gs_idx[4], g_gs_status[4], g_gs_dropped[4], g_grid_n[4], g_medoid_pos[4], g_kept[4], g_lane_off[4], g_frame_lane[4],
    g_lane_idx[4], g_mask_frame[4], g_class[4], g_veh[4], g_fit_k[4], g_fit_status[4], g_yaw_idx[4], g_yaw_src[4], g_tab_off[2], g_tab_frame[4],
    g_mask_off[4], g_flags[4], g_group[4], g_place_src[4], g_sweep_row_off[4], g_frame_sweep_off[4], g_pt_off[4], g_ow_owner[4], g_ow_off[4],
    g_ow_tile_off[4], g_ow_idx[4], g_ow_status[4], g_ow_lost[4];
static float g_hit_xyz[4], g_cl_xyz[4], g_gs_xyz[4], g_lane[4], g_yaw_tab[4], g_centroid[4], g_pose_rt[12], g_pose_inv[16], g_raw[4], g_xf[24],
    g_points[4], g_ow_xyz[4];
static double g_cs[4], g_rect[8], g_lane_dist[4], g_score[4], g_prior[4], g_thr[4], g_rot_thr[4], g_ego[4], g_box[4], g_origin[4], g_grid_z[4],
    g_pushed[8];
static uint8_t g_ws[16], g_gs_ws[16], g_ow_ws[16], g_on_road[4];

struct Name { const void *p; const char *n; };
static const char *who(const void *p)
{
    const Name names[] = {{g_hit_off, "hit_off"}, {g_tile_off, "tile_off"}, {g_hit_idx, "hit_idx"}, {g_tile_work, "tile_work"}, {g_cl_off, "cl_off"},
                          {g_cl_tile_off, "cl_tile_off"}, {g_cl_idx, "cl_idx"}, {g_gs_off, "gs_off"}, {g_gs_tile_off, "gs_tile_off"},
                          {g_gs_idx, "gs_idx"}, {g_gs_xyz, "gs_xyz"}, {g_gs_status, "gs_status"}, {g_gs_dropped, "gs_dropped"}, {g_grid_z, "grid_z"},
                          {g_grid_n, "grid_n"}, {g_medoid_pos, "medoid_pos"}, {g_kept, "kept"}, {g_hit_xyz, "hit_xyz"}, {g_cl_xyz, "cl_xyz"},
                          {g_lane, "lane"}, {g_yaw_tab, "yaw_tab"}, {g_box, "box"}, {g_flags, "flags"}, {g_origin, "origin"}, {g_ego, "ego"},
                          {g_raw, "raw"}, {g_points, "points"}, {g_pt_off, "pt_off"}, {g_ws, "cl_ws"}, {g_gs_ws, "gs_ws"}, {g_rect, "fit_rect"},
                          {g_yaw_src, "yaw_src"}, {g_place_src, "place_src"}, {g_pushed, "place_pushed"}, {g_cl_status, "cl_status"}, {g_ow_owner, "ow_owner"},
                          {g_ow_off, "ow_off"}, {g_ow_tile_off, "ow_tile_off"}, {g_ow_idx, "ow_idx"}, {g_ow_xyz, "ow_xyz"}, {g_ow_status, "ow_status"},
                          {g_ow_lost, "ow_lost"}, {g_ow_ws, "ow_ws"}, {g_mask_off, "mask_off"}, {g_score, "score"}};
    if (!p) return "null";
    for (const Name &e : names)
        if (e.p == p) return e.n;
    return "other";
}

extern "C" {
hipError_t hipEventRecord(hipEvent_t ev, hipStream_t) { CALLED(hipErrorInvalidValue, hipSuccess, "record %#x", (unsigned)(uintptr_t)ev); }

static int part(const char *name, const cm3d_lift_pass_desc *d)
{
    CALLED(CM3D_ERR_LAUNCH, CM3D_OK, "%s hit_off=%s tile_off=%s hit_idx=%s hit_xyz=%s tile_work=%s", name, who(d->hit_off), who(d->tile_off),
           who(d->hit_idx), who(d->hit_xyz), who(d->tile_work));
}
int cm3d_lift_pass(const cm3d_lift_pass_desc *d, cm3d_stream_t) { return part("cm3d_lift_pass", d); }
int cm3d_lift_pass_head(const cm3d_lift_pass_desc *d, cm3d_stream_t) { return part("cm3d_lift_pass_head", d); }
int cm3d_lift_pass_tail(const cm3d_lift_pass_desc *d, cm3d_stream_t) { return part("cm3d_lift_pass_tail", d); }
// the rule of include/cm3d_hip.h, written out once more: the real one lives beside the kernels
int cm3d_ground_strip_check(double cell, double down, double up, double quantile, int32_t min_points, double margin, int32_t min_keep)
{
    const bool ok = std::isfinite(cell) && cell > 0.0 && std::isfinite(down) && down > 0.0 && std::isfinite(up) && up > 0.0 && quantile >= 0.0 &&
                    quantile <= 1.0 && min_points >= 1 && std::isfinite(margin) && min_keep >= 1;
    return ok ? CM3D_OK : CM3D_ERR_ARG;
}
int cm3d_ground_grid(const float *points, const int32_t *pt_off, const float *raw, int32_t raw_stride, const float *sweep_xf,
                     const int32_t *sweep_row_off, const int32_t *frame_sweep_off, int32_t n_sweeps, float halfw, int32_t n_rows,
                     const double *origin, int32_t n_frames, double cell, double down, double up, double quantile, int32_t min_points,
                     double *grid_z, int32_t *grid_n, cm3d_stream_t)
{
    const bool rest = sweep_xf == g_xf && sweep_row_off == g_sweep_row_off && frame_sweep_off == g_frame_sweep_off;
    CALLED(CM3D_ERR_WORKSPACE, CM3D_OK, "cm3d_ground_grid cloud=%s,%s raw=%s,%d rest=%s n=%d,%d,%d halfw=%g origin=%s par=%g,%g,%g,%g,%d out=%s,%s",
           who(points), who(pt_off), who(raw), raw_stride, rest ? "set" : "other", n_sweeps, n_rows, n_frames, (double)halfw, who(origin), cell, down,
           up, quantile, min_points, who(grid_z), who(grid_n));
}
int cm3d_ground_strip(const float *hit_xyz, const int32_t *hit_idx, const int32_t *hit_off, const int32_t *mask_frame, int32_t n_masks,
                      int32_t idx_cap, const double *origin, const double *grid_z, int32_t n_frames, double cell, double margin, int32_t min_keep,
                      int32_t *gs_off, int32_t *gs_tile_off, int32_t *gs_idx, float *gs_xyz, int32_t *gs_status, int32_t *gs_dropped, void *ws,
                      int64_t ws_bytes, cm3d_stream_t)
{
    CALLED(CM3D_ERR_WORKSPACE, CM3D_OK, "cm3d_ground_strip in=%s,%s,%s frame=%s n=%d,%d,%d origin=%s grid=%s par=%g,%g,%d out=%s,%s,%s,%s,%s,%s ws=%s,%lld",
           who(hit_xyz), who(hit_idx), who(hit_off), mask_frame == g_mask_frame ? "set" : "other", n_masks, idx_cap, n_frames, who(origin),
           who(grid_z), cell, margin, min_keep, who(gs_off), who(gs_tile_off), who(gs_idx), who(gs_xyz), who(gs_status), who(gs_dropped), who(ws),
           (long long)ws_bytes);
}
// the rule of include/cm3d_hip.h, written out once more
int cm3d_point_owner_check(int32_t rule, int32_t min_keep) { return (rule == 0 || rule == 1) && min_keep >= 1 ? CM3D_OK : CM3D_ERR_ARG; }
int cm3d_point_owner(const float *hit_xyz, const int32_t *hit_idx, const int32_t *hit_off, const int32_t *mask_off, int32_t n_frames, int32_t n_masks,
                     int32_t idx_cap, int32_t max_pts_per_frame, const double *score, int32_t rule, int32_t min_keep, int32_t *ow_owner,
                     int32_t *ow_off, int32_t *ow_tile_off, int32_t *ow_idx, float *ow_xyz, int32_t *ow_status, int32_t *ow_lost, void *ws,
                     int64_t ws_bytes, cm3d_stream_t)
{
    CALLED(CM3D_ERR_WORKSPACE, CM3D_OK, "cm3d_point_owner in=%s,%s,%s off=%s score=%s n=%d,%d,%d,%d par=%d,%d out=%s,%s,%s,%s,%s,%s,%s ws=%s,%lld",
           who(hit_xyz), who(hit_idx), who(hit_off), who(mask_off), who(score), n_frames, n_masks, idx_cap, max_pts_per_frame, rule, min_keep,
           who(ow_owner), who(ow_off), who(ow_tile_off), who(ow_idx), who(ow_xyz), who(ow_status), who(ow_lost), who(ws), (long long)ws_bytes);
}
int cm3d_depth_cluster(const float *hit_xyz, const int32_t *hit_idx, const int32_t *hit_off, const int32_t *, int32_t, int32_t, const double *origin,
                       int32_t, double, int32_t, int32_t, int32_t *cl_off, int32_t *cl_tile_off, int32_t *cl_idx, float *cl_xyz, int32_t *cl_status,
                       void *ws, int64_t, cm3d_stream_t)
{
    CALLED(CM3D_ERR_WORKSPACE, CM3D_OK, "cm3d_depth_cluster in=%s,%s,%s origin=%s out=%s,%s,%s,%s,%s ws=%s", who(hit_xyz), who(hit_idx), who(hit_off),
           who(origin), who(cl_off), who(cl_tile_off), who(cl_idx), who(cl_xyz), who(cl_status), who(ws));
}
int cm3d_stage2_filter(const float *, const int32_t *medoid_pos, const int32_t *, const int32_t *, const int32_t *, const double *, int32_t, int32_t,
                       const double *, const int32_t *, const int32_t *, const int32_t *, const int32_t *, const double *, const int32_t *, int32_t,
                       const int32_t *, const int32_t *, int32_t, double, double, int32_t *medoid_pos_kept, uint8_t *, cm3d_stream_t)
{
    CALLED(CM3D_ERR_LAUNCH, CM3D_OK, "cm3d_stage2_filter pos=%s out=%s", who(medoid_pos), who(medoid_pos_kept));
}
int cm3d_bev_fit(const float *hit_xyz, const int32_t *hit_off, int32_t, int32_t, const double *, int32_t, double, int32_t, double, int32_t *,
                 double *fit_rect, int32_t *, cm3d_stream_t)
{
    CALLED(CM3D_ERR_ARG, CM3D_OK, "cm3d_bev_fit in=%s,%s out=%s", who(hit_xyz), who(hit_off), who(fit_rect));
}
int cm3d_yaw_select(const double *, const int32_t *, const int32_t *medoid_pos, const int32_t *, const int32_t *, const int32_t *, int32_t,
                    const double *, double, const float *, const int32_t *, const int32_t *, const int32_t *, int32_t, int32_t, const float *, int32_t,
                    int32_t, float *yaw_tab, int32_t *, int32_t *, cm3d_stream_t)
{
    CALLED(CM3D_ERR_WORKSPACE, CM3D_OK, "cm3d_yaw_select pos=%s out=%s", who(medoid_pos), who(yaw_tab));
}
int cm3d_box_nms_bounded(const float *, const int32_t *medoid_pos, const int32_t *, int32_t, int32_t, const int32_t *, const double *,
                         const float *lane, const int32_t *, const int32_t *, const int32_t *, const double *, const double *, const int32_t *,
                         const int32_t *, const double *, int32_t, const double *, const float *, int32_t, double *box, int32_t *flags, cm3d_stream_t)
{
    CALLED(CM3D_ERR_LAUNCH, CM3D_OK, "cm3d_box_nms_bounded pos=%s lane=%s out=%s,%s", who(medoid_pos), who(lane), who(box), who(flags));
}
int cm3d_box_place(double *box, int32_t *flags, const int32_t *, int32_t, int32_t, const double *fit_rect, const int32_t *yaw_src, const double *,
                   const int32_t *, const double *, int32_t, const double *, int32_t waymo, double thin, int32_t, int32_t *place_src,
                   double *place_pushed, cm3d_stream_t)
{
    CALLED(CM3D_ERR_WORKSPACE, CM3D_OK, "cm3d_box_place io=%s,%s in=%s,%s waymo=%d thin=%g out=%s,%s", who(box), who(flags), who(fit_rect), who(yaw_src),
           waymo, thin, who(place_src), who(place_pushed));
}
int cm3d_box_rotated_nms(double *box, int32_t *flags, const int32_t *, int32_t, int32_t, const int32_t *, const double *, const int32_t *, int32_t,
                         const double *, int32_t, int32_t, int32_t, int32_t waymo, int32_t, cm3d_stream_t)
{
    CALLED(CM3D_ERR_WORKSPACE, CM3D_OK, "cm3d_box_rotated_nms io=%s,%s waymo=%d", who(box), who(flags), waymo);
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
    cm3d_box_place_desc b;
    cm3d_ground_strip_desc s;
    cm3d_point_owner_desc w;
};

// the entry point under trace: cm3d_lift_pass_stripped ('s'), cm3d_lift_pass_owned ('w'), cm3d_lift_pass_placed ('p'),
// cm3d_lift_pass_opt ('o') or cm3d_lift_pass_composed ('x')
static char g_entry = 's';

// the entry point with the members `which` names (c, f, y, n: the options' members; p: the placement; o: the options themselves
// -- without it opt is NULL; s: the strip; w: the ownership) pointing at the case's descriptors
static int call(Case &k, const char *which)
{
    k.o.cluster = std::strchr(which, 'c') ? &k.c : nullptr, k.o.filter = std::strchr(which, 'f') ? &k.f : nullptr;
    k.o.yaw = std::strchr(which, 'y') ? &k.y : nullptr, k.o.nms = std::strchr(which, 'n') ? &k.n : nullptr;
    const cm3d_lift_pass_options *o = std::strchr(which, 'o') ? &k.o : nullptr;
    const cm3d_box_place_desc *b = std::strchr(which, 'p') ? &k.b : nullptr;
    const cm3d_ground_strip_desc *s = std::strchr(which, 's') ? &k.s : nullptr;
    const cm3d_point_owner_desc *w = std::strchr(which, 'w') ? &k.w : nullptr;
    if (g_entry == 'x') return cm3d_lift_pass_composed(&k.p, o, b, s, w, nullptr);
    if (g_entry == 'w') return cm3d_lift_pass_owned(&k.p, o, b, s, w, nullptr);
    if (g_entry == 'p') return cm3d_lift_pass_placed(&k.p, o, b, nullptr);
    if (g_entry == 'o') return cm3d_lift_pass_opt(&k.p, o, nullptr);
    return cm3d_lift_pass_stripped(&k.p, o, b, s, nullptr);
}

static void run(const char *name, Case k, const char *which)
{
    std::printf("case %s\n", name);
    g_trace = true, g_calls = 0, g_fail_at = -1;
    const int rc = call(k, which);
    Case before;
    std::memcpy(&before, &k, sizeof k);
    const int n = g_calls;
    std::printf("rc %d\n", rc);
    g_trace = false;
    for (int i = 0; i < n; ++i) {
        g_calls = 0, g_fail_at = i;
        const int ri = call(k, which);
        std::printf("fail %d %d %d\n", i, ri, g_calls);
    }
    if (std::memcmp(&before, &k, sizeof k) != 0) std::printf("a caller's descriptor was changed\n");
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
    p.raw = g_raw, p.raw_stride = 5, p.sweep_xf = g_xf, p.sweep_row_off = g_sweep_row_off, p.frame_sweep_off = g_frame_sweep_off, p.pt_off = g_pt_off;
    p.n_sweeps = 6, p.pt_cap = 5000, p.halfw = 1.5f, p.max_pts_per_frame = 3000;
    p.n_masks = 7, p.n_frames = 3, p.idx_cap = 4096, p.n_tables = 2, p.n_lane_points = 900, p.n_classes = 10, p.planes = 3;
    q.c.size = (int64_t)sizeof q.c;
    q.c.origin = g_origin, q.c.cl_off = g_cl_off, q.c.cl_tile_off = g_cl_tile_off, q.c.cl_idx = g_cl_idx, q.c.cl_xyz = g_cl_xyz;
    q.c.cl_status = g_cl_status, q.c.ws = g_ws, q.c.ws_bytes = 16, q.c.eps = 1.0, q.c.min_points = 20, q.c.pick = 0;
    q.c.ev[0] = (void *)0x50, q.c.ev[1] = (void *)0x51;
    q.f.size = (int64_t)sizeof q.f;
    q.f.medoid_pos_kept = g_kept, q.f.on_road = g_on_road, q.f.lane_max_dist = 20.0, q.f.vehicle_lane_max_dist = 4.0;
    q.f.ev[0] = (void *)0x40, q.f.ev[1] = (void *)0x41;
    q.y.size = (int64_t)sizeof q.y;
    q.y.angle_cs = g_cs, q.y.fit_k = g_fit_k, q.y.fit_rect = g_rect, q.y.fit_status = g_fit_status, q.y.yaw_tab = g_yaw_tab, q.y.yaw_idx = g_yaw_idx;
    q.y.yaw_src = g_yaw_src, q.y.tab_off = g_tab_off, q.y.tab_frame = g_tab_frame;
    q.y.K = 128, q.y.min_points = 20, q.y.d0 = 0.05, q.y.min_length = 1.0, q.y.lane_min_dist = 0.0;
    q.y.ev[0] = (void *)0x60, q.y.ev[1] = (void *)0x61;
    q.n.size = (int64_t)sizeof q.n;
    q.n.thr = g_rot_thr, q.n.n_thr = 10, q.n.measure = 1, q.n.class_agnostic = 1;
    q.o.size = (int64_t)sizeof q.o;
    q.b.size = (int64_t)sizeof q.b;
    q.b.place_src = g_place_src, q.b.place_pushed = g_pushed, q.b.ev[0] = (void *)0x70, q.b.ev[1] = (void *)0x71, q.b.thin = 0.5;
    cm3d_ground_strip_desc &s = q.s;
    s.size = (int64_t)sizeof s;
    s.origin = g_ego, s.grid_z = g_grid_z, s.grid_n = g_grid_n, s.gs_off = g_gs_off, s.gs_tile_off = g_gs_tile_off, s.gs_idx = g_gs_idx;
    s.gs_xyz = g_gs_xyz, s.gs_status = g_gs_status, s.gs_dropped = g_gs_dropped, s.ws = g_gs_ws, s.ws_bytes = 16;
    s.ev[0] = (void *)0x30, s.ev[1] = (void *)0x31;
    s.cell = 2.0, s.down = 4.0, s.up = 3.0, s.quantile = 0.1, s.margin = 0.3, s.min_points = 8, s.min_keep = 5;
    q.w.size = (int64_t)sizeof q.w;
    q.w.ow_owner = g_ow_owner, q.w.ow_off = g_ow_off, q.w.ow_tile_off = g_ow_tile_off, q.w.ow_idx = g_ow_idx, q.w.ow_xyz = g_ow_xyz;
    q.w.ow_status = g_ow_status, q.w.ow_lost = g_ow_lost, q.w.ws = g_ow_ws, q.w.ws_bytes = 16, q.w.rule = 1, q.w.min_keep = 5;
    q.w.ev[0] = (void *)0x20, q.w.ev[1] = (void *)0x21;
    Case w = q;
    w.p.pose_rt = g_pose_rt, w.p.pose_inv = g_pose_inv, w.p.planes = 40;

    // ---- every presence combination of cluster, filter, yaw, placement (with yaw only) and nms
    for (int m = 0; m < 32; ++m) {
        if ((m & 8) && !(m & 4)) continue;
        char which[8] = "os-----", name[40];
        if (m & 1) which[2] = 'c';
        if (m & 2) which[3] = 'f';
        if (m & 4) which[4] = 'y';
        if (m & 8) which[5] = 'p';
        if (m & 16) which[6] = 'n';
        std::snprintf(name, sizeof name, "combo.%s", which + 2);
        run(name, q, which);
    }
    run("combo_waymo.cfypn", w, "oscfypn");
    run("ok.null_opt", q, "s");
    Case e = q;
    e.p.points = g_points;
    run("ok.cloud", e, "os");
    e = q, e.s.ev[0] = e.s.ev[1] = nullptr;
    run("ok.no_events", e, "osc");
    e = q, e.p.hit_idx = nullptr, e.s.gs_idx = nullptr, e.c.cl_idx = nullptr;
    run("ok.without_idx", e, "osc");
    e = q, e.y.hit_xyz = g_gs_xyz, e.y.hit_off = g_gs_off;
    run("rule.gs_lists", e, "osy");
    e = q, e.y.hit_xyz = g_cl_xyz, e.y.hit_off = g_cl_off, e.y.medoid_pos = g_kept;
    run("rule.cl_lists", e, "oscfy");

    // ---- every refusal makes no call
    run("bad.null_strip", q, "ocfyn");
    run("bad.null_strip_null_opt", q, "");
    e = q, e.s.size -= 8;
    run("bad.strip_size", e, "oscfyn");
    e = q, e.o.size += 8;
    run("bad.opt_size", e, "os");
    e = q, e.p.size -= 8;
    run("bad.pass_size", e, "os");
    e = q, e.c.size -= 8;
    run("bad.cluster_size", e, "osc");
    e = q, e.f.on_road = nullptr;
    run("bad.filter_no_on_road", e, "osf");
    e = q, e.y.tab_off = nullptr;
    run("bad.yaw_no_tab_off", e, "osy");
    e = q, e.n.thr = nullptr;
    run("bad.nms_no_thr", e, "osn");
    run("bad.place_without_yaw", q, "oscfpn");
    run("bad.place_null_opt", q, "sp");
    e = q, e.b.size -= 8;
    run("bad.place_size", e, "osyp");
    e = q, e.b.thin = -1.0;
    run("bad.place_thin", e, "osyp");
    const char *outs[] = {"origin", "grid_z", "grid_n", "gs_off", "gs_tile_off", "gs_idx", "gs_xyz", "gs_status", "gs_dropped", "ws"};
    for (int i = 0; i < 10; ++i) {
        char name[40];
        e = q;
        if (i == 0) e.s.origin = nullptr;
        if (i == 1) e.s.grid_z = nullptr;
        if (i == 2) e.s.grid_n = nullptr;
        if (i == 3) e.s.gs_off = nullptr;
        if (i == 4) e.s.gs_tile_off = nullptr;
        if (i == 5) e.s.gs_idx = nullptr;
        if (i == 6) e.s.gs_xyz = nullptr;
        if (i == 7) e.s.gs_status = nullptr;
        if (i == 8) e.s.gs_dropped = nullptr;
        if (i == 9) e.s.ws = nullptr;
        std::snprintf(name, sizeof name, "bad.strip_no_%s", outs[i]);
        run(name, e, "oscfyn");
    }
    const double nan = std::nan("");
    for (int i = 0; i < 12; ++i) {
        char name[40];
        e = q;
        if (i == 0) e.s.cell = 0.0;
        if (i == 1) e.s.cell = nan;
        if (i == 2) e.s.cell = HUGE_VAL;
        if (i == 3) e.s.down = 0.0;
        if (i == 4) e.s.up = nan;
        if (i == 5) e.s.up = 0.0;
        if (i == 6) e.s.quantile = 1.5;
        if (i == 7) e.s.quantile = nan;
        if (i == 8) e.s.min_points = 0;
        if (i == 9) e.s.margin = nan;
        if (i == 10) e.s.margin = HUGE_VAL;
        if (i == 11) e.s.min_keep = 0;
        std::snprintf(name, sizeof name, "bad.strip_param_%d", i);
        run(name, e, "osc");
    }
    e = q, e.y.hit_xyz = g_hit_xyz;
    run("rule.raw_xyz_behind_strip", e, "osy");
    e = q, e.y.hit_off = g_gs_off;
    run("rule.gs_off_behind_cluster", e, "oscy");
    {
        Case y = q;
        std::printf("case bad.null_pass\nrc %d\n", cm3d_lift_pass_stripped(nullptr, nullptr, nullptr, &y.s, nullptr));
    }

    // ---- cm3d_lift_pass_owned: every presence combination of strip, cluster, filter, yaw, placement (with yaw only) and nms
    g_entry = 'w';
    for (int m = 0; m < 64; ++m) {
        if ((m & 16) && !(m & 8)) continue;
        char which[9] = "ow------", name[40];
        if (m & 1) which[2] = 's';
        if (m & 2) which[3] = 'c';
        if (m & 4) which[4] = 'f';
        if (m & 8) which[5] = 'y';
        if (m & 16) which[6] = 'p';
        if (m & 32) which[7] = 'n';
        std::snprintf(name, sizeof name, "owned.combo.%s", which + 2);
        run(name, q, which);
    }
    run("owned.combo_waymo.scfypn", w, "owscfypn");
    run("owned.ok.null_opt", q, "w");
    e = q, e.p.points = g_points;
    run("owned.ok.cloud", e, "ows");
    e = q, e.w.ev[0] = e.w.ev[1] = e.s.ev[0] = e.s.ev[1] = nullptr;
    run("owned.ok.no_events", e, "owsc");
    e = q, e.y.hit_xyz = g_ow_xyz, e.y.hit_off = g_ow_off;
    run("owned.rule.ow_lists", e, "owy");
    e = q, e.y.hit_xyz = g_gs_xyz, e.y.hit_off = g_gs_off;
    run("owned.rule.gs_lists", e, "owsy");

    // ---- every refusal makes no call
    run("owned.bad.null_owner", q, "oscfypn");
    e = q, e.w.size -= 8;
    run("owned.bad.owner_size", e, "owscfypn");
    const char *ows[] = {"ow_owner", "ow_off", "ow_tile_off", "ow_idx", "ow_xyz", "ow_status", "ow_lost", "ws"};
    for (int i = 0; i < 8; ++i) {
        char name[40];
        e = q;
        if (i == 0) e.w.ow_owner = nullptr;
        if (i == 1) e.w.ow_off = nullptr;
        if (i == 2) e.w.ow_tile_off = nullptr;
        if (i == 3) e.w.ow_idx = nullptr;
        if (i == 4) e.w.ow_xyz = nullptr;
        if (i == 5) e.w.ow_status = nullptr;
        if (i == 6) e.w.ow_lost = nullptr;
        if (i == 7) e.w.ws = nullptr;
        std::snprintf(name, sizeof name, "owned.bad.owner_no_%s", ows[i]);
        run(name, e, "owscfypn");
    }
    e = q, e.w.rule = 2;
    run("owned.bad.rule_2", e, "ow");
    e = q, e.w.min_keep = 0;
    run("owned.bad.min_keep_0", e, "owc");
    e = q, e.p.hit_idx = nullptr;
    run("owned.bad.pass_no_hit_idx", e, "ow");
    e = q, e.s.gs_idx = nullptr;
    run("owned.bad.strip_no_gs_idx", e, "ows");
    e = q, e.s.cell = 0.0;
    run("owned.bad.strip_param", e, "ows");
    run("owned.bad.place_without_yaw", q, "owscfpn");
    e = q, e.y.hit_xyz = g_hit_xyz, e.y.hit_off = g_hit_off;
    run("owned.bad.raw_lists_behind_owner", e, "owy");
    e = q, e.y.hit_xyz = g_ow_xyz, e.y.hit_off = g_ow_off;
    run("owned.bad.ow_lists_behind_strip", e, "owsy");

    // ---- cm3d_lift_pass_composed beside the entry point that takes the same arguments: every presence combination, and a NULL opt
    for (int m = 0; m < 128 + 4; ++m) {                  // (the last four: opt == NULL, with and without an ownership and a strip)
        if ((m & 32) && !(m & 16)) continue;
        char which[9] = "o-------", name[40];
        if (m & 1) which[1] = 'w';
        if (m & 2) which[2] = 's';
        if (m & 4) which[3] = 'c';
        if (m & 8) which[4] = 'f';
        if (m & 16) which[5] = 'y';
        if (m & 32) which[6] = 'p';
        if (m & 64) which[7] = 'n';
        if (m & 128) which[0] = '-';
        const char old_entry = std::strchr(which, 'w') ? 'w' : std::strchr(which, 's') ? 's' : std::strchr(which, 'p') ? 'p' : 'o';
        std::snprintf(name, sizeof name, "equiv.old.%s", which);
        g_entry = old_entry, run(name, q, which);
        std::snprintf(name, sizeof name, "equiv.new.%s", which);
        g_entry = 'x', run(name, q, which);
    }
    std::printf("pass_strip_sim done\n");
    return 0;
}
