// Stand-alone trace of cm3d_lift_pass_placed (cm3d_amd/csrc/pass_compose.cpp) over the real seam of csrc/pass_options.cpp and
// stubs of the entry points the two call: the stubs, the arrays and the case runner of tests/pass_options_sim.cpp, taken in whole, plus
// a stub of cm3d_box_place, and of what the composer calls for a strip or an ownership (never reached here).  tests/test_box_place_host.py builds it with the address and undefined-behaviour sanitizers and compares
// the output with the sequence include/cm3d_hip.h states.  Per case, as there: the calls of a clean pass, `rc`, then `fail k rc calls`.
#include <cmath>

#define main pass_options_sim_main
#include "pass_options_sim.cpp"
#undef main

static int32_t g_place_src[4];
static double g_pushed[8];

extern "C" int cm3d_box_place(double *box, int32_t *flags, const int32_t *mask_off, int32_t n_frames, int32_t n_masks, const double *fit_rect,
                              const int32_t *yaw_src, const double *prior_wlh, const int32_t *nms_group, const double *nms_thr,
                              int32_t n_classes, const double *ego_xyz, int32_t waymo, double thin, int32_t max_masks_per_frame,
                              int32_t *place_src, double *place_pushed, cm3d_stream_t)
{
    const bool rest = fit_rect == g_rect && yaw_src == g_yaw_src && prior_wlh == g_prior && nms_group == g_group && nms_thr == g_thr && ego_xyz == g_ego;
    CALLED(CM3D_ERR_WORKSPACE, CM3D_OK, "cm3d_box_place io=%s,%s off=%s rest=%s n=%d,%d,%d waymo=%d thin=%g bound=%d out=%s,%s", who(box), who(flags),
           who(mask_off), rest ? "set" : "other", n_frames, n_masks, n_classes, waymo, thin, max_masks_per_frame,
           place_src == g_place_src ? "set" : "other", place_pushed == g_pushed ? "set" : "other");
}

// what csrc/pass_compose.cpp needs to link beyond that: the ground strip's and the point ownership's entry points.  No case here has a
// strip or an ownership, so none is called; one that were would print its line under the case
extern "C" {
int cm3d_ground_strip_check(double, double, double, double, int32_t, double, int32_t) { CALLED(CM3D_ERR_ARG, CM3D_OK, "cm3d_ground_strip_check"); }
int cm3d_ground_grid(const float *, const int32_t *, const float *, int32_t, const float *, const int32_t *, const int32_t *, int32_t, float, int32_t,
                     const double *, int32_t, double, double, double, double, int32_t, double *, int32_t *, cm3d_stream_t)
{
    CALLED(CM3D_ERR_WORKSPACE, CM3D_OK, "cm3d_ground_grid");
}
int cm3d_ground_strip(const float *, const int32_t *, const int32_t *, const int32_t *, int32_t, int32_t, const double *, const double *, int32_t, double,
                      double, int32_t, int32_t *, int32_t *, int32_t *, float *, int32_t *, int32_t *, void *, int64_t, cm3d_stream_t)
{
    CALLED(CM3D_ERR_WORKSPACE, CM3D_OK, "cm3d_ground_strip");
}
int cm3d_point_owner_check(int32_t, int32_t) { CALLED(CM3D_ERR_ARG, CM3D_OK, "cm3d_point_owner_check"); }
int cm3d_point_owner(const float *, const int32_t *, const int32_t *, const int32_t *, int32_t, int32_t, int32_t, int32_t, const double *, int32_t,
                     int32_t, int32_t *, int32_t *, int32_t *, int32_t *, float *, int32_t *, int32_t *, void *, int64_t, cm3d_stream_t)
{
    CALLED(CM3D_ERR_WORKSPACE, CM3D_OK, "cm3d_point_owner");
}
}

struct PlaceCase { Case k; cm3d_box_place_desc p; };

static void run_placed(const char *name, PlaceCase q, const char *which)
{
    Case &k = q.k;
    k.o.cluster = std::strchr(which, 'c') ? &k.c : nullptr, k.o.filter = std::strchr(which, 'f') ? &k.f : nullptr;
    k.o.yaw = std::strchr(which, 'y') ? &k.y : nullptr, k.o.nms = std::strchr(which, 'n') ? &k.n : nullptr;
    std::printf("case %s\n", name);
    g_trace = true, g_calls = 0, g_fail_at = -1;
    PlaceCase before;
    std::memcpy(&before, &q, sizeof q);
    const int rc = cm3d_lift_pass_placed(&q.k.p, &q.k.o, &q.p, nullptr);
    const int n = g_calls;
    std::printf("rc %d\n", rc);
    if (std::memcmp(&before, &q, sizeof q) != 0) std::printf("a caller's descriptor was changed\n");
    g_trace = false;
    for (int i = 0; i < n; ++i) {
        g_calls = 0, g_fail_at = i;
        const int ri = cm3d_lift_pass_placed(&q.k.p, &q.k.o, &q.p, nullptr);
        std::printf("fail %d %d %d\n", i, ri, g_calls);
    }
}

int main()
{
    // the descriptors of pass_options_sim.cpp's main, every event set
    PlaceCase q;
    std::memset(&q, 0, sizeof q);
    cm3d_lift_pass_desc &p = q.k.p;
    p.size = (int64_t)sizeof p;
    p.hit_off = g_hit_off, p.tile_off = g_tile_off, p.hit_idx = g_hit_idx, p.hit_xyz = g_hit_xyz, p.tile_work = g_tile_work;
    p.medoid_pos = g_medoid_pos, p.centroid_g = g_centroid, p.mask_frame = g_mask_frame;
    p.lane = g_lane, p.lane_off = g_lane_off, p.frame_lane = g_frame_lane, p.lane_idx = g_lane_idx, p.lane_dist = g_lane_dist;
    p.class_id = g_class, p.score = g_score, p.prior_wlh = g_prior, p.is_vehicle = g_veh, p.nms_group = g_group, p.nms_thr = g_thr;
    p.ego_xyz = g_ego, p.box = g_box, p.flags = g_flags, p.mask_off = g_mask_off;
    p.n_masks = 7, p.n_frames = 3, p.idx_cap = 4096, p.n_tables = 2, p.n_lane_points = 900, p.n_classes = 10, p.planes = 3;
    Case &k = q.k;
    k.c.size = (int64_t)sizeof k.c;
    k.c.origin = g_origin, k.c.cl_off = g_cl_off, k.c.cl_tile_off = g_cl_tile_off, k.c.cl_idx = g_cl_idx, k.c.cl_xyz = g_cl_xyz;
    k.c.cl_status = g_cl_status, k.c.ws = g_ws, k.c.ws_bytes = 16, k.c.eps = 1.0, k.c.min_points = 20, k.c.pick = 0;
    k.f.size = (int64_t)sizeof k.f;
    k.f.medoid_pos_kept = g_kept, k.f.on_road = g_on_road, k.f.lane_max_dist = 20.0, k.f.vehicle_lane_max_dist = 4.0;
    k.y.size = (int64_t)sizeof k.y;
    k.y.angle_cs = g_cs, k.y.fit_k = g_fit_k, k.y.fit_rect = g_rect, k.y.fit_status = g_fit_status, k.y.yaw_tab = g_yaw_tab, k.y.yaw_idx = g_yaw_idx;
    k.y.yaw_src = g_yaw_src, k.y.tab_off = g_tab_off, k.y.tab_frame = g_tab_frame;
    k.y.K = 128, k.y.min_points = 20, k.y.d0 = 0.05, k.y.min_length = 1.0, k.y.lane_min_dist = 0.0;
    k.n.size = (int64_t)sizeof k.n;
    k.n.thr = g_rot_thr, k.n.n_thr = 10, k.n.measure = 1, k.n.class_agnostic = 1;
    k.o.size = (int64_t)sizeof k.o;
    k = with_events(k);
    q.p.size = (int64_t)sizeof q.p;
    q.p.place_src = g_place_src, q.p.place_pushed = g_pushed, q.p.ev[0] = (void *)0x70, q.p.ev[1] = (void *)0x71, q.p.thin = 0.5;
    PlaceCase w = q;
    w.k.p.pose_rt = g_pose_rt, w.k.p.pose_inv = g_pose_inv, w.k.p.planes = 40;

    // ---- every presence combination of cluster, filter and nms, with yaw; nuScenes and Waymo descriptors
    for (int m = 0; m < 8; ++m) {
        char which[5] = "--y-", name[32];
        if (m & 1) which[0] = 'c';
        if (m & 2) which[1] = 'f';
        if (m & 4) which[3] = 'n';
        std::snprintf(name, sizeof name, "combo.%s", which);
        run_placed(name, q, which);
        std::snprintf(name, sizeof name, "combo_waymo.%s", which);
        run_placed(name, w, which);
    }
    PlaceCase e = q;
    e.p.ev[0] = e.p.ev[1] = nullptr, e.p.thin = 0.0;
    run_placed("ok.no_events_thin_0", e, "--yn");

    // ---- every refusal makes no call
    run_placed("bad.no_yaw", q, "cf-n");
    run_placed("bad.no_member", q, "----");
    e = q, e.p.size -= 8;
    run_placed("bad.place_size", e, "cfyn");
    e = q, e.k.o.size += 8;
    run_placed("bad.opt_size", e, "cfyn");
    e = q, e.k.p.size -= 8;
    run_placed("bad.pass_size", e, "cfyn");
    e = q, e.k.y.size -= 8;
    run_placed("bad.yaw_size", e, "--y-");
    e = q, e.k.n.size -= 8;
    run_placed("bad.nms_size", e, "--yn");
    e = q, e.k.n.thr = nullptr;
    run_placed("bad.nms_no_thr", e, "cfyn");
    e = q, e.k.c.size -= 8;
    run_placed("bad.cluster_size", e, "cfyn");
    e = q, e.k.f.on_road = nullptr;
    run_placed("bad.filter_no_on_road", e, "-fy-");
    e = q, e.p.place_src = nullptr;
    run_placed("bad.no_place_src", e, "--y-");
    e = q, e.p.place_pushed = nullptr;
    run_placed("bad.no_place_pushed", e, "--yn");
    e = q, e.k.y.fit_rect = nullptr;
    run_placed("bad.yaw_no_fit_rect", e, "--y-");
    e = q, e.k.y.yaw_src = nullptr;
    run_placed("bad.yaw_no_yaw_src", e, "--y-");
    e = q, e.k.y.tab_off = nullptr;
    run_placed("bad.yaw_no_tab_off", e, "--y-");
    e = q, e.p.thin = -0.5;
    run_placed("bad.thin_negative", e, "--y-");
    e = q, e.p.thin = std::nan("");
    run_placed("bad.thin_nan", e, "--y-");
    e = q, e.p.thin = HUGE_VAL;
    run_placed("bad.thin_inf", e, "--y-");
    g_trace = true, g_fail_at = -1;                      // (a call would print its line under the case)
    std::printf("case bad.null_place\nrc %d\n", cm3d_lift_pass_placed(&q.k.p, &q.k.o, nullptr, nullptr));
    std::printf("case bad.null_opt\nrc %d\n", cm3d_lift_pass_placed(&q.k.p, nullptr, &q.p, nullptr));
    {
        PlaceCase y = q;
        y.k.o.yaw = &y.k.y;
        std::printf("case bad.null_pass\nrc %d\n", cm3d_lift_pass_placed(nullptr, &y.k.o, &y.p, nullptr));
    }
    std::printf("pass_place_sim done\n");
    return 0;
}
