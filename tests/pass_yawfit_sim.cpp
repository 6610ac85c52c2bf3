// Stand-alone trace of cm3d_lift_pass_yaw_fitted and cm3d_yaw_fit_boxes (cm3d_amd/csrc/pass_yawfit.cpp) over stubs of the four entry
// points they call and of hipEventRecord (tests/test_bev_fit_host.py builds it with the address and undefined-behaviour sanitizers and
// compares the output with the sequence include/cm3d_hip.h states).  Per case: the calls of a clean pass, one line each with the
// arguments that matter, then `rc`; then, for every call k of that pass, `fail k rc calls`: the pass again with call k answering an error.
#include <hip/hip_runtime_api.h>

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
static unsigned id(const void *p) { return (unsigned)(uintptr_t)p; }

// what the pass owns and what the fit owns: the stubs say whose array they were handed
static int32_t g_hit_off[4], g_cl_off[4], g_medoid_pos[4], g_kept[4], g_lane_off[4], g_frame_lane[4], g_lane_idx[4], g_mask_frame[4], g_class[4],
    g_veh[4], g_fit_k[4], g_fit_status[4], g_yaw_idx[4], g_yaw_src[4], g_tab_off[2], g_tab_frame[4], g_mask_off[4], g_flags[4], g_group[4];
static float g_hit_xyz[4], g_cl_xyz[4], g_lane[4], g_yaw_tab[4], g_centroid[4], g_pose_rt[12], g_pose_inv[16];
static double g_cs[4], g_rect[8], g_lane_dist[4], g_score[4], g_prior[4], g_thr[4], g_ego[4], g_box[4];

struct Name { const void *p; const char *n; };
static const char *who(const void *p)
{
    const Name names[] = {{g_hit_off, "hit_off"}, {g_cl_off, "cl_off"}, {g_medoid_pos, "medoid_pos"}, {g_kept, "kept"}, {g_lane_off, "lane_off"},
                          {g_frame_lane, "frame_lane"}, {g_lane_idx, "lane_idx"}, {g_yaw_idx, "yaw_idx"}, {g_tab_off, "tab_off"},
                          {g_tab_frame, "tab_frame"}, {g_hit_xyz, "hit_xyz"}, {g_cl_xyz, "cl_xyz"}, {g_lane, "lane"}, {g_yaw_tab, "yaw_tab"},
                          {g_pose_rt, "pose_rt"}, {g_pose_inv, "pose_inv"}, {g_lane_dist, "lane_dist"}, {g_box, "box"}, {g_flags, "flags"}};
    if (!p) return "null";
    for (const Name &e : names)
        if (e.p == p) return e.n;
    return "other";
}

extern "C" {
hipError_t hipEventRecord(hipEvent_t ev, hipStream_t) { CALLED(hipErrorInvalidValue, hipSuccess, "record %#x", id(ev)); }

int cm3d_lift_pass(const cm3d_lift_pass_desc *d, cm3d_stream_t)
{
    CALLED(CM3D_ERR_LAUNCH, CM3D_OK, "cm3d_lift_pass size=%s n_masks=%d", d->size == (int64_t)sizeof *d ? "ok" : "bad", d->n_masks);
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
}

typedef int (*entry_t)(const cm3d_lift_pass_desc *, const cm3d_yaw_fit_desc *, cm3d_stream_t);

static void run_case(const char *name, entry_t fn, const cm3d_lift_pass_desc *d, const cm3d_yaw_fit_desc *y)
{
    std::printf("case %s\n", name);
    g_trace = true, g_calls = 0, g_fail_at = -1;
    const cm3d_lift_pass_desc before = d ? *d : cm3d_lift_pass_desc();
    const cm3d_yaw_fit_desc ybefore = y ? *y : cm3d_yaw_fit_desc();
    const int rc = fn(d, y, nullptr);
    const int n = g_calls;
    std::printf("rc %d\n", rc);
    if ((d && std::memcmp(&before, d, sizeof before) != 0) || (y && std::memcmp(&ybefore, y, sizeof ybefore) != 0))
        std::printf("a caller's descriptor was changed\n");
    g_trace = false;
    for (int k = 0; k < n; ++k) {
        g_calls = 0, g_fail_at = k;
        const int rk = fn(d, y, nullptr);
        std::printf("fail %d %d %d\n", k, rk, g_calls);
    }
}

int main()
{
    cm3d_lift_pass_desc p;
    std::memset(&p, 0, sizeof p);
    p.size = (int64_t)sizeof p;
    p.hit_off = g_hit_off, p.hit_xyz = g_hit_xyz, p.medoid_pos = g_medoid_pos, p.centroid_g = g_centroid, p.mask_frame = g_mask_frame;
    p.lane = g_lane, p.lane_off = g_lane_off, p.frame_lane = g_frame_lane, p.lane_idx = g_lane_idx, p.lane_dist = g_lane_dist;
    p.class_id = g_class, p.score = g_score, p.prior_wlh = g_prior, p.is_vehicle = g_veh, p.nms_group = g_group, p.nms_thr = g_thr;
    p.ego_xyz = g_ego, p.box = g_box, p.flags = g_flags, p.mask_off = g_mask_off;
    p.n_masks = 7, p.n_frames = 3, p.idx_cap = 4096, p.n_tables = 2, p.n_lane_points = 900, p.n_classes = 10, p.planes = 3;
    cm3d_yaw_fit_desc q;
    std::memset(&q, 0, sizeof q);
    q.size = (int64_t)sizeof q;
    q.angle_cs = g_cs, q.fit_k = g_fit_k, q.fit_rect = g_rect, q.fit_status = g_fit_status, q.yaw_tab = g_yaw_tab, q.yaw_idx = g_yaw_idx;
    q.yaw_src = g_yaw_src, q.tab_off = g_tab_off, q.tab_frame = g_tab_frame;
    q.K = 128, q.min_points = 20, q.d0 = 0.05, q.min_length = 1.0, q.lane_min_dist = 0.0;

    cm3d_yaw_fit_desc y = q;
    run_case("plain", cm3d_lift_pass_yaw_fitted, &p, &y);
    run_case("boxes_alone", cm3d_yaw_fit_boxes, &p, &y);
    y = q, y.ev[0] = (void *)0x50, y.ev[1] = (void *)0x51, y.K = 64, y.min_points = 5, y.d0 = 0.1, y.min_length = 2.5, y.lane_min_dist = 1.5;
    y.hit_xyz = g_cl_xyz, y.hit_off = g_cl_off, y.medoid_pos = g_kept;
    cm3d_lift_pass_desc w = p;
    w.pose_rt = g_pose_rt, w.pose_inv = g_pose_inv, w.planes = 40;
    run_case("waymo_events_own_lists", cm3d_lift_pass_yaw_fitted, &w, &y);
    y = q, y.size -= 8;
    run_case("wrong_size", cm3d_lift_pass_yaw_fitted, &p, &y);
    run_case("wrong_size_boxes", cm3d_yaw_fit_boxes, &p, &y);
    w = p, w.size += 8, y = q;
    run_case("wrong_pass_size", cm3d_lift_pass_yaw_fitted, &w, &y);
    const char *outs[] = {"no_angle_cs", "no_fit_k", "no_fit_rect", "no_fit_status", "no_yaw_tab", "no_yaw_idx", "no_yaw_src", "no_tab_off",
                          "no_tab_frame"};
    for (int k = 0; k < 9; ++k) {
        y = q;
        if (k == 0) y.angle_cs = nullptr;
        if (k == 1) y.fit_k = nullptr;
        if (k == 2) y.fit_rect = nullptr;
        if (k == 3) y.fit_status = nullptr;
        if (k == 4) y.yaw_tab = nullptr;
        if (k == 5) y.yaw_idx = nullptr;
        if (k == 6) y.yaw_src = nullptr;
        if (k == 7) y.tab_off = nullptr;
        if (k == 8) y.tab_frame = nullptr;
        run_case(outs[k], k & 1 ? cm3d_yaw_fit_boxes : cm3d_lift_pass_yaw_fitted, &p, &y);
    }
    y = q;
    run_case("null_pass", cm3d_lift_pass_yaw_fitted, nullptr, &y);
    run_case("null_fit", cm3d_yaw_fit_boxes, &p, nullptr);
    std::printf("pass_yawfit_sim done\n");
    return 0;
}
