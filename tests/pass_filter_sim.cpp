// Stand-alone trace of cm3d_lift_pass_filtered (cm3d_amd/csrc/pass_filter.cpp) over stubs of the three entry points it calls and of
// hipEventRecord (tests/test_drivable_host.py builds it with the address and undefined-behaviour sanitizers and compares the output
// with the sequence include/cm3d_hip.h states).  Per case: the calls of a clean pass, one line each with the arguments that matter,
// then `rc`; then, for every call k of that pass, `fail k rc calls`: the pass again with call k answering an error.
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
#define STAGE(...) CALLED(CM3D_ERR_LAUNCH, CM3D_OK, __VA_ARGS__)
static const char *set(const void *p) { return p ? "set" : "null"; }
static unsigned id(const void *p) { return (unsigned)(uintptr_t)p; }

static int32_t g_med[4], g_kept[4];

extern "C" {
hipError_t hipEventRecord(hipEvent_t ev, hipStream_t) { CALLED(hipErrorInvalidValue, hipSuccess, "record %#x", id(ev)); }

int cm3d_lift_pass(const cm3d_lift_pass_desc *d, cm3d_stream_t) { STAGE("cm3d_lift_pass size=%s", d->size == (int64_t)sizeof *d ? "ok" : "bad"); }
int cm3d_stage2_filter(const float *, const int32_t *medoid_pos, const int32_t *, const int32_t *, const int32_t *, const double *, int32_t n_masks,
                       int32_t n_frames, const double *tab_y, const int32_t *, const int32_t *, const int32_t *, const int32_t *, const double *,
                       const int32_t *, int32_t n_tables, const int32_t *needs_road, const int32_t *, int32_t n_classes, double lane_max_dist,
                       double vehicle_lane_max_dist, int32_t *medoid_pos_kept, uint8_t *on_road, cm3d_stream_t)
{
    STAGE("cm3d_stage2_filter med=%s n=%d,%d,%d polygons=%s tables=%d needs_road=%s thr=%g,%g kept=%s on_road=%s",
          medoid_pos == g_med ? "pass" : "other", n_masks, n_frames, n_classes, set(tab_y), n_tables, set(needs_road), lane_max_dist,
          vehicle_lane_max_dist, medoid_pos_kept == g_kept ? "kept" : "other", set(on_road));
}
int cm3d_box_nms_bounded(const float *, const int32_t *medoid_pos, const int32_t *, int32_t, int32_t, const int32_t *, const double *, const float *,
                         const int32_t *, const int32_t *, const int32_t *, const double *, const double *, const int32_t *, const int32_t *,
                         const double *, int32_t, const double *, const float *pose_inv, int32_t max_masks_per_frame, double *, int32_t *,
                         cm3d_stream_t)
{
    STAGE("cm3d_box_nms_bounded med=%s bound=%d pose_inv=%s", medoid_pos == g_kept ? "kept" : "other", max_masks_per_frame, set(pose_inv));
}
}

static void run_case(const char *name, const cm3d_lift_pass_desc *d, const cm3d_stage2_filter_desc *f)
{
    std::printf("case %s\n", name);
    g_trace = true, g_calls = 0, g_fail_at = -1;
    const int rc = cm3d_lift_pass_filtered(d, f, nullptr);
    const int n = g_calls;
    std::printf("rc %d\n", rc);
    g_trace = false;
    for (int k = 0; k < n; ++k) {
        g_calls = 0, g_fail_at = k;
        const int rk = cm3d_lift_pass_filtered(d, f, nullptr);
        std::printf("fail %d %d %d\n", k, rk, g_calls);
    }
}

int main()
{
    static double g_d[4];
    static int32_t g_i[4];
    static uint8_t g_b[4];
    static float g_f[4];
    cm3d_lift_pass_desc p;
    std::memset(&p, 0, sizeof p);
    p.size = (int64_t)sizeof p;
    p.medoid_pos = g_med, p.n_masks = 7, p.n_frames = 3, p.n_classes = 10, p.planes = 1, p.n_tables = 2;
    cm3d_stage2_filter_desc q;
    std::memset(&q, 0, sizeof q);
    q.size = (int64_t)sizeof q;
    q.medoid_pos_kept = g_kept, q.on_road = g_b;
    q.lane_max_dist = 20.0, q.vehicle_lane_max_dist = 4.0;

    cm3d_stage2_filter_desc f = q;
    run_case("lanes_only", &p, &f);
    f = q, f.tab_y = g_d, f.tab_slab = g_i, f.slab_off = g_i, f.ent_edge = g_i, f.ent_ring = g_i, f.edge = g_d, f.ring_info = g_i;
    f.needs_road = g_i, f.n_poly_tables = 2;
    run_case("polygons", &p, &f);
    f = q, f.ev[0] = (void *)0x40, f.ev[1] = (void *)0x41;
    run_case("events", &p, &f);
    cm3d_lift_pass_desc d = p;
    d.pose_inv = g_f, d.planes = 3;
    f = q;
    run_case("pose_planes", &d, &f);
    d.planes = 32;
    run_case("planes_32", &d, &f);
    f = q, f.size -= 8;
    run_case("wrong_size", &p, &f);
    f = q, f.medoid_pos_kept = nullptr;
    run_case("no_output", &p, &f);
    f = q;
    run_case("null_pass", nullptr, &f);
    run_case("null_filter", &p, nullptr);
    std::printf("pass_filter_sim done\n");
    return 0;
}
