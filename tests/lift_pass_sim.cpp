// Stand-alone trace of cm3d_lift_pass (cm3d_amd/csrc/pipeline.cpp) over stubs of the stage entry points and of the runtime calls the
// file uses (tests/test_pipe_sched_host.py builds it with the address and undefined-behaviour sanitizers and compares the output with
// the sequence include/cm3d_hip.h states).  Per case: the calls of a clean pass, one line each with the arguments that select a route,
// then `rc`; then, for every call k of that pass, `fail k rc calls`: the pass again with call k answering an error.
#include <hip/hip_runtime_api.h>

#include <cstdint>
#include <cstdio>
#include <cstring>

#include "../include/cm3d_hip.h"

static int g_calls = 0, g_fail_at = -1;
static bool g_trace = true;

// prints the call, counts it, and answers an error if it is the one that has to fail
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
#define RUNTIME(...) CALLED(hipErrorInvalidValue, hipSuccess, __VA_ARGS__)
static const char *set(const void *p) { return p ? "set" : "null"; }
static unsigned id(const void *p) { return (unsigned)(uintptr_t)p; }

extern "C" {
hipError_t hipEventRecord(hipEvent_t ev, hipStream_t) { RUNTIME("record %#x", id(ev)); }
hipError_t hipStreamWaitEvent(hipStream_t, hipEvent_t ev, unsigned) { RUNTIME("wait %#x", id(ev)); }
// (the pipeline object's: linked, not called here)
hipError_t hipEventQuery(hipEvent_t) { return hipSuccess; }
hipError_t hipGetLastError(void) { return hipSuccess; }
hipError_t hipEventCreateWithFlags(hipEvent_t *, unsigned) { return hipErrorInvalidValue; }
hipError_t hipEventDestroy(hipEvent_t) { return hipSuccess; }
hipError_t hipEventSynchronize(hipEvent_t) { return hipSuccess; }

int cm3d_batch_begin(int32_t *, int32_t *, int32_t, uint32_t *, int64_t, cm3d_stream_t) { STAGE("cm3d_batch_begin"); }
int cm3d_sweep_prep(const float *, int32_t, const float *, const int32_t *, int32_t, int32_t max_rows_per_sweep, const float *, const int32_t *,
                    int32_t, float, float *points, int32_t, int32_t *, uint32_t *, int32_t *, cm3d_stream_t)
{
    STAGE("cm3d_sweep_prep max_rows=%d points=%s", max_rows_per_sweep, set(points));
}
int cm3d_erode_pack(const uint8_t *dense, int32_t, int32_t, int32_t, uint32_t *, int32_t *, cm3d_stream_t)
{
    STAGE("cm3d_erode_pack dense=%s", set(dense));
}
int cm3d_rle_erode_pack(const uint32_t *, const int32_t *, int32_t, int32_t, int32_t, int32_t, uint32_t *, int32_t *, void *, int64_t,
                        cm3d_stream_t)
{
    STAGE("cm3d_rle_erode_pack");
}
int cm3d_rle_erode_pack_begin(const uint32_t *, const int32_t *, int32_t, int32_t, int32_t, int32_t, uint32_t *, int32_t *, void *, int64_t,
                              int32_t *, int32_t *, int32_t, uint32_t *, int64_t, cm3d_stream_t)
{
    STAGE("cm3d_rle_erode_pack_begin");
}
int cm3d_rle_erode_pack_sized(const uint32_t *, const int32_t *, int32_t, int32_t, int32_t, int32_t, const int32_t *mask_wh, uint32_t *,
                              int32_t *, void *, int64_t, cm3d_stream_t)
{
    STAGE("cm3d_rle_erode_pack_sized mask_wh=%s", set(mask_wh));
}
int cm3d_rle_erode_pack_sized_begin(const uint32_t *, const int32_t *, int32_t, int32_t, int32_t, int32_t, const int32_t *mask_wh, uint32_t *,
                                    int32_t *, void *, int64_t, int32_t *, int32_t *, int32_t, uint32_t *, int64_t, cm3d_stream_t)
{
    STAGE("cm3d_rle_erode_pack_sized_begin mask_wh=%s", set(mask_wh));
}
int cm3d_project_hits(const float *points, const int32_t *, int32_t, int32_t, int32_t, const float *, int32_t, const int32_t *, const int32_t *,
                      const int32_t *, const uint32_t *, int32_t, int32_t, int32_t, float, int32_t, uint32_t *, int32_t *, int32_t *, void *,
                      int64_t, void *ev_start, void *ev_stop, cm3d_stream_t)
{
    STAGE("cm3d_project_hits points=%s ev=%#x,%#x", set(points), id(ev_start), id(ev_stop));
}
int cm3d_sweep_project_hits(const float *, int32_t, const float *, const int32_t *, int32_t, int32_t, const float *, const int32_t *, float,
                            float *points, int32_t, int32_t *, uint32_t *, int32_t, int32_t, int32_t, const float *, int32_t, const int32_t *,
                            const int32_t *, const int32_t *, const uint32_t *, int32_t, int32_t, int32_t, float, int32_t, uint32_t *,
                            int32_t *, int32_t *, void *, int64_t, void *ev_start, void *ev_stop, cm3d_stream_t)
{
    STAGE("cm3d_sweep_project_hits points=%s ev=%#x,%#x", set(points), id(ev_start), id(ev_stop));
}
int cm3d_compact_hits(const uint32_t *, int32_t, int32_t, int32_t, int32_t, const int32_t *, int32_t, const int32_t *, const uint32_t *,
                      const float *raw, int32_t, const float *intensity, const float *sweep_xf, const float *points, int32_t *, int32_t *,
                      int32_t *, int32_t *, float *, int32_t, int32_t *, int32_t *, void *, int64_t, cm3d_stream_t)
{
    STAGE("cm3d_compact_hits raw=%s intensity=%s sweep_xf=%s points=%s", set(raw), set(intensity), set(sweep_xf), set(points));
}
int cm3d_medoid2(const float *, const int32_t *, const int32_t *, int32_t, const int32_t *, const int32_t *, const int32_t *, int32_t,
                 const int32_t *, int32_t *, float *, float *, void *, int64_t, int32_t flags, int32_t *, cm3d_stream_t)
{
    STAGE("cm3d_medoid2 flags=%d", flags);
}
int cm3d_centroid_transform(const float *, const int32_t *, const int32_t *, int32_t, const float *pose_rt, float *, cm3d_stream_t)
{
    STAGE("cm3d_centroid_transform pose_rt=%s", set(pose_rt));
}
int cm3d_lane_nn(const float *, const int32_t *, const int32_t *, int32_t, const float *, const int32_t *, const int32_t *, int32_t, int32_t,
                 const void *, int32_t *, double *, void *, int64_t, cm3d_stream_t)
{
    STAGE("cm3d_lane_nn");
}
int cm3d_box_nms_bounded(const float *, const int32_t *, const int32_t *, int32_t, int32_t, const int32_t *, const double *, const float *,
                         const int32_t *, const int32_t *, const int32_t *, const double *, const double *, const int32_t *, const int32_t *,
                         const double *, int32_t, const double *, const float *pose_inv, int32_t max_masks_per_frame, double *, int32_t *,
                         cm3d_stream_t)
{
    STAGE("cm3d_box_nms_bounded bound=%d pose_inv=%s", max_masks_per_frame, set(pose_inv));
}
int cm3d_obb(const float *, const int32_t *, int32_t, int32_t, double *yaw, int32_t *, double *, uint8_t *, void *, int64_t, cm3d_stream_t)
{
    STAGE("cm3d_obb yaw=%s", set(yaw));
}
}

// nothing behind these pointers is ever read: the stubs only look at which are set
static float g_f[4];
static int32_t g_i[4];
static double g_d[4];
static uint8_t g_b[4];

static void run_case(const char *name, cm3d_lift_pass_desc d)
{
    std::printf("case %s\n", name);
    g_trace = true, g_calls = 0, g_fail_at = -1;
    const int rc = cm3d_lift_pass(&d, nullptr);
    const int n = g_calls;
    std::printf("rc %d\n", rc);
    g_trace = false;
    for (int k = 0; k < n; ++k) {
        g_calls = 0, g_fail_at = k;
        const int rk = cm3d_lift_pass(&d, nullptr);
        std::printf("fail %d %d %d\n", k, rk, g_calls);
    }
}

int main()
{
    int32_t feedback = 1;
    cm3d_lift_pass_desc p;
    std::memset(&p, 0, sizeof p);
    p.size = (int64_t)sizeof p;
    p.raw = g_f, p.intensity = g_f, p.sweep_xf = g_f;       // the plain pass: fused sweeps, no cloud, one plane of mask bits
    p.fused = 1, p.planes = 1, p.max_rows_per_sweep = 77;
    p.md_feedback = &feedback;

    cm3d_lift_pass_desc d = p;
    run_case("plain", d);
    d = p, d.separate_reset = 1;
    run_case("separate_reset", d);
    d = p, d.mask_wh = g_i;
    run_case("mask_wh", d);
    d = p, d.mask_wh = g_i, d.separate_reset = 1;
    run_case("mask_wh+separate_reset", d);
    d = p, d.dense = g_b;
    run_case("dense", d);
    d = p, d.fused = 0, d.points = g_f, d.planes = 2;
    run_case("not_fused", d);
    d = p, d.fused = 0, d.points = g_f, d.dense = g_b;
    run_case("not_fused+dense", d);
    d = p, d.pose_rt = g_f, d.pose_inv = g_f, d.planes = 32;
    run_case("pose", d);
    d = p, d.obb_yaw = g_d, d.obb_status = g_i, d.obb_ws = g_b;
    run_case("obb", d);
    d = p, d.lane_ready = (void *)0x30;
    run_case("lane_ready", d);
    d = p, d.ev_project[0] = (void *)0x20, d.ev_project[1] = (void *)0x21;
    for (int i = 0; i < 5; ++i) d.ev_stage[i] = (void *)(uintptr_t)(0x10 + i);
    run_case("events", d);
    d = p, d.md_hint = 1, feedback = 0;
    run_case("md_hint_feedback_0", d);
    feedback = 1;
    run_case("md_hint_feedback_1", d);
    d = p, d.size -= 8;
    run_case("wrong_size", d);
    d = p, d.fused = 0;
    run_case("not_fused_without_cloud", d);
    std::printf("lift_pass_sim done\n");
    return 0;
}
