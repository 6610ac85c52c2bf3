// Stand-alone trace of cm3d_lift_pass_clustered (cm3d_amd/csrc/pass_cluster.cpp) over stubs of the three entry points it calls and of
// hipEventRecord (tests/test_depth_cluster_host.py builds it with the address and undefined-behaviour sanitizers and compares the
// output with the sequence include/cm3d_hip.h states).  Per case: the calls of a clean pass, one line each with the arguments that
// matter, then `rc`; then, for every call k of that pass, `fail k rc calls`: the pass again with call k answering an error.
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
static const char *set(const void *p) { return p ? "set" : "null"; }
static unsigned id(const void *p) { return (unsigned)(uintptr_t)p; }

// the raw lists of the pass and the clustered ones: the stubs say which of the two they were handed
static int32_t g_hit_off[4], g_tile_off[4], g_hit_idx[4], g_tile_work[4], g_cl_off[4], g_cl_tile_off[4], g_cl_idx[4], g_cl_status[4], g_frame[4];
static float g_hit_xyz[4], g_cl_xyz[4];
static double g_origin[4];
static uint8_t g_ws[16];

static const char *which(const void *p, const void *raw, const void *cl) { return !p ? "null" : p == raw ? "raw" : p == cl ? "cl" : "other"; }

extern "C" {
hipError_t hipEventRecord(hipEvent_t ev, hipStream_t) { CALLED(hipErrorInvalidValue, hipSuccess, "record %#x", id(ev)); }

static int half(const char *name, const cm3d_lift_pass_desc *d)
{
    CALLED(CM3D_ERR_LAUNCH, CM3D_OK, "%s size=%s hit_off=%s tile_off=%s hit_idx=%s hit_xyz=%s tile_work=%s n_masks=%d", name,
           d->size == (int64_t)sizeof *d ? "ok" : "bad", which(d->hit_off, g_hit_off, g_cl_off), which(d->tile_off, g_tile_off, g_cl_tile_off),
           which(d->hit_idx, g_hit_idx, g_cl_idx), which(d->hit_xyz, g_hit_xyz, g_cl_xyz), which(d->tile_work, g_tile_work, nullptr),
           d->n_masks);
}
int cm3d_lift_pass_head(const cm3d_lift_pass_desc *d, cm3d_stream_t) { return half("cm3d_lift_pass_head", d); }
int cm3d_lift_pass_tail(const cm3d_lift_pass_desc *d, cm3d_stream_t) { return half("cm3d_lift_pass_tail", d); }
int cm3d_depth_cluster(const float *hit_xyz, const int32_t *hit_idx, const int32_t *hit_off, const int32_t *mask_frame, int32_t n_masks,
                       int32_t idx_cap, const double *origin, int32_t n_frames, double eps, int32_t min_points, int32_t pick, int32_t *cl_off,
                       int32_t *cl_tile_off, int32_t *cl_idx, float *cl_xyz, int32_t *cl_status, void *workspace, int64_t workspace_bytes,
                       cm3d_stream_t)
{
    CALLED(CM3D_ERR_WORKSPACE, CM3D_OK,
           "cm3d_depth_cluster in=%s,%s,%s frame=%s n=%d,%d,%d origin=%s eps=%g min=%d pick=%d out=%s,%s,%s,%s status=%s ws=%s,%lld",
           which(hit_xyz, g_hit_xyz, g_cl_xyz), which(hit_idx, g_hit_idx, g_cl_idx), which(hit_off, g_hit_off, g_cl_off), set(mask_frame),
           n_masks, idx_cap, n_frames, origin == g_origin ? "set" : "other", eps, min_points, pick, which(cl_off, g_hit_off, g_cl_off),
           which(cl_tile_off, g_tile_off, g_cl_tile_off), which(cl_idx, g_hit_idx, g_cl_idx), which(cl_xyz, g_hit_xyz, g_cl_xyz),
           set(cl_status), set(workspace), (long long)workspace_bytes);
}
}

static void run_case(const char *name, const cm3d_lift_pass_desc *d, const cm3d_depth_cluster_desc *c)
{
    std::printf("case %s\n", name);
    g_trace = true, g_calls = 0, g_fail_at = -1;
    const cm3d_lift_pass_desc before = d ? *d : cm3d_lift_pass_desc();
    const int rc = cm3d_lift_pass_clustered(d, c, nullptr);
    const int n = g_calls;
    std::printf("rc %d\n", rc);
    if (d && std::memcmp(&before, d, sizeof before) != 0) std::printf("the caller's descriptor was changed\n");
    g_trace = false;
    for (int k = 0; k < n; ++k) {
        g_calls = 0, g_fail_at = k;
        const int rk = cm3d_lift_pass_clustered(d, c, nullptr);
        std::printf("fail %d %d %d\n", k, rk, g_calls);
    }
}

int main()
{
    cm3d_lift_pass_desc p;
    std::memset(&p, 0, sizeof p);
    p.size = (int64_t)sizeof p;
    p.hit_off = g_hit_off, p.tile_off = g_tile_off, p.hit_idx = g_hit_idx, p.hit_xyz = g_hit_xyz, p.tile_work = g_tile_work;
    p.mask_frame = g_frame, p.n_masks = 7, p.n_frames = 3, p.idx_cap = 4096;
    cm3d_depth_cluster_desc q;
    std::memset(&q, 0, sizeof q);
    q.size = (int64_t)sizeof q;
    q.origin = g_origin, q.cl_off = g_cl_off, q.cl_tile_off = g_cl_tile_off, q.cl_idx = g_cl_idx, q.cl_xyz = g_cl_xyz, q.cl_status = g_cl_status;
    q.ws = g_ws, q.ws_bytes = 16, q.eps = 1.0, q.min_points = 20, q.pick = 0;

    cm3d_depth_cluster_desc c = q;
    run_case("plain", &p, &c);
    c = q, c.ev[0] = (void *)0x50, c.ev[1] = (void *)0x51, c.eps = 0.5, c.min_points = 3, c.pick = 1;
    run_case("events", &p, &c);
    c = q, c.size -= 8;
    run_case("wrong_size", &p, &c);
    const char *outs[] = {"no_cl_off", "no_cl_tile_off", "no_cl_idx", "no_cl_xyz", "no_cl_status"};
    for (int k = 0; k < 5; ++k) {
        c = q;
        if (k == 0) c.cl_off = nullptr;
        if (k == 1) c.cl_tile_off = nullptr;
        if (k == 2) c.cl_idx = nullptr;
        if (k == 3) c.cl_xyz = nullptr;
        if (k == 4) c.cl_status = nullptr;
        run_case(outs[k], &p, &c);
    }
    c = q;
    run_case("null_pass", nullptr, &c);
    run_case("null_cluster", &p, nullptr);
    std::printf("pass_cluster_sim done\n");
    return 0;
}
