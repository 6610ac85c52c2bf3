// Stand-alone check of the pipeline object's executors (cm3d_amd/csrc/pipeline.cpp, csrc/pipe_sched.h: pipe_exec_plan, cm3d_pipe_create2,
// cm3d_pipe_null_exec) over stubs of the stage entry points and of the runtime calls, in the manner of tests/lift_pass_sim.cpp
// (tests/test_pipe_null_exec_host.py builds it with the address and undefined-behaviour sanitizers).  Every stub logs the stream it was
// given; the program checks the log itself and prints what the Python side compares with the values the header states:
//   plan <depth> <queues> <n_exec> <null_last>      the listed plans
//   pass <depth> <queues, or minus an explicit executor count> <k> <slot> <exec> <handle> <waited>     one line per pass of a trace
//   fail <position> <rc> <calls> <event_recorded>   a pass of the null executor with call <position> answering an error
#include <hip/hip_runtime_api.h>

#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "../cm3d_amd/csrc/pipe_sched.h"
#include "../include/cm3d_hip.h"

#define CHECK(cond)                                                            \
    do {                                                                       \
        if (!(cond)) {                                                         \
            std::printf("FAILED %s:%d: %s\n", __FILE__, __LINE__, #cond);      \
            std::exit(1);                                                      \
        }                                                                      \
    } while (0)

struct Call {
    std::string what;
    uintptr_t stream, event;
};
static std::vector<Call> g_log;
static int g_fail_at = -1;            // the call (position in g_log) that answers an error
static bool g_events_pending = true;  // hipEventQuery: not ready, so that every wait the scheduler asks for is made
static uintptr_t g_next_event = 0xE00;

static bool logged(const char *what, const void *stream, const void *event = nullptr)
{
    g_log.push_back({what, (uintptr_t)stream, (uintptr_t)event});
    return (int)g_log.size() - 1 == g_fail_at;
}
#define STAGE(st) return logged(__func__, st) ? CM3D_ERR_LAUNCH : CM3D_OK

extern "C" {
hipError_t hipEventRecord(hipEvent_t ev, hipStream_t st) { return logged("record", st, ev) ? hipErrorInvalidValue : hipSuccess; }
hipError_t hipStreamWaitEvent(hipStream_t st, hipEvent_t ev, unsigned) { return logged("wait", st, ev) ? hipErrorInvalidValue : hipSuccess; }
hipError_t hipEventQuery(hipEvent_t) { return g_events_pending ? hipErrorNotReady : hipSuccess; }
hipError_t hipGetLastError(void) { return hipSuccess; }
hipError_t hipEventCreateWithFlags(hipEvent_t *ev, unsigned)
{
    *ev = (hipEvent_t)(g_next_event++);
    return hipSuccess;
}
hipError_t hipEventDestroy(hipEvent_t) { return hipSuccess; }
hipError_t hipEventSynchronize(hipEvent_t ev) { return logged("sync", nullptr, ev) ? hipErrorInvalidValue : hipSuccess; }

int cm3d_batch_begin(int32_t *, int32_t *, int32_t, uint32_t *, int64_t, cm3d_stream_t st) { STAGE(st); }
int cm3d_sweep_prep(const float *, int32_t, const float *, const int32_t *, int32_t, int32_t, const float *, const int32_t *, int32_t, float,
                    float *, int32_t, int32_t *, uint32_t *, int32_t *, cm3d_stream_t st)
{
    STAGE(st);
}
int cm3d_erode_pack(const uint8_t *, int32_t, int32_t, int32_t, uint32_t *, int32_t *, cm3d_stream_t st) { STAGE(st); }
int cm3d_rle_erode_pack(const uint32_t *, const int32_t *, int32_t, int32_t, int32_t, int32_t, uint32_t *, int32_t *, void *, int64_t,
                        cm3d_stream_t st)
{
    STAGE(st);
}
int cm3d_rle_erode_pack_begin(const uint32_t *, const int32_t *, int32_t, int32_t, int32_t, int32_t, uint32_t *, int32_t *, void *, int64_t,
                              int32_t *, int32_t *, int32_t, uint32_t *, int64_t, cm3d_stream_t st)
{
    STAGE(st);
}
int cm3d_rle_erode_pack_sized(const uint32_t *, const int32_t *, int32_t, int32_t, int32_t, int32_t, const int32_t *, uint32_t *, int32_t *,
                              void *, int64_t, cm3d_stream_t st)
{
    STAGE(st);
}
int cm3d_rle_erode_pack_sized_begin(const uint32_t *, const int32_t *, int32_t, int32_t, int32_t, int32_t, const int32_t *, uint32_t *,
                                    int32_t *, void *, int64_t, int32_t *, int32_t *, int32_t, uint32_t *, int64_t, cm3d_stream_t st)
{
    STAGE(st);
}
int cm3d_project_hits(const float *, const int32_t *, int32_t, int32_t, int32_t, const float *, int32_t, const int32_t *, const int32_t *,
                      const int32_t *, const uint32_t *, int32_t, int32_t, int32_t, float, int32_t, uint32_t *, int32_t *, int32_t *, void *,
                      int64_t, void *, void *, cm3d_stream_t st)
{
    STAGE(st);
}
int cm3d_sweep_project_hits(const float *, int32_t, const float *, const int32_t *, int32_t, int32_t, const float *, const int32_t *, float,
                            float *, int32_t, int32_t *, uint32_t *, int32_t, int32_t, int32_t, const float *, int32_t, const int32_t *,
                            const int32_t *, const int32_t *, const uint32_t *, int32_t, int32_t, int32_t, float, int32_t, uint32_t *,
                            int32_t *, int32_t *, void *, int64_t, void *, void *, cm3d_stream_t st)
{
    STAGE(st);
}
int cm3d_compact_hits(const uint32_t *, int32_t, int32_t, int32_t, int32_t, const int32_t *, int32_t, const int32_t *, const uint32_t *,
                      const float *, int32_t, const float *, const float *, const float *, int32_t *, int32_t *, int32_t *, int32_t *, float *,
                      int32_t, int32_t *, int32_t *, void *, int64_t, cm3d_stream_t st)
{
    STAGE(st);
}
int cm3d_medoid2(const float *, const int32_t *, const int32_t *, int32_t, const int32_t *, const int32_t *, const int32_t *, int32_t,
                 const int32_t *, int32_t *, float *, float *, void *, int64_t, int32_t, int32_t *, cm3d_stream_t st)
{
    STAGE(st);
}
int cm3d_centroid_transform(const float *, const int32_t *, const int32_t *, int32_t, const float *, float *, cm3d_stream_t st) { STAGE(st); }
int cm3d_lane_nn(const float *, const int32_t *, const int32_t *, int32_t, const float *, const int32_t *, const int32_t *, int32_t, int32_t,
                 const void *, int32_t *, double *, void *, int64_t, cm3d_stream_t st)
{
    STAGE(st);
}
int cm3d_box_nms_bounded(const float *, const int32_t *, const int32_t *, int32_t, int32_t, const int32_t *, const double *, const float *,
                         const int32_t *, const int32_t *, const int32_t *, const double *, const double *, const int32_t *, const int32_t *,
                         const double *, int32_t, const double *, const float *, int32_t, double *, int32_t *, cm3d_stream_t st)
{
    STAGE(st);
}
int cm3d_obb(const float *, const int32_t *, int32_t, int32_t, double *, int32_t *, double *, uint8_t *, void *, int64_t, cm3d_stream_t st)
{
    STAGE(st);
}
}

static float g_f[4];
static const int kPlainCalls = 6;     // the steady-state nuScenes pass: masks with the reset, projection, compaction, medoid, lanes, boxes
static cm3d_stream_t g_streams[cm3d::kPipeMaxDepth];

static cm3d_lift_pass_desc plain_desc()
{
    static int32_t feedback = 1;
    cm3d_lift_pass_desc p;
    std::memset(&p, 0, sizeof p);
    p.size = (int64_t)sizeof p;
    p.raw = g_f, p.intensity = g_f, p.sweep_xf = g_f;
    p.fused = 1, p.planes = 1;
    p.md_feedback = &feedback;
    return p;
}

static void set_queues(int q)
{
    if (q > 0)
        setenv("GPU_MAX_HW_QUEUES", std::to_string(q).c_str(), 1);
    else
        unsetenv("GPU_MAX_HW_QUEUES");
}

static uintptr_t handle_of(int exec, int null_exec) { return exec == null_exec ? 0 : (uintptr_t)g_streams[exec]; }

static void check_plans()
{
    for (int depth = 1; depth <= 8; ++depth)
        for (int q = -2; q <= 64; ++q) {
            const cm3d::PipeExecPlan plan = cm3d::pipe_exec_plan(depth, q);
            const int old_n = cm3d::pipe_exec_streams(depth, q);
            const int most = depth < 4 ? depth : 4;
            const bool queue_limited = (q - 1 < 1 ? 1 : q - 1) < most;
            CHECK(plan.n_exec >= 1 && plan.n_exec <= most);
            CHECK(plan.null_last == queue_limited);            // a null executor only where the old policy stopped at the queues
            CHECK(plan.n_exec == old_n + (queue_limited ? 1 : 0));
            CHECK(!plan.null_last || plan.n_exec >= 2);
        }
    const int listed[][2] = {{4, 4}, {3, 4}, {4, 8}, {4, 2}, {1, 1}, {1, 4}, {1, 64}, {2, 4}, {8, 4}, {4, 1}, {4, 5}};
    for (const auto &dq : listed) {
        const cm3d::PipeExecPlan plan = cm3d::pipe_exec_plan(dq[0], dq[1]);
        std::printf("plan %d %d %d %d\n", dq[0], dq[1], plan.n_exec, (int)plan.null_last);
    }
    // the old policy, bit for bit
    CHECK(cm3d::pipe_exec_streams(4, 4) == 3 && cm3d_pipe_exec_streams_for(4, 4) == 3 && cm3d_pipe_exec_streams_for(4, 8) == 4);
}

static void check_create()
{
    set_queues(4);
    unsetenv("CM3D_PIPE_NULL_EXEC");
    struct Case { int depth, exec_streams, null_exec, want_n, want_null; bool old_create; };
    const Case cases[] = {
        {4, 0, 0, 3, -1, true},   {4, 4, 0, 4, -1, true},  {2, 0, 0, 2, -1, true},      // cm3d_pipe_create never makes one
        {4, 0, 0, 3, -1, false},  {4, 0, -1, 4, 3, false}, {3, 0, -1, 3, -1, false},    // the plan
        {4, 3, -1, 3, -1, false}, {4, 4, -1, 4, -1, false}, {4, 1, -1, 1, -1, false},   // an explicit count makes none
        {4, 0, 1, 4, 3, false},   {2, 0, 1, 2, 1, false},  {4, 2, 1, 2, 1, false},      // asked for: the last of at least two
        {1, 0, 1, 1, -1, false},  {4, 1, 1, 1, -1, false}, {3, 0, 1, 3, 2, false},
    };
    for (const Case &c : cases) {
        void *p = c.old_create ? cm3d_pipe_create(c.depth, c.exec_streams, g_streams) : cm3d_pipe_create2(c.depth, c.exec_streams, g_streams, c.null_exec);
        CHECK(p);
        CHECK(cm3d_pipe_exec_streams(p) == c.want_n);
        CHECK(cm3d_pipe_null_exec(p) == c.want_null);
        cm3d_pipe_destroy(p);
    }
    setenv("CM3D_PIPE_NULL_EXEC", "0", 1);          // switched off: the old plan where nothing is asked, an explicit request stands
    void *p = cm3d_pipe_create2(4, 0, g_streams, -1);
    CHECK(p && cm3d_pipe_exec_streams(p) == 3 && cm3d_pipe_null_exec(p) == -1);
    cm3d_pipe_destroy(p);
    p = cm3d_pipe_create2(4, 0, g_streams, 1);
    CHECK(p && cm3d_pipe_exec_streams(p) == 4 && cm3d_pipe_null_exec(p) == 3);
    cm3d_pipe_destroy(p);
    unsetenv("CM3D_PIPE_NULL_EXEC");
    set_queues(8);                                  // queues of its own for every executor: none
    p = cm3d_pipe_create2(4, 0, g_streams, -1);
    CHECK(p && cm3d_pipe_exec_streams(p) == 4 && cm3d_pipe_null_exec(p) == -1);
    cm3d_pipe_destroy(p);
    set_queues(0);                                  // unset: the runtime's four
    p = cm3d_pipe_create2(4, 0, g_streams, -1);
    CHECK(p && cm3d_pipe_exec_streams(p) == 4 && cm3d_pipe_null_exec(p) == 3);
    cm3d_pipe_destroy(p);
    CHECK(!cm3d_pipe_create2(4, 0, g_streams, 2) && !cm3d_pipe_create2(4, 0, g_streams, -2) && !cm3d_pipe_create2(4, 0, nullptr, -1));
    CHECK(!cm3d_pipe_create2(0, 0, g_streams, -1) && cm3d_pipe_null_exec(nullptr) == -1);
    std::printf("create ok\n");
}

// 13 round-robin passes: which executor each pass's calls received, where the slot's event was recorded and what was waited for
static void trace(int depth, int queues, int exec_streams = 0, int null_arg = -1)
{
    set_queues(queues);
    void *p = cm3d_pipe_create2(depth, exec_streams, g_streams, null_arg);
    CHECK(p);
    const cm3d::PipeExecPlan plan = cm3d::pipe_exec_plan(depth, queues);
    const int n_exec = cm3d_pipe_exec_streams(p), null_exec = cm3d_pipe_null_exec(p);
    if (exec_streams == 0)
        CHECK(n_exec == plan.n_exec && null_exec == (plan.null_last ? n_exec - 1 : -1));
    else
        CHECK(n_exec == exec_streams && null_exec == (null_arg == 1 ? n_exec - 1 : -1));
    int n_waits = 0;
    const cm3d_lift_pass_desc d = plain_desc();
    std::vector<int> last(depth, -1);
    std::vector<uintptr_t> done(depth, 0);
    for (int k = 0; k < 13; ++k) {
        const int slot = k % depth;
        g_log.clear();
        const int e = cm3d_pipe_submit(p, slot, &d);
        CHECK(e == (n_exec >= depth ? slot : k % n_exec));
        CHECK(cm3d_pipe_last_stream(p, slot) == e);
        const uintptr_t h = handle_of(e, null_exec);
        CHECK((h == 0) == (e == null_exec));                     // handle 0 for the null executor and nobody else
        const bool want_wait = last[slot] >= 0 && last[slot] != e;
        size_t i = 0;
        if (want_wait) {                                         // behind the slot's previous pass first, on the new executor
            CHECK(g_log[0].what == "wait" && g_log[0].stream == h && g_log[0].event == done[slot]);
            i = 1;
        }
        CHECK(g_log.size() == i + kPlainCalls + 1);
        for (size_t j = i; j < i + kPlainCalls; ++j) CHECK(g_log[j].what.rfind("cm3d_", 0) == 0 && g_log[j].stream == h);
        const Call &rec = g_log.back();                          // the slot's event on the executor that ran the pass
        CHECK(rec.what == "record" && rec.stream == h && rec.event != 0);
        CHECK(done[slot] == 0 || done[slot] == rec.event);
        done[slot] = rec.event;
        last[slot] = e;
        n_waits += want_wait;
        std::printf("pass %d %d %d %d %d %#lx %d\n", depth, exec_streams ? -exec_streams : queues, k, slot, e, (unsigned long)h, (int)want_wait);
    }
    CHECK((n_waits > 0) == (n_exec < depth && depth % n_exec != 0));
    // acquire / release and wait work on executors too
    g_log.clear();
    const int e = cm3d_pipe_acquire(p, 0);
    CHECK(e >= 0 && cm3d_pipe_release(p, 0) == CM3D_OK);
    CHECK(g_log.back().what == "record" && g_log.back().stream == handle_of(e, null_exec) && g_log.back().event == done[0]);
    g_log.clear();
    CHECK(cm3d_pipe_wait(p, 0) == CM3D_OK && g_log.size() == 1 && g_log[0].what == "sync" && g_log[0].event == done[0]);
    cm3d_pipe_destroy(p);
}

// a fired event is not waited for, on whichever executor
static void check_fired_events_are_not_waited_for()
{
    set_queues(2);
    void *p = cm3d_pipe_create2(4, 0, g_streams, -1);
    CHECK(p && cm3d_pipe_null_exec(p) == 1);
    const cm3d_lift_pass_desc d = plain_desc();
    g_events_pending = false;
    g_log.clear();
    for (int k = 0; k < 13; ++k) CHECK(cm3d_pipe_submit(p, k % 4, &d) == k % 2);
    for (const Call &c : g_log) CHECK(c.what != "wait");
    g_events_pending = true;
    cm3d_pipe_destroy(p);
}

// pin: the null executor ends, its slot goes to its own stream behind the pass the null stream ran
static void check_pin()
{
    set_queues(4);
    void *p = cm3d_pipe_create2(4, 0, g_streams, -1);
    CHECK(p && cm3d_pipe_null_exec(p) == 3);
    const cm3d_lift_pass_desc d = plain_desc();
    for (int k = 0; k < 4; ++k) CHECK(cm3d_pipe_submit(p, k, &d) == k);
    g_log.clear();
    CHECK(cm3d_pipe_pin(p) == CM3D_OK && cm3d_pipe_null_exec(p) == -1);
    CHECK(g_log.size() == 1 && g_log[0].what == "wait" && g_log[0].stream == (uintptr_t)g_streams[3] && g_log[0].event != 0);
    for (int k = 0; k < 8; ++k) {
        g_log.clear();
        CHECK(cm3d_pipe_submit(p, k % 4, &d) == k % 4);
        for (const Call &c : g_log) CHECK(c.what != "wait" && c.stream == (uintptr_t)g_streams[k % 4]);
    }
    g_log.clear();
    CHECK(cm3d_pipe_pin(p) == CM3D_OK && g_log.empty());         // again: nothing left to do
    cm3d_pipe_destroy(p);
    // two executors under four slots, pinned while slot 1's last pass sits on the null stream and slot 2's on streams[0]
    set_queues(2);
    p = cm3d_pipe_create2(4, 0, g_streams, -1);
    CHECK(p && cm3d_pipe_null_exec(p) == 1);
    for (int k = 0; k < 6; ++k) CHECK(cm3d_pipe_submit(p, k % 4, &d) == k % 2);      // slot 1: pass 5 on executor 1; slot 2: pass 2 on 0
    g_log.clear();
    CHECK(cm3d_pipe_pin(p) == CM3D_OK);
    CHECK(g_log.size() == 1 && g_log[0].what == "wait" && g_log[0].stream == (uintptr_t)g_streams[1]);
    g_log.clear();
    CHECK(cm3d_pipe_submit(p, 2, &d) == 2);                      // the scheduler's own wait: executor 0 -> streams[2]
    CHECK(g_log[0].what == "wait" && g_log[0].stream == (uintptr_t)g_streams[2]);
    g_log.clear();
    CHECK(cm3d_pipe_submit(p, 3, &d) == 3);                      // slot 3's pass 3 ran on the null stream as executor 1
    CHECK(g_log[0].what == "wait" && g_log[0].stream == (uintptr_t)g_streams[3]);
    for (const Call &c : g_log) CHECK(c.stream == (uintptr_t)g_streams[3]);
    cm3d_pipe_destroy(p);
    std::printf("pin ok\n");
}

// a pass of the null executor with each call in turn answering an error
static void check_errors()
{
    set_queues(2);                                   // depth 4 on streams[0] and the null stream: slot 1's second pass waits, then runs on the null stream
    const cm3d_lift_pass_desc d = plain_desc();
    const int n_positions = 1 + kPlainCalls + 1;     // the wait, the pass's calls, the record
    for (int pos = 0; pos < n_positions; ++pos) {
        void *p = cm3d_pipe_create2(4, 0, g_streams, -1);
        CHECK(p && cm3d_pipe_null_exec(p) == 1);
        g_fail_at = -1;
        for (int k = 0; k < 6; ++k) CHECK(cm3d_pipe_submit(p, k % 4, &d) == k % 2);
        CHECK(cm3d_pipe_submit(p, 1, &d) == 0);      // pass 6: slot 1 on executor 0, so that its next pass changes executor
        g_log.clear();
        g_fail_at = pos;
        const int rc = cm3d_pipe_submit(p, 1, &d);   // pass 7: slot 1 on the null executor, behind a wait
        g_fail_at = -1;
        CHECK(rc == CM3D_ERR_LAUNCH);
        CHECK((int)g_log.size() == (pos == 0 ? 1 : pos == n_positions - 1 ? n_positions : pos + 2));
        for (const Call &c : g_log) CHECK(c.stream == 0);        // all of it on the null stream
        const bool recorded = g_log.back().what == "record";
        CHECK(recorded == (pos > 0));                // behind whatever the pass did enqueue; a failed wait enqueues nothing
        std::printf("fail %d %d %d %d\n", pos, rc, (int)g_log.size(), (int)recorded);
        cm3d_pipe_destroy(p);
    }
}

int main()
{
    for (int i = 0; i < cm3d::kPipeMaxDepth; ++i) g_streams[i] = (cm3d_stream_t)(uintptr_t)(0x1000 + 0x10 * i);
    check_plans();
    check_create();
    trace(4, 4);
    trace(4, 2);
    trace(3, 4);
    trace(3, 4, 2, 1);      // three slots on streams[0] and the null stream: the slots change executor, so their events are waited for
    check_fired_events_are_not_waited_for();
    check_pin();
    check_errors();
    std::printf("pipe_null_exec_sim ok\n");
    return 0;
}
