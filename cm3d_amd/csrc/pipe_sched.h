// Which stream the next pass of a LiftPipeline slot goes to (cm3d_amd/csrc/pipeline.cpp; DESIGN.md, "Passes rotate over as many
// streams as the process has queues for").  Plain C++17, no HIP: the policy compiles and runs on a CPU (tests/test_pipe_sched_host.py).
#ifndef CM3D_PIPE_SCHED_H
#define CM3D_PIPE_SCHED_H

#include <cstdlib>

namespace cm3d {

// DESIGN.md, "Four batches in flight": four streams on four pipes of their own is the optimum; five and more executing streams are
// slower again on any number of queues.
constexpr int kPipeMaxExecStreams = 4;
// hardware queues a process gets when GPU_MAX_HW_QUEUES is not set (the HIP runtime's default)
constexpr int kPipeDefaultHwQueues = 4;
constexpr int kPipeMaxDepth = 64;

// GPU_MAX_HW_QUEUES as the runtime reads it (text, may be NULL): read only, never set here.
inline int pipe_hw_queues(const char *env_value)
{
    if (!env_value || !*env_value) return kPipeDefaultHwQueues;
    char *end = nullptr;
    long v = std::strtol(env_value, &end, 10);
    if (end == env_value || v < 1) return kPipeDefaultHwQueues;
    return v > 1024 ? 1024 : (int)v;
}

// Streams that execute passes at the same time: no more than batches in flight, than the chip has pipes for, or than the process has
// queues for -- less one, the queue the null stream and everything else in the process share.
inline int pipe_exec_streams(int depth, int hw_queues)
{
    int n = hw_queues - 1;
    if (n < 1) n = 1;
    if (n > kPipeMaxExecStreams) n = kPipeMaxExecStreams;
    if (n > depth) n = depth;
    return n < 1 ? 1 : n;
}

// The executors of a pipeline: streams that execute passes at the same time, the last of which may be the legacy null stream.
struct PipeExecPlan {
    int n_exec;
    bool null_last;   // executor n_exec - 1 is the null stream, not one of the pipeline's own
};

// The null stream has a queue to itself that carries nothing while passes run ("A fourth batch on the null stream's
// queue").  Where pipe_exec_streams stops at the queues -- not at the batches in flight or at the four pipes -- that queue takes one
// more executor; everywhere else the plan is pipe_exec_streams' own.
inline PipeExecPlan pipe_exec_plan(int depth, int hw_queues)
{
    PipeExecPlan plan = {pipe_exec_streams(depth, hw_queues), false};
    const int by_queues = hw_queues - 1 < 1 ? 1 : hw_queues - 1;
    const int by_rest = depth < kPipeMaxExecStreams ? (depth < 1 ? 1 : depth) : kPipeMaxExecStreams;
    if (by_queues < by_rest) {
        plan.n_exec += 1;
        plan.null_last = true;
    }
    return plan;
}

struct PipeTicket {
    int stream;   // index into the pipeline's streams
    bool wait;    // the slot's previous pass ran on another stream: order this one behind it first
};

// Hands out streams.  With n_exec >= depth slot s owns stream s (no cross-stream order is ever needed).  With fewer executing streams
// than slots, pass number k goes to stream k % n_exec whichever slot it belongs to: under round-robin submission every stream gets every
// n_exec-th pass and the slots take turns on them.
struct PipeSched {
    int depth = 1;
    int n_exec = 1;
    bool pinned = false;          // pin(): slot s stays on stream s from now on
    long long passes = 0;
    int last[kPipeMaxDepth];      // stream of the slot's last pass, -1: none yet

    PipeSched(int depth_, int n_exec_)
    {
        depth = depth_ < 1 ? 1 : (depth_ > kPipeMaxDepth ? kPipeMaxDepth : depth_);
        n_exec = n_exec_ < 1 ? 1 : (n_exec_ > depth ? depth : n_exec_);
        for (int i = 0; i < kPipeMaxDepth; ++i) last[i] = -1;
    }

    bool rotating() const { return !pinned && n_exec < depth; }

    // something outside the scheduler runs the slots on their own streams (a captured graph replays where it was captured)
    void pin() { pinned = true; }

    PipeTicket next(int slot)
    {
        PipeTicket t;
        t.stream = rotating() ? (int)(passes % n_exec) : slot;
        t.wait = last[slot] >= 0 && last[slot] != t.stream;
        last[slot] = t.stream;
        ++passes;
        return t;
    }
};

}  // namespace cm3d
#endif
