// Stand-alone simulation of cm3d_amd/csrc/pipe_sched.h (tests/test_pipe_sched_host.py builds it with the address and undefined-behaviour
// sanitizers and runs it): depth 1..8 x executing streams 1..8 x queue counts 1..32, three submit patterns.
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "pipe_sched.h"

static long long g_checks = 0;
#define REQUIRE(cond, ...)                                   \
    do {                                                     \
        ++g_checks;                                          \
        if (!(cond)) {                                       \
            std::fprintf(stderr, "FAILED %s: ", #cond);      \
            std::fprintf(stderr, __VA_ARGS__);               \
            std::fprintf(stderr, "\n");                      \
            std::exit(1);                                    \
        }                                                    \
    } while (0)

enum Pattern { ROUND_ROBIN, SLOT_ZERO, RANDOM };

static uint32_t lcg(uint32_t &s) { return s = s * 1664525u + 1013904223u; }

static void simulate(int depth, int n_exec_asked, Pattern pat, int pin_after)
{
    cm3d::PipeSched sch(depth, n_exec_asked);
    const int n_exec = sch.n_exec;
    REQUIRE(n_exec >= 1 && n_exec <= depth, "depth %d asked %d got %d", depth, n_exec_asked, n_exec);
    std::vector<int> prev(depth, -1), per_stream(depth, 0);
    uint32_t seed = 12345u + 97u * depth + 7u * n_exec_asked;
    const int n_pass = 13 * depth + 5;
    for (int k = 0; k < n_pass; ++k) {
        if (k == pin_after) sch.pin();
        const bool pinned = pin_after >= 0 && k >= pin_after;
        const int slot = pat == ROUND_ROBIN ? k % depth : pat == SLOT_ZERO ? 0 : (int)((lcg(seed) >> 8) % (uint32_t)depth);
        const cm3d::PipeTicket t = sch.next(slot);
        REQUIRE(t.stream >= 0 && t.stream < depth, "stream %d of %d", t.stream, depth);
        // (i) two consecutive passes of one slot: same stream, or the later one is told to wait
        REQUIRE(prev[slot] < 0 || prev[slot] == t.stream || t.wait, "depth %d exec %d pass %d slot %d: %d -> %d without a wait", depth, n_exec, k,
                slot, prev[slot], t.stream);
        REQUIRE(!(t.wait && (prev[slot] < 0 || prev[slot] == t.stream)), "a wait nobody needs (pass %d)", k);
        if (n_exec >= depth || pinned) REQUIRE(t.stream == slot, "slot %d on stream %d", slot, t.stream);
        // (iii) as many executing streams as slots: the slot's own stream, never a wait
        if (n_exec >= depth) REQUIRE(!t.wait, "wait with exec %d >= depth %d", n_exec, depth);
        if (n_exec < depth && !pinned) REQUIRE(t.stream < n_exec && t.stream == k % n_exec, "pass %d on stream %d of %d", k, t.stream, n_exec);
        REQUIRE(sch.last[slot] == t.stream, "last[%d]", slot);
        prev[slot] = t.stream;
        ++per_stream[t.stream];
    }
    // (ii) round robin: every executing stream carries its share
    if (pat == ROUND_ROBIN && pin_after < 0) {
        int lo = n_pass, hi = 0;
        for (int s = 0; s < n_exec; ++s) {
            lo = per_stream[s] < lo ? per_stream[s] : lo;
            hi = per_stream[s] > hi ? per_stream[s] : hi;
        }
        REQUIRE(hi - lo <= 1, "depth %d exec %d: %d..%d passes per stream", depth, n_exec, lo, hi);
        for (int s = n_exec; s < depth; ++s) REQUIRE(per_stream[s] == 0, "stream %d beyond the executing ones ran a pass", s);
    }
}

int main()
{
    // (iv) the policy
    REQUIRE(cm3d::pipe_exec_streams(4, 4) == 3, "(4, 4)");
    REQUIRE(cm3d::pipe_exec_streams(4, 8) == 4, "(4, 8)");
    REQUIRE(cm3d::pipe_exec_streams(8, 16) == 4, "(8, 16)");
    for (int q = -2; q <= 64; ++q) REQUIRE(cm3d::pipe_exec_streams(1, q) == 1, "(1, %d)", q);
    REQUIRE(cm3d::pipe_hw_queues(nullptr) == 4 && cm3d::pipe_hw_queues("") == 4 && cm3d::pipe_hw_queues("x") == 4 && cm3d::pipe_hw_queues("0") == 4,
            "unset or unusable GPU_MAX_HW_QUEUES");
    REQUIRE(cm3d::pipe_hw_queues("8") == 8 && cm3d::pipe_hw_queues("32") == 32 && cm3d::pipe_hw_queues("1") == 1, "GPU_MAX_HW_QUEUES values");
    for (int depth = 1; depth <= 8; ++depth)
        for (int e = 1; e <= 8; ++e)
            for (int q = 1; q <= 32; ++q) {
                const int pol = cm3d::pipe_exec_streams(depth, q);
                REQUIRE(pol >= 1 && pol <= depth && pol <= cm3d::kPipeMaxExecStreams && (pol <= q - 1 || pol == 1), "policy (%d, %d) = %d", depth, q, pol);
                for (int pat = ROUND_ROBIN; pat <= RANDOM; ++pat) {
                    simulate(depth, e, (Pattern)pat, -1);
                    simulate(depth, pol, (Pattern)pat, -1);
                    simulate(depth, e, (Pattern)pat, 2 * depth + 1);      // a graph capture pins the slots part-way
                }
            }
    std::printf("pipe_sched ok: %lld checks\n", g_checks);
    return 0;
}
