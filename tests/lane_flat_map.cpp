// Stand-alone check of the flat scan's index arithmetic (cm3d_amd/csrc/lane_flat.h), which k_lane_nn_grid uses to deal the points of a
// ring batch's segments to the lanes of a wave: for every flat position of a vector of 64 (or five) segment ranges, the sorted-table
// index the map gives must be the one a linear walk over the segments reaches.  Random and crafted length vectors.  Prints
// "lane_flat_map ok" and the number of positions checked.
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "lane_flat.h"

static long g_checked = 0;

struct Seg { int a, b; };

// the wave's arithmetic on host arrays: inclusive sums, bases, then the map for every position below the total, in rounds of 64
// positions per lane exactly as the kernel steps through them (p0, p0 + 64, ... inside blocks of 64 * LF_ROUNDS)
static bool check(const std::vector<Seg> &seg, bool first, const char *what)
{
    std::vector<int> incl(64), base(64);
    int run = 0;
    for (int s = 0; s < 64; ++s) {
        const int len = s < (int)seg.size() ? seg[s].b - seg[s].a : 0, a = s < (int)seg.size() ? seg[s].a : 0;
        base[s] = a - run;
        run += len;
        incl[s] = run;
    }
    const int T = incl[63];
    std::vector<int> walk;
    for (const Seg &g : seg)
        for (int q = g.a; q < g.b; ++q) walk.push_back(q);
    if ((int)walk.size() != T) { std::printf("%s: total %d, walk %zu\n", what, T, walk.size()); return false; }
    std::vector<char> seen(T > 0 ? T : 1, 0);
    for (int p0 = 0; p0 < T; p0 += 64 * LF_ROUNDS)
        for (int v = 0; v < LF_ROUNDS; ++v)
            for (int lane = 0; lane < 64; ++lane) {
                const int raw = p0 + v * 64 + lane;
                const int p = raw < T - 1 ? raw : T - 1;             // the kernel's clamp: a dead position reads the last point
                int probes = 0, q;
                if (first) q = p + lf_pick5(p, incl[0], incl[1], incl[2], incl[3], base[0], base[1], base[2], base[3], base[4]);
                else {
                    const int s = lf_segment(p, [&](int l) {
                        if (l < 0 || l > 63) { std::printf("%s: probe at lane %d\n", what, l); std::exit(1); }
                        ++probes;
                        return incl[l];
                    });
                    if (probes != 6 || s < 0 || s > 63) { std::printf("%s: %d probes, segment %d\n", what, probes, s); return false; }
                    q = p + base[s];
                }
                if (q != walk[p]) { std::printf("%s: position %d -> %d, the walk says %d\n", what, p, q, walk[p]); return false; }
                if (raw < T) { seen[raw] = 1; ++g_checked; }
            }
    for (int p = 0; p < T; ++p)
        if (!seen[p]) { std::printf("%s: position %d never visited\n", what, p); return false; }
    return true;
}

// segments with the given lengths, laid out in a table with gaps between them (so that a wrong segment gives a wrong index)
static std::vector<Seg> lay(const std::vector<int> &len, uint32_t &rng)
{
    std::vector<Seg> seg;
    int at = 1000;
    for (int l : len) {
        rng = rng * 1664525u + 1013904223u;
        at += (int)((rng >> 24) % 7);
        seg.push_back({at, at + l});
        at += l;
    }
    return seg;
}

int main()
{
    uint32_t rng = 12345u;
    bool ok = true;
    auto both = [&](std::vector<int> len, const char *what) {
        ok = ok && check(lay(len, rng), false, what);
        if (len.size() <= 5) ok = ok && check(lay(len, rng), true, what);
    };
    both({}, "all empty");
    both({0, 0, 0, 0, 0}, "five empty");
    both(std::vector<int>(64, 0), "64 empty");
    both({1}, "one of 1");
    both({0, 0, 1}, "one of 1 behind empties");
    both({0, 0, 0, 0, 1}, "one of 1 in the last of five");
    for (int l : {12, 13, 63, 64, 65, 127, 128, 129, 255, 256, 257, 600}) {
        both({l}, "one segment");
        both({0, l, 0}, "one segment between empties");
        both({l, 1}, "segment and 1");
        both({1, l}, "1 and segment");
        std::vector<int> last(64, 0);
        last[63] = l;
        both(last, "segment in lane 63");
    }
    both(std::vector<int>(64, 1), "64 live of 1");
    both(std::vector<int>(64, 4), "64 live of 4: 256");
    {
        std::vector<int> v(64, 4);
        v[17] = 3; both(v, "255 over 64");
        v[17] = 5; both(v, "257 over 64");
        v[0] = 0; v[63] = 0; both(v, "64 with empty ends");
    }
    for (int T : {63, 64, 65, 128, 129, 255, 256, 257, 600}) {          // totals over five segments, cut at every place of the first
        for (int c = 0; c <= T; c += (T > 130 ? 37 : 1)) both({c, 0, T - c, 0, 0}, "total in two of five");
        both({T / 5, T / 5, T / 5, T / 5, T - 4 * (T / 5)}, "total in five");
    }
    for (int it = 0; it < 3000 && ok; ++it) {
        rng = rng * 1664525u + 1013904223u;
        const int n = it % 3 == 0 ? 5 : 1 + (int)((rng >> 16) % 64);
        const int kind = (int)((rng >> 8) % 4);
        std::vector<int> len(n);
        for (int &l : len) {
            rng = rng * 1664525u + 1013904223u;
            const uint32_t r = rng >> 12;
            l = kind == 0 ? (int)(r % 3) : kind == 1 ? (int)(r % 20) : kind == 2 ? ((r % 5) ? 0 : (int)(r % 90)) : (int)(r % 130);
        }
        both(len, "random");
    }
    if (!ok) return 1;
    std::printf("lane_flat_map ok: %ld positions\n", g_checked);
    return 0;
}
