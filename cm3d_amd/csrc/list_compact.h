// Stable compaction of every mask's list by keep bytes, shared by the stages that drop points from the in-mask lists
// (csrc/cluster.hip: cm3d_depth_cluster; csrc/groundstrip.hip: cm3d_ground_strip).  A stage writes one keep byte per list position and
// the kept count of every mask; then
//   k_list_compact_scan     one workgroup: the offsets and the tile offsets of the kept lists
//   k_list_compact_scatter  one workgroup per mask: the kept entries in the list's own order (ballot + prefix)
// Every offset read from hit_off is clamped into [0, idx_cap] first (lc_range), and the scatter checks its destination: nothing at or
// beyond idx_cap is touched whatever the offsets hold.  The kernels have internal linkage: each file that includes this has its own.
#pragma once
#include "common.h"

#define LC_THREADS 256
#define LC_WAVES (LC_THREADS / CM3D_WAVE)

struct LcRange { int lo, n; };
static __device__ __forceinline__ LcRange lc_range(const int32_t *hit_off, int m, int idx_cap)
{
    int lo = hit_off[m], hi = hit_off[m + 1];
    lo = lo < 0 ? 0 : (lo > idx_cap ? idx_cap : lo);
    hi = hi < lo ? lo : (hi > idx_cap ? idx_cap : hi);
    return LcRange{lo, hi - lo};
}

static __global__ __launch_bounds__(1024) void k_list_compact_scan(const int32_t *count, int n_masks, int32_t *out_off, int32_t *out_tile_off)
{
    __shared__ int s_a[16], s_b[16];
    int base_o = 0, base_t = 0;
    for (long long m0 = 0; m0 < n_masks; m0 += 1024) {
        const long long m = m0 + threadIdx.x;
        const int c = m < n_masks ? count[m] : 0;
        int tot_o, tot_t;
        const int eo = cm3d_block1024_excl_scan(c, s_a, tot_o);
        const int et = cm3d_block1024_excl_scan((c + CM3D_MEDOID_TILE - 1) / CM3D_MEDOID_TILE, s_b, tot_t);
        if (m < n_masks) {
            out_off[m] = base_o + eo;
            out_tile_off[m] = base_t + et;
        }
        base_o += tot_o;
        base_t += tot_t;
    }
    if (threadIdx.x == 0) {
        out_off[n_masks] = base_o;
        out_tile_off[n_masks] = base_t;
    }
}

static __global__ __launch_bounds__(LC_THREADS) void k_list_compact_scatter(const float4 *hit_xyz, const int32_t *hit_idx, const int32_t *hit_off,
                                                                            int idx_cap, const uint8_t *keep, const int32_t *out_off,
                                                                            int32_t *out_idx, float4 *out_xyz)
{
    __shared__ int s_cnt[LC_WAVES];
    const int m = blockIdx.x, lane = cm3d_lane(), wave = threadIdx.x >> 6;
    const LcRange r = lc_range(hit_off, m, idx_cap);
    long long out = out_off[m];
    for (long long base = 0; base < r.n; base += LC_THREADS) {
        const long long i = base + threadIdx.x;
        const bool k = i < r.n && keep[r.lo + i] != 0;
        const uint64_t b = __ballot(k);
        if (lane == 0) s_cnt[wave] = __popcll(b);
        __syncthreads();
        int pre = 0, tot = 0;
#pragma unroll
        for (int w = 0; w < LC_WAVES; ++w) {
            const int c = s_cnt[w];
            if (w < wave) pre += c;
            tot += c;
        }
        if (k) {
            const long long d = out + pre + cm3d_mbcnt(b);
            if (d >= 0 && d < idx_cap) {                 // (offsets that describe more than exists: nothing lands out of range)
                out_xyz[d] = hit_xyz[r.lo + i];
                if (hit_idx) out_idx[d] = hit_idx[r.lo + i];
            }
        }
        out += tot;
        __syncthreads();
    }
}
