// Depth clustering of every mask's in-mask list (cm3d_depth_cluster, include/cm3d_hip.h states the semantics; host statement
// cm3d_amd/cluster.py): a 1-D gap clustering on the range from the frame's origin.  Three launches:
//   k_depth_cluster          one workgroup per mask: (range bits, position) keys, a bitonic sort -- in LDS up to
//                            CM3D_DEPTH_CLUSTER_LDS_POINTS points, in the workspace beyond --, then one wave walks the sorted ranges 64 at a
//                            time (ballot of the boundary flags, the segment that ends at each boundary, a wave-wide choice) and the
//                            workgroup writes one keep byte per list position and the kept count
//   k_list_compact_scan      one workgroup: cl_off, cl_tile_off                                                (csrc/list_compact.h,
//   k_list_compact_scatter   one workgroup per mask: stable compaction of hit_idx / hit_xyz by the keep bytes   shared with groundstrip.hip)
// Every offset read from hit_off is clamped into [0, idx_cap] first (lc_range), and the scatter checks its destination: nothing at or
// beyond idx_cap is touched whatever the offsets hold.  The keys are distinct (the position breaks ties), so the sorted order -- and
// with it every output byte -- is the same on every run.
#include "common.h"
#include "list_compact.h"

#define DC_THREADS 256
#define DC_WAVES (DC_THREADS / CM3D_WAVE)
#define DC_L CM3D_DEPTH_CLUSTER_LDS_POINTS

static_assert(DC_THREADS == LC_THREADS, "the scatter's workgroup is the clustering's");

// non-negative doubles order like their bit patterns
static __device__ __forceinline__ uint64_t dc_key(const float4 p, double ox, double oy, double oz)
{
    const double dx = (double)p.x - ox, dy = (double)p.y - oy, dz = (double)p.z - oz;
    const double r = sqrt((dx * dx + dy * dy) + dz * dz);
    return (uint64_t)__double_as_longlong(r);
}

static __device__ __forceinline__ void dc_cmpx(uint64_t *key, uint32_t *pos, long long i, long long j)
{
    const uint64_t a = key[i], b = key[j];
    const uint32_t pa = pos[i], pb = pos[j];
    if (a > b || (a == b && pa > pb)) {
        key[i] = b; key[j] = a;
        pos[i] = pb; pos[j] = pa;
    }
}

// Bitonic network in its one-direction form (per merge of width k: partner i ^ (k - 1), then i ^ j for j = k/4 .. 1): every
// comparator puts the smaller pair at the lower index, so the elements a power-of-two padding would add -- all larger than any key,
// all at the top -- never move, and a comparator whose upper end is >= n is simply left out.  Comparator t of a step is owned by
// thread t mod DC_THREADS; its lower end grows with t.
static __device__ __forceinline__ void dc_sort(uint64_t *key, uint32_t *pos, int n)
{
    for (int lk = 1; (1ll << (lk - 1)) < n; ++lk) {
        const int half = 1 << (lk - 1);
        for (long long t = threadIdx.x;; t += DC_THREADS) {
            const long long blk = (t >> (lk - 1)) << lk, off = t & (half - 1);
            if (blk + off >= n) break;
            const long long j = blk + (2ll * half - 1 - off);
            if (j < n) dc_cmpx(key, pos, blk + off, j);
        }
        __syncthreads();
        for (int lj = lk - 2; lj >= 0; --lj) {
            const int d = 1 << lj;
            for (long long t = threadIdx.x;; t += DC_THREADS) {
                const long long i = ((t >> lj) << (lj + 1)) + (t & (d - 1));
                if (i >= n) break;
                if (i + d < n) dc_cmpx(key, pos, i, i + d);
            }
            __syncthreads();
        }
    }
}

// a qualifying segment: larger w wins, then the smaller start (w = size for "largest", 1 for "nearest"; w == 0: none)
struct DcSeg { uint32_t w; uint32_t inv_start; int32_t size; };
static __device__ __forceinline__ DcSeg dc_better(DcSeg a, DcSeg b)
{
    return (b.w > a.w || (b.w == a.w && b.inv_start > a.inv_start)) ? b : a;
}
static __device__ __forceinline__ DcSeg dc_seg(int start, int size, int min_points, int pick, DcSeg best)
{
    if (size < min_points) return best;
    return dc_better(best, DcSeg{pick ? 1u : (uint32_t)size, 0xFFFFFFFFu - (uint32_t)start, size});
}

// One mask, its keys in `key` / `pos` (LDS or the workspace): fill, sort, choose, mark.  s_res: 2 ints of LDS.
static __device__ __forceinline__ void dc_mask(uint64_t *key, uint32_t *pos, const float4 *xyz, int n, double ox, double oy, double oz, double eps,
                                               int min_points, int pick, uint8_t *keep, int32_t *count, int32_t *status, int *s_res)
{
    for (long long i = threadIdx.x; i < n; i += DC_THREADS) {
        key[i] = dc_key(xyz[i], ox, oy, oz);
        pos[i] = (uint32_t)i;
    }
    __syncthreads();
    dc_sort(key, pos, n);
    if (threadIdx.x < CM3D_WAVE) {
        const int lane = threadIdx.x;
        int cur_start = 0;                       // start of the segment that is open at the chunk's first position (wave-uniform)
        DcSeg best = {0u, 0u, 0};
        for (long long base = 0; base < n; base += CM3D_WAVE) {
            const long long k = base + lane;
            bool flag = false;
            if (k > 0 && k < n) flag = __longlong_as_double((long long)key[k]) - __longlong_as_double((long long)key[k - 1]) > eps;
            const uint64_t b = __ballot(flag);
            if (flag) {                          // the segment that ends in front of k starts at the boundary before it
                const uint64_t below = b & ((1ull << lane) - 1ull);
                const int ps = below ? (int)base + 63 - __clzll((long long)below) : cur_start;
                best = dc_seg(ps, (int)k - ps, min_points, pick, best);
            }
            if (b) cur_start = (int)base + 63 - __clzll((long long)b);
        }
        if (lane == 0) best = dc_seg(cur_start, n - cur_start, min_points, pick, best);
        best = cm3d_wave_reduce_t(best, [](DcSeg a, DcSeg b) { return dc_better(a, b); });
        if (lane == 0) {
            const int cs = best.w ? (int)(0xFFFFFFFFu - best.inv_start) : 0;
            s_res[0] = cs;
            s_res[1] = best.w ? cs + best.size : n;
            *count = best.w ? best.size : n;
            *status = best.w ? 0 : 1;
        }
    }
    __syncthreads();
    const int cs = s_res[0], ce = s_res[1];
    // (every position stands once in `pos`: each keep byte is written once)
    for (long long k = threadIdx.x; k < n; k += DC_THREADS) keep[pos[k]] = (k >= cs && k < ce) ? 1 : 0;
}

__global__ __launch_bounds__(DC_THREADS) void k_depth_cluster(const float4 *hit_xyz, const int32_t *hit_off, const int32_t *mask_frame,
                                                              int idx_cap, const double *origin, int n_frames, double eps, int min_points,
                                                              int pick, uint64_t *g_key, uint32_t *g_pos, uint8_t *keep, int32_t *count,
                                                              int32_t *cl_status)
{
    __shared__ uint64_t s_key[DC_L];
    __shared__ uint32_t s_pos[DC_L];
    __shared__ int s_res[2];
    const int m = blockIdx.x;
    const LcRange r = lc_range(hit_off, m, idx_cap);
    if (r.n == 0) {
        if (threadIdx.x == 0) {
            count[m] = 0;
            cl_status[m] = 2;
        }
        return;
    }
    const int f = mask_frame[m];
    const bool fo = f >= 0 && f < n_frames;
    const double ox = fo ? origin[3 * (long long)f] : 0.0, oy = fo ? origin[3 * (long long)f + 1] : 0.0, oz = fo ? origin[3 * (long long)f + 2] : 0.0;
    if (r.n <= DC_L)
        dc_mask(s_key, s_pos, hit_xyz + r.lo, r.n, ox, oy, oz, eps, min_points, pick, keep + r.lo, count + m, cl_status + m, s_res);
    else
        dc_mask(g_key + r.lo, g_pos + r.lo, hit_xyz + r.lo, r.n, ox, oy, oz, eps, min_points, pick, keep + r.lo, count + m, cl_status + m,
                s_res);
}

extern "C" int64_t cm3d_depth_cluster_workspace_bytes(int32_t n_masks, int32_t idx_cap)
{
    if (n_masks <= 0 || idx_cap <= 0) return 0;
    return 13 * (int64_t)idx_cap + 4 * (int64_t)n_masks;
}

extern "C" int cm3d_depth_cluster(const float *hit_xyz, const int32_t *hit_idx, const int32_t *hit_off, const int32_t *mask_frame,
                                  int32_t n_masks, int32_t idx_cap, const double *origin, int32_t n_frames, double eps, int32_t min_points,
                                  int32_t pick, int32_t *cl_off, int32_t *cl_tile_off, int32_t *cl_idx, float *cl_xyz, int32_t *cl_status,
                                  void *workspace, int64_t workspace_bytes, cm3d_stream_t stream)
{
    if (!hit_xyz || !hit_off || !mask_frame || !origin || !cl_off || !cl_tile_off || !cl_xyz || !cl_status || !workspace) return CM3D_ERR_ARG;
    if ((hit_idx == nullptr) != (cl_idx == nullptr)) return CM3D_ERR_ARG;
    if (n_masks <= 0 || idx_cap <= 0 || n_frames <= 0) return CM3D_ERR_ARG;
    if (!(eps > 0.0) || min_points < 1 || (pick != 0 && pick != 1)) return CM3D_ERR_ARG;          // (a NaN eps fails the comparison)
    if (((uintptr_t)workspace & 7) != 0) return CM3D_ERR_ARG;
    if (workspace_bytes < cm3d_depth_cluster_workspace_bytes(n_masks, idx_cap)) return CM3D_ERR_WORKSPACE;
    hipStream_t st = (hipStream_t)stream;
    // key u64[idx_cap] | pos u32[idx_cap] | count i32[n_masks] | keep u8[idx_cap]
    uint64_t *g_key = (uint64_t *)workspace;
    uint32_t *g_pos = (uint32_t *)(g_key + idx_cap);
    int32_t *count = (int32_t *)(g_pos + idx_cap);
    uint8_t *keep = (uint8_t *)(count + n_masks);
    hipLaunchKernelGGL(k_depth_cluster, dim3(n_masks), dim3(DC_THREADS), 0, st, (const float4 *)hit_xyz, hit_off, mask_frame, idx_cap, origin,
                       n_frames, eps, min_points, pick, g_key, g_pos, keep, count, cl_status);
    CM3D_CHECK_LAUNCH();
    hipLaunchKernelGGL(k_list_compact_scan, dim3(1), dim3(1024), 0, st, count, n_masks, cl_off, cl_tile_off);
    CM3D_CHECK_LAUNCH();
    hipLaunchKernelGGL(k_list_compact_scatter, dim3(n_masks), dim3(DC_THREADS), 0, st, (const float4 *)hit_xyz, hit_idx, hit_off, idx_cap,
                       keep, cl_off, cl_idx, (float4 *)cl_xyz);
    CM3D_CHECK_LAUNCH();
    return CM3D_OK;
}
