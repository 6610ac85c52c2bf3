// Ground points stripped from the in-mask lists (opt-in): cm3d_ground_grid and cm3d_ground_strip of include/cm3d_hip.h, which states
// the rule; cm3d_amd/groundstrip.py is the host statement, to the bit.
//   k_ground_grid    one workgroup of GG_WAVES waves per (frame, tile of GG_TILE x GG_TILE cells).  The tile's 256 cells x 64 bins of
//                    int32 counters fill 64 KiB of LDS.  The workgroup streams the whole frame's rows -- the cloud's float4 rows, or the
//                    raw rows sweep by sweep through the row addressing, ego-box test and fma chains of k_box_ground (csrc/ground.hip)
//                    and k_sweep_xform (csrc/sweep.hip), GG_UNROLL rows of a thread in flight at once.  A point outside the tile's
//                    rectangle (a little wider than the rule's rounding can reach) costs two comparisons; a member of a cell of the
//                    tile does one integer LDS add (sums of ones: the counts do not depend on the order in which points arrive).
//                    Behind a barrier one wave per cell holds one bin per lane: a wave prefix sum gives n and the lane that owns rank
//                    k, which writes the cell's two outputs (lane 0 where the cell has no estimate).  A frame's rows are read once per
//                    tile, 16 times, from L2 after the first.
//   k_ground_strip   one workgroup per mask: one keep byte per list position (0: ground), the kept count behind a workgroup sum, the
//                    MIN_KEEP rule (the workgroup then sets its keep bytes again), gs_status and gs_dropped.
//   k_list_compact_scan / _scatter (csrc/list_compact.h, shared with cm3d_depth_cluster): gs_off, gs_tile_off and the stable compaction.
// Every offset read from device memory is clamped first: rows into [0, n_rows], sweeps into [0, n_sweeps], list positions into
// [0, idx_cap]; a frame number outside [0, n_frames) reads no grid.  Plain stores, no global atomic, no allocation, no read-back.
#include "common.h"
#include "list_compact.h"

#define GG_CELLS CM3D_GROUND_GRID_CELLS
#define GG_BINS CM3D_GROUND_GRID_BINS
#define GG_HALF (GG_CELLS / 2)
#define GG_TILE 16
#define GG_TILES (GG_CELLS / GG_TILE)
#define GG_WAVES 16
#define GG_THREADS (64 * GG_WAVES)
#define GG_UNROLL 4
static_assert(GG_BINS == 64, "the scan gives every lane of a wave one of the 64 counters");
static_assert(GG_CELLS % GG_TILE == 0 && GG_TILE * GG_TILE * GG_BINS * 4 == 65536, "a tile's counters are 64 KiB of LDS");

static __device__ __forceinline__ bool gg_finite(double v) { return fabs(v) < INFINITY; }      // (false for NaN)
static __device__ __forceinline__ int gg_clamp(int v, int lo, int hi) { return v < lo ? lo : (v > hi ? hi : v); }

struct GgCloud {                // as GrCloud of csrc/ground.hip
    const float4 *points; const int32_t *pt_off;                                       // the materialised cloud, or
    const float *raw; int raw_stride; const float *sweep_xf; const int32_t *sweep_row_off, *frame_sweep_off; int n_sweeps; float halfw;
    int n_rows;
};

struct GgTile {                 // what a workgroup knows of its tile, in registers
    double ox, oy, z0, cell, dz;
    double xmin, xmax, ymin, ymax;
    double iu0, iv0;            // the tile's first cell, as floor() gives it
};

// The cell of a point along one axis, as the rule states it: floor(((double)p - o) / C), inside the grid iff -32 <= . < 32.
static __device__ __forceinline__ double gg_cell(float p, double o, double c) { return floor(((double)p - o) / c); }

// one point of the frame against the tile
static __device__ __forceinline__ void gg_point(int *cnt, const GgTile &q, float px, float py, float pz)
{
    const double x = (double)px, y = (double)py;
    if (!(x >= q.xmin && x <= q.xmax && y >= q.ymin && y <= q.ymax)) return;          // (a NaN fails)
    const double iu = gg_cell(px, q.ox, q.cell) - q.iu0, iv = gg_cell(py, q.oy, q.cell) - q.iv0;          // (small integers: exact)
    if (!(iu >= 0.0 && iu < (double)GG_TILE && iv >= 0.0 && iv < (double)GG_TILE)) return;
    const double t = ((double)pz - q.z0) / q.dz;
    if (t >= 0.0 && t < (double)GG_BINS) atomicAdd(&cnt[((int)iv * GG_TILE + (int)iu) * GG_BINS + (int)t], 1);
}

// MODE 0: the cloud; 1: raw rows of raw_stride floats; 2: the quad layout
template <int MODE>
__global__ __launch_bounds__(GG_THREADS) void k_ground_grid(GgCloud c, const double *__restrict__ origin, int n_frames, double cell, double down,
                                                            double dz, double quantile, int min_points, double *__restrict__ grid_z,
                                                            int32_t *__restrict__ grid_n)
{
    __shared__ int s_cnt[GG_TILE * GG_TILE * GG_BINS];
    const int t = threadIdx.x, lane = cm3d_lane(), wave = t >> 6;
    const int f = blockIdx.x / (GG_TILES * GG_TILES), tile = blockIdx.x % (GG_TILES * GG_TILES);
    const int tu = (tile % GG_TILES) * GG_TILE, tv = (tile / GG_TILES) * GG_TILE;          // the tile's first cell, 0-based
    for (int i = t; i < GG_TILE * GG_TILE * GG_BINS; i += GG_THREADS) s_cnt[i] = 0;
    GgTile q;
    q.ox = origin[3 * (size_t)f], q.oy = origin[3 * (size_t)f + 1];
    const double oz = origin[3 * (size_t)f + 2];
    q.z0 = oz - down, q.cell = cell, q.dz = dz;
    q.iu0 = (double)(tu - GG_HALF), q.iv0 = (double)(tv - GG_HALF);
    const bool ok = gg_finite(q.ox) && gg_finite(q.oy) && gg_finite(oz);
    {   // the tile's rectangle, a little wider than the rounding of the subtraction and the division can reach
        const double x0 = q.ox + q.iu0 * cell, x1 = q.ox + (q.iu0 + (double)GG_TILE) * cell;
        const double y0 = q.oy + q.iv0 * cell, y1 = q.oy + (q.iv0 + (double)GG_TILE) * cell;
        const double ex = cell * 0x1p-20 + (fabs(x0) + fabs(x1)) * 0x1p-40, ey = cell * 0x1p-20 + (fabs(y0) + fabs(y1)) * 0x1p-40;
        q.xmin = x0 - ex, q.xmax = x1 + ex, q.ymin = y0 - ey, q.ymax = y1 + ey;
    }
    __syncthreads();
    if (ok) {                   // (the same in every thread)
        if (MODE == 0) {
            const int p0 = gg_clamp(c.pt_off[f], 0, c.n_rows), p1 = gg_clamp(c.pt_off[f + 1], p0, c.n_rows);
            for (int g0 = p0; g0 < p1; g0 += GG_UNROLL * GG_THREADS) {
                float4 p[GG_UNROLL];
#pragma unroll
                for (int u = 0; u < GG_UNROLL; ++u) {
                    const int g = g0 + u * GG_THREADS + t;
                    p[u] = g < p1 ? c.points[g] : make_float4(NAN, NAN, NAN, 0.f);
                }
#pragma unroll
                for (int u = 0; u < GG_UNROLL; ++u) gg_point(s_cnt, q, p[u].x, p[u].y, p[u].z);
            }
        } else {
            const int s0 = gg_clamp(c.frame_sweep_off[f], 0, c.n_sweeps), s1 = gg_clamp(c.frame_sweep_off[f + 1], s0, c.n_sweeps);
            for (int sw = s0; sw < s1; ++sw) {
                const float *const xf = c.sweep_xf + (size_t)sw * CM3D_SWEEP_XF_STRIDE;      // (uniform: scalar loads)
                const int r0 = gg_clamp(c.sweep_row_off[sw], 0, c.n_rows), r1 = gg_clamp(c.sweep_row_off[sw + 1], r0, c.n_rows);
                for (int g0 = r0; g0 < r1; g0 += GG_UNROLL * GG_THREADS) {
                    float x[GG_UNROLL], y[GG_UNROLL], z[GG_UNROLL];
#pragma unroll
                    for (int u = 0; u < GG_UNROLL; ++u) {
                        const int g = g0 + u * GG_THREADS + t;
                        x[u] = y[u] = z[u] = NAN;                    // (beyond the sweep: never dropped, never a member)
                        if (g < r1 && MODE == 2) {                   // quad layout: x, y, z of row g at 12 (g >> 2) + (g & 3) + 0 / 4 / 8
                            const float *p = c.raw + (size_t)(g >> 2) * 12 + (g & 3);
                            x[u] = p[0], y[u] = p[4], z[u] = p[8];
                        } else if (g < r1) {
                            const float *p = c.raw + (size_t)g * c.raw_stride;
                            x[u] = p[0], y[u] = p[1], z[u] = p[2];
                        }
                    }
#pragma unroll
                    for (int u = 0; u < GG_UNROLL; ++u) {
                        if (fabsf(x[u]) < c.halfw && fabsf(y[u]) < c.halfw) continue;      // the row the preparation drops
                        float ax, ay, az, bx, by, bz;
                        cm3d_rot3(xf, x[u], y[u], z[u], ax, ay, az);
                        ax = ax + xf[9]; ay = ay + xf[10]; az = az + xf[11];
                        cm3d_rot3(xf + 12, ax, ay, az, bx, by, bz);
                        bx = bx + xf[21]; by = by + xf[22]; bz = bz + xf[23];
                        gg_point(s_cnt, q, bx, by, bz);
                    }
                }
            }
        }
    }
    __syncthreads();
    for (int j = wave; j < GG_TILE * GG_TILE; j += GG_WAVES) {                    // (j is the same in every lane of the wave)
        const int cnt = s_cnt[j * GG_BINS + lane];
        const int incl = cm3d_wave_incl_scan(cnt), excl = incl - cnt;
        const int n = __builtin_amdgcn_readlane(incl, 63);
        const bool has = n >= min_points;                                         // (min_points >= 1: n >= 1, so k < n)
        const int k = has ? (int)(quantile * (double)(n - 1)) : 0;
        const bool mine = has ? (excl <= k && k < incl) : lane == 0;              // exactly one lane
        if (mine) {
            const size_t o = (size_t)f * (GG_CELLS * GG_CELLS) + (size_t)(tv + j / GG_TILE) * GG_CELLS + (size_t)(tu + j % GG_TILE);
            grid_z[o] = has ? q.z0 + (((double)lane + 0.5) * dz) : (double)NAN;
            grid_n[o] = n;
        }
    }
}

extern "C" int cm3d_ground_strip_check(double cell, double down, double up, double quantile, int32_t min_points, double margin,
                                       int32_t min_keep)
{
    if (!(cell > 0.0 && cell < INFINITY) || !(down > 0.0 && down < INFINITY) || !(up > 0.0 && up < INFINITY)) return CM3D_ERR_ARG;      // (a NaN fails)
    if (!(quantile >= 0.0 && quantile <= 1.0) || min_points < 1 || !(fabs(margin) < INFINITY) || min_keep < 1) return CM3D_ERR_ARG;
    return CM3D_OK;
}

extern "C" int cm3d_ground_grid(const float *points, const int32_t *pt_off, const float *raw, int32_t raw_stride, const float *sweep_xf,
                                const int32_t *sweep_row_off, const int32_t *frame_sweep_off, int32_t n_sweeps, float halfw, int32_t n_rows,
                                const double *origin, int32_t n_frames, double cell, double down, double up, double quantile,
                                int32_t min_points, double *grid_z, int32_t *grid_n, cm3d_stream_t stream)
{
    if (cm3d_ground_strip_check(cell, down, up, quantile, min_points, 0.0, 1) != CM3D_OK) return CM3D_ERR_ARG;
    if (n_frames < 0 || n_rows < 0 || n_sweeps < 0) return CM3D_ERR_ARG;
    const bool cloud = points && pt_off, rows = raw && sweep_xf && sweep_row_off && frame_sweep_off;
    if (!cloud && !rows) return CM3D_ERR_ARG;
    if (!cloud && raw_stride < 4 && raw_stride != CM3D_RAW_QUADS) return CM3D_ERR_ARG;
    if (cloud && ((uintptr_t)points & 15)) return CM3D_ERR_ARG;
    if (n_frames == 0) return CM3D_OK;
    if (!origin || !grid_z || !grid_n || (int64_t)n_frames * (GG_TILES * GG_TILES) > 0x7FFFFFFF) return CM3D_ERR_ARG;
    const GgCloud c{cloud ? (const float4 *)points : nullptr, pt_off, raw, raw_stride, sweep_xf, sweep_row_off, frame_sweep_off, n_sweeps,
                    halfw, n_rows};
    const double dz = (down + up) / (double)GG_BINS;
    const dim3 grid((unsigned)(n_frames * GG_TILES * GG_TILES)), block(GG_THREADS);
    hipStream_t st = (hipStream_t)stream;
    if (cloud)
        hipLaunchKernelGGL(k_ground_grid<0>, grid, block, 0, st, c, origin, n_frames, cell, down, dz, quantile, min_points, grid_z, grid_n);
    else if (raw_stride == CM3D_RAW_QUADS)
        hipLaunchKernelGGL(k_ground_grid<2>, grid, block, 0, st, c, origin, n_frames, cell, down, dz, quantile, min_points, grid_z, grid_n);
    else
        hipLaunchKernelGGL(k_ground_grid<1>, grid, block, 0, st, c, origin, n_frames, cell, down, dz, quantile, min_points, grid_z, grid_n);
    CM3D_CHECK_LAUNCH();
    return CM3D_OK;
}

// ---- the strip ----------------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(LC_THREADS) void k_ground_strip(const float4 *__restrict__ hit_xyz, const int32_t *__restrict__ hit_off,
                                                             const int32_t *__restrict__ mask_frame, int idx_cap,
                                                             const double *__restrict__ origin, const double *__restrict__ grid_z, int n_frames,
                                                             double cell, double margin, int min_keep, uint8_t *__restrict__ keep,
                                                             int32_t *__restrict__ count, int32_t *__restrict__ gs_status,
                                                             int32_t *__restrict__ gs_dropped)
{
    __shared__ int s_cnt[LC_WAVES];
    const int m = blockIdx.x, lane = cm3d_lane(), wave = threadIdx.x >> 6;
    const LcRange r = lc_range(hit_off, m, idx_cap);
    if (r.n == 0) {
        if (threadIdx.x == 0) count[m] = 0, gs_status[m] = 2, gs_dropped[m] = 0;
        return;
    }
    const int f = mask_frame[m];
    const bool fo = f >= 0 && f < n_frames;
    const double ox = fo ? origin[3 * (size_t)f] : (double)NAN, oy = fo ? origin[3 * (size_t)f + 1] : (double)NAN;
    const double *const gz = grid_z + (size_t)(fo ? f : 0) * (GG_CELLS * GG_CELLS);
    int kept = 0;
    for (long long i = threadIdx.x; i < r.n; i += LC_THREADS) {
        const float4 p = hit_xyz[r.lo + i];
        bool ground = false;
        if (fo) {
            const double iu = gg_cell(p.x, ox, cell), iv = gg_cell(p.y, oy, cell);          // (a NaN origin or coordinate: outside)
            if (iu >= -(double)GG_HALF && iu < (double)GG_HALF && iv >= -(double)GG_HALF && iv < (double)GG_HALF) {
                const double g = gz[((int)iv + GG_HALF) * GG_CELLS + ((int)iu + GG_HALF)];
                const double z = (double)p.z;
                ground = gg_finite(z) && z < g + margin;                                    // (a NaN g: no estimate, never ground)
            }
        }
        keep[r.lo + i] = ground ? 0 : 1;
        kept += ground ? 0 : 1;
    }
    kept = cm3d_wave_sum(kept);
    if (lane == 0) s_cnt[wave] = kept;
    __syncthreads();
    kept = 0;
#pragma unroll
    for (int w = 0; w < LC_WAVES; ++w) kept += s_cnt[w];
    const bool whole = kept < min_keep;
    if (whole)                  // the list is kept whole (every thread sets the bytes it wrote itself)
        for (long long i = threadIdx.x; i < r.n; i += LC_THREADS) keep[r.lo + i] = 1;
    if (threadIdx.x == 0) {
        count[m] = whole ? r.n : kept;
        gs_status[m] = whole ? 1 : 0;
        gs_dropped[m] = whole ? 0 : r.n - kept;
    }
}

extern "C" int64_t cm3d_ground_strip_workspace_bytes(int32_t n_masks, int32_t idx_cap)
{
    if (n_masks <= 0 || idx_cap <= 0) return 0;
    return 4 * (int64_t)n_masks + (int64_t)idx_cap;
}

extern "C" int cm3d_ground_strip(const float *hit_xyz, const int32_t *hit_idx, const int32_t *hit_off, const int32_t *mask_frame,
                                 int32_t n_masks, int32_t idx_cap, const double *origin, const double *grid_z, int32_t n_frames,
                                 double cell, double margin, int32_t min_keep, int32_t *gs_off, int32_t *gs_tile_off, int32_t *gs_idx,
                                 float *gs_xyz, int32_t *gs_status, int32_t *gs_dropped, void *workspace, int64_t workspace_bytes,
                                 cm3d_stream_t stream)
{
    if (cm3d_ground_strip_check(cell, 1.0, 1.0, 0.0, 1, margin, min_keep) != CM3D_OK) return CM3D_ERR_ARG;
    if (n_masks < 0 || idx_cap <= 0 || n_frames < 0) return CM3D_ERR_ARG;
    if ((hit_idx == nullptr) != (gs_idx == nullptr)) return CM3D_ERR_ARG;
    if (n_masks == 0) return CM3D_OK;
    if (!hit_xyz || !hit_off || !mask_frame || !gs_off || !gs_tile_off || !gs_xyz || !gs_status || !gs_dropped || !workspace) return CM3D_ERR_ARG;
    if (n_frames > 0 && (!origin || !grid_z)) return CM3D_ERR_ARG;
    if (((uintptr_t)hit_xyz & 15) || ((uintptr_t)gs_xyz & 15) || ((uintptr_t)workspace & 3)) return CM3D_ERR_ARG;
    if (workspace_bytes < cm3d_ground_strip_workspace_bytes(n_masks, idx_cap)) return CM3D_ERR_WORKSPACE;
    hipStream_t st = (hipStream_t)stream;
    // count i32[n_masks] | keep u8[idx_cap]
    int32_t *count = (int32_t *)workspace;
    uint8_t *keep = (uint8_t *)(count + n_masks);
    hipLaunchKernelGGL(k_ground_strip, dim3(n_masks), dim3(LC_THREADS), 0, st, (const float4 *)hit_xyz, hit_off, mask_frame, idx_cap, origin,
                       grid_z, n_frames, cell, margin, min_keep, keep, count, gs_status, gs_dropped);
    CM3D_CHECK_LAUNCH();
    hipLaunchKernelGGL(k_list_compact_scan, dim3(1), dim3(1024), 0, st, count, n_masks, gs_off, gs_tile_off);
    CM3D_CHECK_LAUNCH();
    hipLaunchKernelGGL(k_list_compact_scatter, dim3(n_masks), dim3(LC_THREADS), 0, st, (const float4 *)hit_xyz, hit_idx, hit_off, idx_cap,
                       keep, gs_off, gs_idx, (float4 *)gs_xyz);
    CM3D_CHECK_LAUNCH();
    return CM3D_OK;
}
