// Ground height under each box from the frame's own sweep (opt-in): cm3d_box_ground of include/cm3d_hip.h, which states the rule;
// cm3d_amd/boxground.py is the host statement, to the bit.  The first stage behind the projection that looks at a point outside a
// mask, so the first new pass over the sweep rows: a streaming kernel.
//   k_box_ground   one workgroup of GR_WAVES waves per (frame, chunk of the frame's masks).  A chunk holds up to GR_CHUNK masks; the
//                  launch takes smaller chunks (down to GR_MIN_CHUNK) while that gives the chip more workgroups, up to GR_TARGET_WGS
//                  (cm3d_box_ground_chunk): a workgroup's time is the mask loop's, points times masks; the rows it streams are cheap beside it.
//     setup        thread j < chunk holds mask j of the chunk: centre, z0 and reference height into LDS (a mask with a non-finite
//                  centre or reference height gets a NaN centre: no point is its member); every thread then folds the chunk's
//                  centres into the bounding rectangle of their circles, kept in registers.
//     stream       the workgroup reads the frame's rows once: the cloud's float4 rows, or the raw rows sweep by sweep through the very
//                  row addressing, ego-box test and fma chains of k_sweep_xform (csrc/sweep.hip) with the sweep's transform uniform,
//                  GR_UNROLL rows of a thread in flight at once.  A point outside the rectangle skips the mask loop; a member
//                  does one integer LDS add into its mask's row of the GR_CHUNK x CM3D_GROUND_BINS counter table (sums of ones:
//                  the counts do not depend on the order in which points arrive).
//     scan + apply one wave per mask, two bins per lane: a wave prefix sum over the 128 counters gives n and the lane whose bins hold
//                  rank k; that lane applies the rule and writes the mask's outputs (lane 0 where there is no ground).
// Every offset read from device memory is clamped first: rows into [0, n_rows], sweeps into [0, n_sweeps], masks into [0, n_masks];
// nothing outside the arrays' stated sizes is read or written.  Plain stores, no global atomic, no workspace, no allocation.
#include "common.h"

#define GR_WAVES 16
#define GR_THREADS (64 * GR_WAVES)
#define GR_CHUNK CM3D_GROUND_CHUNK
#define GR_BINS CM3D_GROUND_BINS
#define GR_UNROLL 4
#define GR_TARGET_WGS 256                       // workgroups the launch tries to give the chip before a chunk stays whole: one per CU
#define GR_MIN_CHUNK 8
static_assert(GR_BINS == 128, "the scan gives every lane of a wave two of the 128 counters");
static_assert(GR_CHUNK <= GR_THREADS, "one thread per mask of the chunk in the setup");

static __device__ __forceinline__ bool gr_finite(double v) { return fabs(v) < INFINITY; }      // (false for NaN)
static __device__ __forceinline__ int gr_clamp(int v, int lo, int hi) { return v < lo ? lo : (v > hi ? hi : v); }

struct GrCloud {
    const float4 *points; const int32_t *pt_off;                                       // the materialised cloud, or
    const float *raw; int raw_stride; const float *sweep_xf; const int32_t *sweep_row_off, *frame_sweep_off; int n_sweeps; float halfw;
    int n_rows;
};

struct GrOut {
    double *box;
    const int32_t *flags;
    const double *prior_wlh;
    int n_classes;
    const double *zref;
    const int32_t *vert_status; const double *vert_z, *vert_h;
    double lo, hi, up;
    double *ground_z; int32_t *ground_n; double *ground_h; int32_t *ground_src, *ground_status; double *ground_zref;
};

struct GrChunk {                // LDS of a workgroup
    int cnt[GR_CHUNK * GR_BINS];
    double cx[GR_CHUNK], cy[GR_CHUNK], z0[GR_CHUNK], zr[GR_CHUNK];
    int bad[GR_CHUNK];
};

struct GrRect { double xmin, xmax, ymin, ymax; };

// one point of the frame against the chunk's masks
static __device__ __forceinline__ void gr_point(GrChunk &s, const GrRect &q, int nm, double rr, double dz, float px, float py, float pz)
{
    const double x = (double)px, y = (double)py;
    if (!(x >= q.xmin && x <= q.xmax && y >= q.ymin && y <= q.ymax)) return;          // (a NaN fails)
    const double z = (double)pz;
    for (int j = 0; j < nm; ++j) {
        const double dx = x - s.cx[j], dy = y - s.cy[j];
        if (dx * dx + dy * dy <= rr) {
            const double t = (z - s.z0[j]) / dz;
            if (t >= 0.0 && t < (double)GR_BINS) atomicAdd(&s.cnt[j * GR_BINS + (int)t], 1);
        }
    }
}

// the lane that holds a mask's ground: the status, n and the ground out, then the rule's table
static __device__ __forceinline__ void gr_apply(const GrOut &o, int m, int status, int n, double g, double zr)
{
    double *const b = o.box + (size_t)m * CM3D_BOX_STRIDE;
    const int fl = o.flags[m];
    const double b8 = b[8];
    const int cls = b8 >= 0.0 && b8 < (double)o.n_classes ? (int)b8 : 0;               // what cm3d_box_vertical reads of the record
    const double h0 = o.prior_wlh[3 * cls + 2];
    const bool has_v = o.vert_status != nullptr;
    double h = has_v ? o.vert_h[m] : h0;
    int src = 0;
    if ((fl & 1) && status == 0 && gr_finite(h0) && h0 > 0.0) {
        if (has_v && o.vert_status[m] == 0) {
            const double ext = o.vert_z[2 * (size_t)m + 1] - g, r = ext / h0;
            if (r >= o.lo && r <= o.hi) {
                src = 1, h = ext;
                b[2] = g + (ext * 0.5);
            }
        }
        if (src == 0 && zr - g <= h0 + o.up) {
            src = 2, h = h0;
            b[2] = g + (h0 * 0.5);
        }
    }
    o.ground_status[m] = status;
    o.ground_n[m] = n;
    o.ground_z[m] = g;
    o.ground_h[m] = h;
    o.ground_src[m] = src;
    o.ground_zref[m] = zr;
}

// MODE 0: the cloud; 1: raw rows of raw_stride floats; 2: the quad layout
template <int MODE>
__global__ __launch_bounds__(GR_THREADS) void k_box_ground(GrCloud c, const int32_t *__restrict__ mask_off, int n_frames, int n_masks,
                                                           int chunk, int chunks, double radius, double quantile, int min_points, double down,
                                                           double dz, GrOut o)
{
    __shared__ GrChunk s;
    const int t = threadIdx.x, lane = cm3d_lane(), wave = t >> 6;
    const int f = blockIdx.x / chunks;
    const int m0 = gr_clamp(mask_off[f], 0, n_masks), m1 = gr_clamp(mask_off[f + 1], m0, n_masks);
    const double rr = radius * radius;
    for (int base = m0 + (blockIdx.x % chunks) * chunk; base < m1; base += chunks * chunk) {
        const int nm = min(chunk, m1 - base);
        for (int i = t; i < nm * GR_BINS; i += GR_THREADS) s.cnt[i] = 0;
        if (t < nm) {
            const int m = base + t;
            const double cx = o.box[(size_t)m * CM3D_BOX_STRIDE], cy = o.box[(size_t)m * CM3D_BOX_STRIDE + 1];
            const double zr = o.zref ? o.zref[m] : o.box[(size_t)m * CM3D_BOX_STRIDE + 2];
            const bool ok = gr_finite(cx) && gr_finite(cy) && gr_finite(zr);
            s.cx[t] = ok ? cx : (double)NAN, s.cy[t] = ok ? cy : (double)NAN;
            s.z0[t] = zr - down, s.zr[t] = zr, s.bad[t] = !ok;
        }
        __syncthreads();
        // the rectangle around the chunk's circles, a little wider than the rule's rounding can reach: a point outside it is no member
        GrRect q{INFINITY, -INFINITY, INFINITY, -INFINITY};
        for (int j = 0; j < nm; ++j) {
            const double cx = s.cx[j], cy = s.cy[j];
            if (cx == cx) {
                const double ex = radius + (radius * 0x1p-20 + fabs(cx) * 0x1p-40), ey = radius + (radius * 0x1p-20 + fabs(cy) * 0x1p-40);
                q.xmin = fmin(q.xmin, cx - ex), q.xmax = fmax(q.xmax, cx + ex);
                q.ymin = fmin(q.ymin, cy - ey), q.ymax = fmax(q.ymax, cy + ey);
            }
        }
        if (q.xmin <= q.xmax) {                    // (the same in every thread)
            if (MODE == 0) {
                const int p0 = gr_clamp(c.pt_off[f], 0, c.n_rows), p1 = gr_clamp(c.pt_off[f + 1], p0, c.n_rows);
                for (int g0 = p0; g0 < p1; g0 += GR_UNROLL * GR_THREADS) {
                    float4 p[GR_UNROLL];
#pragma unroll
                    for (int u = 0; u < GR_UNROLL; ++u) {
                        const int g = g0 + u * GR_THREADS + t;
                        p[u] = g < p1 ? c.points[g] : make_float4(NAN, NAN, NAN, 0.f);
                    }
#pragma unroll
                    for (int u = 0; u < GR_UNROLL; ++u) gr_point(s, q, nm, rr, dz, p[u].x, p[u].y, p[u].z);
                }
            } else {
                const int s0 = gr_clamp(c.frame_sweep_off[f], 0, c.n_sweeps), s1 = gr_clamp(c.frame_sweep_off[f + 1], s0, c.n_sweeps);
                for (int sw = s0; sw < s1; ++sw) {
                    const float *const xf = c.sweep_xf + (size_t)sw * CM3D_SWEEP_XF_STRIDE;      // (uniform: scalar loads)
                    const int r0 = gr_clamp(c.sweep_row_off[sw], 0, c.n_rows), r1 = gr_clamp(c.sweep_row_off[sw + 1], r0, c.n_rows);
                    for (int g0 = r0; g0 < r1; g0 += GR_UNROLL * GR_THREADS) {
                        float x[GR_UNROLL], y[GR_UNROLL], z[GR_UNROLL];
#pragma unroll
                        for (int u = 0; u < GR_UNROLL; ++u) {
                            const int g = g0 + u * GR_THREADS + t;
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
                        for (int u = 0; u < GR_UNROLL; ++u) {
                            if (fabsf(x[u]) < c.halfw && fabsf(y[u]) < c.halfw) continue;      // the row the preparation drops
                            float ax, ay, az, bx, by, bz;
                            cm3d_rot3(xf, x[u], y[u], z[u], ax, ay, az);
                            ax = ax + xf[9]; ay = ay + xf[10]; az = az + xf[11];
                            cm3d_rot3(xf + 12, ax, ay, az, bx, by, bz);
                            bx = bx + xf[21]; by = by + xf[22]; bz = bz + xf[23];
                            gr_point(s, q, nm, rr, dz, bx, by, bz);
                        }
                    }
                }
            }
        }
        __syncthreads();
        for (int j = wave; j < nm; j += GR_WAVES) {                    // (j is the same in every lane of the wave)
            const int c0 = s.cnt[j * GR_BINS + 2 * lane], c1 = s.cnt[j * GR_BINS + 2 * lane + 1];
            const int incl = cm3d_wave_incl_scan(c0 + c1), excl = incl - (c0 + c1);
            const int n = __builtin_amdgcn_readlane(incl, 63);
            const int status = s.bad[j] ? 4 : n == 0 ? 2 : n < min_points ? 1 : 0;
            const int k = status == 0 ? (int)(quantile * (double)(n - 1)) : 0;
            const bool mine = status == 0 ? (excl <= k && k < incl) : lane == 0;       // exactly one lane: k < n
            if (mine) {
                const int bin = 2 * lane + (excl + c0 > k ? 0 : 1);
                const double g = status == 0 ? s.z0[j] + (((double)bin + 0.5) * dz) : 0.0;
                gr_apply(o, base + j, status, status == 4 ? 0 : n, g, s.zr[j]);
            }
        }
        __syncthreads();
    }
}

// the masks of a workgroup for a batch of n_frames frames of at most max_masks_per_frame masks (what the launch takes)
extern "C" int32_t cm3d_box_ground_chunk(int32_t n_frames, int32_t max_masks_per_frame)
{
    if (n_frames <= 0 || max_masks_per_frame <= GR_MIN_CHUNK) return max_masks_per_frame > 0 ? GR_MIN_CHUNK : GR_CHUNK;
    const int64_t most = ((int64_t)max_masks_per_frame + GR_MIN_CHUNK - 1) / GR_MIN_CHUNK;
    int64_t per_frame = (GR_TARGET_WGS + (int64_t)n_frames - 1) / n_frames;
    per_frame = per_frame < 1 ? 1 : (per_frame > most ? most : per_frame);
    const int64_t chunk = ((int64_t)max_masks_per_frame + per_frame - 1) / per_frame;
    return (int32_t)(chunk < GR_MIN_CHUNK ? GR_MIN_CHUNK : (chunk > GR_CHUNK ? GR_CHUNK : chunk));
}

extern "C" int cm3d_box_ground(const float *points, const int32_t *pt_off, const float *raw, int32_t raw_stride, const float *sweep_xf,
                               const int32_t *sweep_row_off, const int32_t *frame_sweep_off, int32_t n_sweeps, float halfw, int32_t n_rows,
                               const int32_t *mask_off, int32_t n_frames, int32_t n_masks, int32_t max_masks_per_frame, double *box,
                               const int32_t *flags, const double *prior_wlh, int32_t n_classes, const double *zref,
                               const int32_t *vert_status, const double *vert_z, const double *vert_h, double radius, double quantile,
                               int32_t min_points, double down, double up, double lo, double hi, double *ground_z, int32_t *ground_n,
                               double *ground_h, int32_t *ground_src, int32_t *ground_status, double *ground_zref, cm3d_stream_t stream)
{
    if (!(radius > 0.0 && radius < INFINITY) || !(quantile >= 0.0 && quantile <= 1.0) || min_points < 1) return CM3D_ERR_ARG;      // (a NaN fails)
    if (!(down > 0.0 && down < INFINITY && up >= 0.0 && up < INFINITY) || !(lo > 0.0 && lo <= hi && hi < INFINITY)) return CM3D_ERR_ARG;
    if (n_masks < 0 || n_frames < 0 || n_rows < 0 || n_sweeps < 0 || n_classes < 0 || max_masks_per_frame < 0) return CM3D_ERR_ARG;
    const bool cloud = points && pt_off, rows = raw && sweep_xf && sweep_row_off && frame_sweep_off;
    if (!cloud && !rows) return CM3D_ERR_ARG;
    if (!cloud && raw_stride < 4 && raw_stride != CM3D_RAW_QUADS) return CM3D_ERR_ARG;
    if (cloud && ((uintptr_t)points & 15)) return CM3D_ERR_ARG;
    if (n_masks == 0) return CM3D_OK;
    if (n_classes == 0 || n_frames == 0 || !mask_off || !box || !flags || !prior_wlh || !ground_z || !ground_n || !ground_h || !ground_src ||
        !ground_status || !ground_zref)
        return CM3D_ERR_ARG;
    if ((vert_status || vert_z || vert_h) && !(vert_status && vert_z && vert_h)) return CM3D_ERR_ARG;
    const int chunk = cm3d_box_ground_chunk(n_frames, max_masks_per_frame);
    const int chunks = max_masks_per_frame <= chunk ? 1 : (int)(((int64_t)max_masks_per_frame + chunk - 1) / chunk);
    if ((int64_t)chunks * n_frames > 0x7FFFFFFF) return CM3D_ERR_ARG;
    const GrCloud c{cloud ? (const float4 *)points : nullptr, pt_off, raw, raw_stride, sweep_xf, sweep_row_off, frame_sweep_off, n_sweeps,
                    halfw, n_rows};
    const GrOut o{box, flags, prior_wlh, n_classes, zref, vert_status, vert_z, vert_h, lo, hi, up, ground_z, ground_n, ground_h, ground_src,
                  ground_status, ground_zref};
    const double dz = (down + up) / (double)GR_BINS;
    const dim3 grid((unsigned)(chunks * n_frames)), block(GR_THREADS);
    hipStream_t st = (hipStream_t)stream;
    if (cloud)
        hipLaunchKernelGGL(k_box_ground<0>, grid, block, 0, st, c, mask_off, n_frames, n_masks, chunk, chunks, radius, quantile, min_points, down, dz, o);
    else if (raw_stride == CM3D_RAW_QUADS)
        hipLaunchKernelGGL(k_box_ground<2>, grid, block, 0, st, c, mask_off, n_frames, n_masks, chunk, chunks, radius, quantile, min_points, down, dz, o);
    else
        hipLaunchKernelGGL(k_box_ground<1>, grid, block, 0, st, c, mask_off, n_frames, n_masks, chunk, chunks, radius, quantile, min_points, down, dz, o);
    CM3D_CHECK_LAUNCH();
    return CM3D_OK;
}
