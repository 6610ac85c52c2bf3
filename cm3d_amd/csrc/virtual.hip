// Virtual points from each mask (opt-in): cm3d_hit_project and cm3d_virtual_points of include/cm3d_hip.h, which states the rule;
// cm3d_amd/virtualpoints.py is the host statement, to the bit.  Pixels sampled inside every eroded mask take the depth of the nearest
// in-mask return in the image and are unprojected through the mask's own camera, float64.
//   k_hit_project     one thread per list position; its mask by a search of the offsets; the camera's float32 chain for one point --
//                     what project_pair of project.hip evaluates for two, with the true division -- and (u, v, depth, 0) out.
//   k_virtual_points  one workgroup of VP_WAVES waves per mask.
//     (a) rows        every thread counts a run of consecutive rows of the eroded bounds, a block scan makes the row prefix in LDS: A.
//     (b) select      a wave per sample: the rank's row by a search of the prefix, the row's words 64 at a time through a wave scan,
//                     the bit inside the word.
//     (c) nearest     the same wave: an argmin over the list, a lane's own candidates in ascending position under strict <, then
//                     the lexicographic (d2, position) minimum across the lanes: the first minimum.  (u, v) of a list of up to
//                     VP_LDS_LIST positions is staged in LDS once; a longer list is read from memory by every sample.
//     (d) write       the samples' keep flags are scanned in ascending j, a thread per four samples; the kept ones are unprojected
//                     in float64 (no contraction: the library is compiled with -ffp-contract=off) and stored without holes.
// Nothing outside a mask's slot of `packed` is read, whatever bbox holds (vp_rect); every offset is clamped into [0, idx_cap] first.
// Plain stores, no global atomic, no allocation; rows behind a mask's count are never written.
#include "common.h"

#define VP_WAVES 4
#define VP_THREADS (64 * VP_WAVES)
#define VP_MAX_K CM3D_VP_MAX_K
#define VP_MAX_ROWS CM3D_VP_MAX_ROWS
#define VP_LDS_LIST CM3D_VP_LDS_LIST
#define VP_PROJECT_BLOCKS 2048                   // k_hit_project's grid at most: eight workgroups of 256 a CU
static_assert(VP_MAX_K == 4 * VP_THREADS, "the write phase gives every thread four consecutive samples");
static_assert(VP_MAX_ROWS % VP_THREADS == 0, "the row phase gives every thread a run of rows");

struct VpRange { int lo, n; };
static __device__ __forceinline__ VpRange vp_range(const int32_t *off, int m, int idx_cap)
{
    int lo = off[m], hi = off[m + 1];
    lo = lo < 0 ? 0 : (lo > idx_cap ? idx_cap : lo);
    hi = hi < lo ? lo : (hi > idx_cap ? idx_cap : hi);
    return VpRange{lo, hi - lo};
}

// The camera's float32 chain for one point (include/cm3d_hip.h, cm3d_project_hits: `cams`): stages with optional t_pre / t_post,
// k-sequential fmaf (cm3d_rot3), then the K' rows with the trailing fmaf(0, 1, acc), then IEEE division.  depth is the last stage's z.
static __device__ __forceinline__ void vp_chain(const float *cm, float x, float y, float z, float &u, float &v, float &depth)
{
    const int ns = (int)cm[54], fl = (int)cm[55];
#pragma unroll
    for (int s = 0; s < 3; ++s) {
        if (s < ns) {
            const float *st = cm + 15 * s;
            if (fl & (1 << (2 * s))) { x = x + st[0]; y = y + st[1]; z = z + st[2]; }
            cm3d_rot3(st + 3, x, y, z, x, y, z);
            if (fl & (2 << (2 * s))) { x = x + st[12]; y = y + st[13]; z = z + st[14]; }
        }
    }
    depth = z;
    const float *K = cm + 45;
    float uh = K[0] * x; uh = fmaf(K[1], y, uh); uh = fmaf(K[2], z, uh); uh = fmaf(0.0f, 1.0f, uh);
    float vh = K[3] * x; vh = fmaf(K[4], y, vh); vh = fmaf(K[5], z, vh); vh = fmaf(0.0f, 1.0f, vh);
    float zh = K[6] * x; zh = fmaf(K[7], y, zh); zh = fmaf(K[8], z, zh); zh = fmaf(0.0f, 1.0f, zh);
    u = uh / zh;
    v = vh / zh;
}

__global__ __launch_bounds__(256) void k_hit_project(const float *__restrict__ xyz, const int32_t *__restrict__ off,
                                                     const int32_t *__restrict__ mask_frame, const int32_t *__restrict__ mask_cam,
                                                     const float *__restrict__ cams, int n_cams, int n_frames, int n_masks, int idx_cap,
                                                     float *__restrict__ hit_uvd)
{
    // the positions below the last offset, clamped: the host does not know how many there are (idx_cap is the buffers' capacity, many
    // times the lists), so the grid is bounded and walks them
    int end = off[n_masks];
    end = end < 0 ? 0 : (end > idx_cap ? idx_cap : end);
    for (long long pl = (long long)blockIdx.x * 256 + threadIdx.x; pl < end; pl += (long long)gridDim.x * 256) {
        const int p = (int)pl;
        // the last mask whose offset is <= p (the offsets ascend: cm3d_compact_hits and the stages behind it write them so)
        int lo = 0, hi = n_masks;                // off[lo] <= p is not known yet; the answer lies in [lo, hi)
        if (off[0] > p) continue;
        while (hi - lo > 1) {
            const int mid = (lo + hi) >> 1;
            if (off[mid] <= p) lo = mid; else hi = mid;
        }
        const int m = lo;
        const VpRange r = vp_range(off, m, idx_cap);
        if (p < r.lo || p >= r.lo + r.n) continue;   // offsets that do not ascend: not a position of mask m
        const int f = mask_frame[m], c = mask_cam[m];
        if (f < 0 || f >= n_frames || c < 0 || c >= n_cams) continue;
        const float *cm = cams + ((size_t)f * n_cams + c) * CM3D_CAM_STRIDE;
        const float4 q = *reinterpret_cast<const float4 *>(xyz + (size_t)p * 4);
        float u, v, d;
        vp_chain(cm, q.x, q.y, q.z, u, v, d);
        *reinterpret_cast<float4 *>(hit_uvd + (size_t)p * 4) = make_float4(u, v, d, 0.0f);
    }
}

extern "C" int cm3d_hit_project(const float *xyz, const int32_t *off, const int32_t *mask_frame, const int32_t *mask_cam, const float *cams,
                                int32_t n_cams, int32_t n_frames, int32_t n_masks, int32_t idx_cap, float *hit_uvd, cm3d_stream_t stream)
{
    if (n_masks < 0 || idx_cap < 0 || n_frames < 0 || n_cams < 0 || n_cams > CM3D_MAX_CAMS) return CM3D_ERR_ARG;
    if (n_masks == 0 || idx_cap == 0) return CM3D_OK;
    if (!xyz || !off || !mask_frame || !mask_cam || !cams || !hit_uvd || n_frames == 0 || n_cams == 0) return CM3D_ERR_ARG;
    if (((uintptr_t)xyz & 15) || ((uintptr_t)hit_uvd & 15)) return CM3D_ERR_ARG;
    const int blocks = (idx_cap + 255) / 256;
    hipLaunchKernelGGL(k_hit_project, dim3(blocks < VP_PROJECT_BLOCKS ? blocks : VP_PROJECT_BLOCKS), dim3(256), 0, (hipStream_t)stream, xyz, off, mask_frame, mask_cam, cams,
                       n_cams, n_frames, n_masks, idx_cap, hit_uvd);
    CM3D_CHECK_LAUNCH();
    return CM3D_OK;
}

static __device__ __forceinline__ uint32_t vp_mix(uint32_t x)
{
    x ^= x >> 16; x *= 0x7FEB352Du; x ^= x >> 15; x *= 0x846CA68Bu; x ^= x >> 16;
    return x;
}

static __device__ __forceinline__ bool vp_finite(double v) { return fabs(v) < INFINITY; }      // (false for NaN)

// The eroded bounds of a mask and where its rows lie in `packed`: valid only when every word of the bounds lies inside the stored
// rectangle and the stored rectangle inside the mask's slot.
struct VpRect {
    int x0, y0, x1, y1;          // eroded bounds, inclusive
    int w0, nw;                  // first word column of the bounds, word columns
    int stride;                  // words per stored row
    long long base;              // word of `packed` that holds word column w0 of row y0
    bool ok;
};
static __device__ __forceinline__ VpRect vp_rect(const int32_t *bbox, int m, int W, int H)
{
    const int32_t *b = bbox + (size_t)m * CM3D_BBOX_STRIDE;
    VpRect r;
    r.x0 = b[0], r.y0 = b[1], r.x1 = b[2], r.y1 = b[3];
    const int xw0 = b[4], ys = b[5], wc = b[6], rows = b[7];
    const int Wp = (W + 31) >> 5;
    r.w0 = r.x0 >> 5, r.nw = (r.x1 >> 5) - r.w0 + 1, r.stride = wc;
    r.ok = r.x0 >= 0 && r.x0 <= r.x1 && r.x1 < W && r.y0 >= 0 && r.y0 <= r.y1 && r.y1 < H &&           // (an empty mask has x0 > x1)
           xw0 >= 0 && wc >= 1 && xw0 + wc <= Wp && ys >= 0 && rows >= 1 && ys + rows <= H &&         // rows * wc <= H * Wp: inside the slot
           r.w0 >= xw0 && (r.x1 >> 5) < xw0 + wc && r.y0 >= ys && r.y1 < ys + rows;
    r.base = (long long)m * H * Wp + (long long)(r.ok ? r.y0 - ys : 0) * wc + (r.ok ? r.w0 - xw0 : 0);
    return r;
}
// word column w0 + i of row y0 + row, bits outside [x0, x1] cleared
static __device__ __forceinline__ uint32_t vp_word(const uint32_t *packed, const VpRect &r, int row, int i)
{
    uint32_t w = packed[r.base + (long long)row * r.stride + i];
    if (i == 0) w &= 0xFFFFFFFFu << (r.x0 & 31);
    if (i == r.nw - 1) w &= 0xFFFFFFFFu >> (31 - (r.x1 & 31));
    return w;
}

struct VpArgs {
    const uint32_t *packed;
    const int32_t *bbox;
    const float *cams;
    const int32_t *mask_off, *mask_frame, *mask_cam, *flags;
    const float *hit_uvd;
    const int32_t *off;
    const uint32_t *frame_seed;
    int W, H, n_cams, n_frames, n_masks, idx_cap, K;
    uint32_t seed;
    double max_px;
    int kept_only;
    int32_t *vp_count, *vp_status;
    double *vp_xyz;
    int32_t *vp_pix, *vp_src;
    float *vp_depth, *vp_d2;
};

__global__ __launch_bounds__(VP_THREADS) void k_virtual_points(VpArgs a)
{
    __shared__ int s_pre[VP_MAX_ROWS + 1];       // set pixels in the rows before row r of the eroded bounds
    __shared__ float2 s_uv[VP_LDS_LIST];
    __shared__ int s_px[VP_MAX_K], s_py[VP_MAX_K], s_src[VP_MAX_K];
    __shared__ float s_d2[VP_MAX_K];
    __shared__ int s_part[VP_WAVES];
    const int t = threadIdx.x, lane = cm3d_lane(), wave = t >> 6;
    const int m = blockIdx.x;

    // ---- what decides about the whole mask (the same in every thread: each branch below that holds a barrier is taken by all)
    const int f = a.mask_frame[m], c = a.mask_cam[m];
    const bool cam_there = f >= 0 && f < a.n_frames && c >= 0 && c < a.n_cams;
    const float *cm = a.cams + ((size_t)(cam_there ? f : 0) * a.n_cams + (cam_there ? c : 0)) * CM3D_CAM_STRIDE;
    const int ns = (int)cm[54], fl = (int)cm[55];
    const float *Kf = cm + 45;
    const double K00 = (double)Kf[0], K01 = (double)Kf[1], K02 = (double)Kf[2], K11 = (double)Kf[4], K12 = (double)Kf[5];
    const bool cam_ok = cam_there && ns >= 0 && ns <= 3 && Kf[3] == 0.0f && Kf[6] == 0.0f && Kf[7] == 0.0f && Kf[8] == 1.0f &&
                        vp_finite(K00) && K00 != 0.0 && vp_finite(K11) && K11 != 0.0;
    const VpRange lr = vp_range(a.off, m, a.idx_cap);
    const int n = lr.n;
    const VpRect rc = vp_rect(a.bbox, m, a.W, a.H);
    const int rows = rc.ok ? rc.y1 - rc.y0 + 1 : 0;
    int status = 0;
    if (a.kept_only && (a.flags[m] & 3) != 3) status = 1;
    else if (!cam_ok) status = 4;
    else if (n == 0 || rows == 0) status = 2;
    if (status != 0) {
        if (t == 0) a.vp_status[m] = status, a.vp_count[m] = 0;
        return;
    }

    // ---- (a) the row prefix: thread t counts rows [t * rpt, (t + 1) * rpt) of the bounds
    const int rpt = (rows + VP_THREADS - 1) / VP_THREADS;
    {
        int sum = 0;
        for (int q = 0; q < rpt; ++q) {
            const int r = t * rpt + q;
            if (r < rows) {
                int pc = 0;
                for (int i = 0; i < rc.nw; ++i) pc += __popc(vp_word(a.packed, rc, r, i));
                sum += pc;
                s_pre[r + 1] = sum;              // inclusive inside the thread's run; the runs before it are added below
            }
        }
        const int inc = cm3d_wave_incl_scan(sum);
        if (lane == 63) s_part[wave] = inc;
        __syncthreads();
        int before = inc - sum;
        for (int w = 0; w < wave; ++w) before += s_part[w];
        for (int q = 0; q < rpt; ++q) {
            const int r = t * rpt + q;
            if (r < rows) s_pre[r + 1] += before;
        }
        if (t == 0) s_pre[0] = 0;
    }
    const bool staged = n <= VP_LDS_LIST;
    if (staged)
        for (int i = t; i < n; i += VP_THREADS) {
            const float2 uv = *reinterpret_cast<const float2 *>(a.hit_uvd + (size_t)(lr.lo + i) * 4);
            s_uv[i] = uv;
        }
    __syncthreads();
    const int A = s_pre[rows];
    if (A == 0) {
        if (t == 0) a.vp_status[m] = 2, a.vp_count[m] = 0;
        return;
    }
    const int k = a.K < A ? a.K : A;
    const uint32_t kk = (uint32_t)(m - a.mask_off[f]);
    const uint32_t h0 = a.seed ^ (a.frame_seed[f] * 0x9E3779B1u) ^ (kk * 0x85EBCA77u);
    const bool limited = a.max_px > 0.0;
    const double max2 = a.max_px * a.max_px;

    // ---- (b) + (c): a wave per sample
    for (int j = wave; j < k; j += VP_WAVES) {
        const uint64_t lo = (uint64_t)j * (uint64_t)A / (uint64_t)k, hi = (uint64_t)(j + 1) * (uint64_t)A / (uint64_t)k;
        const uint32_t w = (uint32_t)(hi - lo);
        const uint32_t h = vp_mix(h0 ^ ((uint32_t)j * 0xC2B2AE3Du));
        const int rank = (int)(lo + (uint64_t)(h % w));
        // the last row r with s_pre[r] <= rank
        int r0 = 0, r1 = rows;
        while (r1 - r0 > 1) {
            const int mid = (r0 + r1) >> 1;
            if (s_pre[mid] <= rank) r0 = mid; else r1 = mid;
        }
        int rem = rank - s_pre[r0];              // 0-based rank inside the row
        int px = -1;
        for (int base = 0; base < rc.nw; base += 64) {
            const int i = base + lane;
            const uint32_t word = i < rc.nw ? vp_word(a.packed, rc, r0, i) : 0u;
            const int pc = __popc(word);
            const int inc = cm3d_wave_incl_scan(pc);
            const int tot = __builtin_amdgcn_readlane(inc, 63);
            if (rem < tot) {
                const int L = (int)__builtin_ctzll(__ballot(inc > rem));
                uint32_t wv = (uint32_t)__shfl((int)word, L);
                int nth = rem - (__shfl(inc, L) - __shfl(pc, L));
                for (int q = 0; q < nth; ++q) wv &= wv - 1u;
                px = ((rc.w0 + base + L) << 5) + (int)__builtin_ctz(wv);
                break;
            }
            rem -= tot;
        }
        const int py = rc.y0 + r0;
        const float cx = (float)px + 0.5f, cy = (float)py + 0.5f;
        // the nearest list position in the image: the first least d2 under strict <, a NaN never wins
        float best = INFINITY;
        int bi = 0x7FFFFFFF;
        for (int i = lane; i < n; i += 64) {
            float2 uv;
            if (staged) uv = s_uv[i];
            else uv = *reinterpret_cast<const float2 *>(a.hit_uvd + (size_t)(lr.lo + i) * 4);
            const float du = uv.x - cx, dv = uv.y - cy;
            const float d2 = fmaf(dv, dv, du * du);
            if (d2 == d2 && (bi == 0x7FFFFFFF || d2 < best)) best = d2, bi = i;
        }
        const Cm3dValIdx win = cm3d_wave_argmin_f(best, bi);          // (equal d2: the lower position; a lane without a candidate loses to any)
        bool keep = win.j != 0x7FFFFFFF;
        if (keep && limited && (double)win.s > max2) keep = false;
        if (lane == 0) s_px[j] = px, s_py[j] = py, s_src[j] = keep ? win.j : -1, s_d2[j] = win.s;
    }
    __syncthreads();

    // ---- (d) the kept samples in ascending j, without holes: thread t has samples 4t .. 4t + 3
    int cnt = 0;
#pragma unroll
    for (int q = 0; q < 4; ++q) {
        const int j = 4 * t + q;
        cnt += (j < k && s_src[j] >= 0) ? 1 : 0;
    }
    const int inc = cm3d_wave_incl_scan(cnt);
    if (lane == 63) s_part[wave] = inc;
    __syncthreads();
    int pos = inc - cnt, total = 0;
    for (int w = 0; w < VP_WAVES; ++w) {
        if (w < wave) pos += s_part[w];
        total += s_part[w];
    }
    if (t == 0) a.vp_status[m] = 0, a.vp_count[m] = total;
    for (int q = 0; q < 4; ++q) {
        const int j = 4 * t + q;
        if (j >= k || s_src[j] < 0) continue;
        const int src = s_src[j], px = s_px[j], py = s_py[j];
        const float depth = a.hit_uvd[(size_t)(lr.lo + src) * 4 + 2];
        const double cx = (double)((float)px + 0.5f), cy = (double)((float)py + 0.5f), d = (double)depth;
        double y = ((cy - K12) * d) / K11;
        double x = (((cx - K02) * d) - K01 * y) / K00;
        double z = d;
        for (int s = 2; s >= 0; --s) {
            if (s >= ns) continue;
            const float *st = cm + 15 * s;
            if (fl & (2 << (2 * s))) { x = x - (double)st[12]; y = y - (double)st[13]; z = z - (double)st[14]; }
            const float *R = st + 3;
            const double ox = ((double)R[0] * x + (double)R[3] * y) + (double)R[6] * z;
            const double oy = ((double)R[1] * x + (double)R[4] * y) + (double)R[7] * z;
            const double oz = ((double)R[2] * x + (double)R[5] * y) + (double)R[8] * z;
            x = ox, y = oy, z = oz;
            if (fl & (1 << (2 * s))) { x = x - (double)st[0]; y = y - (double)st[1]; z = z - (double)st[2]; }
        }
        const size_t row = (size_t)m * a.K + pos;
        a.vp_xyz[3 * row] = x, a.vp_xyz[3 * row + 1] = y, a.vp_xyz[3 * row + 2] = z;
        a.vp_pix[2 * row] = px, a.vp_pix[2 * row + 1] = py;
        a.vp_src[row] = src;
        a.vp_depth[row] = depth;
        a.vp_d2[row] = s_d2[j];
        ++pos;
    }
}

extern "C" int cm3d_virtual_points_check(int32_t per_mask, double max_px)
{
    if (per_mask < 1 || per_mask > CM3D_VP_MAX_K) return CM3D_ERR_ARG;
    if (!(max_px >= 0.0 && max_px < INFINITY)) return CM3D_ERR_ARG;                               // (a NaN fails)
    return CM3D_OK;
}

extern "C" int cm3d_virtual_points(const uint32_t *packed, const int32_t *bbox, int32_t W, int32_t H, const float *cams, int32_t n_cams,
                                   const int32_t *mask_off, const int32_t *mask_frame, const int32_t *mask_cam, const int32_t *flags,
                                   int32_t n_frames, int32_t n_masks, const float *hit_uvd, const int32_t *off, int32_t idx_cap,
                                   int32_t per_mask, uint32_t seed, double max_px, int32_t kept_only, const uint32_t *frame_seed,
                                   int32_t *vp_count, int32_t *vp_status, double *vp_xyz, int32_t *vp_pix, int32_t *vp_src, float *vp_depth,
                                   float *vp_d2, cm3d_stream_t stream)
{
    if (cm3d_virtual_points_check(per_mask, max_px) != CM3D_OK) return CM3D_ERR_ARG;
    if (n_masks < 0 || idx_cap < 0 || n_frames < 0 || n_cams < 0 || n_cams > CM3D_MAX_CAMS) return CM3D_ERR_ARG;
    if (W < 1 || H < 1 || H > CM3D_VP_MAX_ROWS || (int64_t)n_masks * H * ((W + 31) / 32) > 0x7FFFFFFFll) return CM3D_ERR_ARG;
    if (n_masks == 0) return CM3D_OK;
    if (!packed || !bbox || !cams || !mask_off || !mask_frame || !mask_cam || (kept_only && !flags) || (!hit_uvd && idx_cap > 0) || !off ||
        !frame_seed || !vp_count || !vp_status || !vp_xyz || !vp_pix || !vp_src || !vp_depth || !vp_d2 || n_frames == 0 || n_cams == 0)
        return CM3D_ERR_ARG;
    if ((uintptr_t)hit_uvd & 15) return CM3D_ERR_ARG;
    const VpArgs a{packed, bbox, cams, mask_off, mask_frame, mask_cam, flags, hit_uvd, off, frame_seed, W, H, n_cams, n_frames, n_masks,
                   idx_cap, per_mask, seed, max_px, kept_only ? 1 : 0, vp_count, vp_status, vp_xyz, vp_pix, vp_src, vp_depth, vp_d2};
    hipLaunchKernelGGL(k_virtual_points, dim3(n_masks), dim3(VP_THREADS), 0, (hipStream_t)stream, a);
    CM3D_CHECK_LAUNCH();
    return CM3D_OK;
}
