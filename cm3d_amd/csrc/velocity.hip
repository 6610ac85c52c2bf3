// Box velocity from frame-to-frame association (include/cm3d_hip.h: cm3d_box_velocity; host statement cm3d_amd/velocity.py).
// The reference writes "velocity": [0, 0] (src/nuscenes/2d_to_3d.py:808-817); this stage is what fills the field, behind the pass.
//
// Launches for all links f -> frame_next[f] of a batch (link slot f = frame f):
//   k_track_init         one thread per mask / frame: the four outputs, every mask's frame, the range check of frame_next
//   k_assign_block_owner assign.h: the first slot of every 256-pair block
//   k_track_weight       one thread per (mask of f, mask of n) pair: gated centre distance -> int32 weight matrix (L2 resident)
//   k_track_assign<C>    one wave per link of at most 64 C masks on its larger side (C = 1, 2, 4, 16): assign.h's AssignSolver with
//                        rows = the smaller side, then next_match of f's masks and prev_match of n's
//   k_track_velocity     one thread per mask: central / forward / backward difference
// Latency / integer bound like the fusion matcher (a link's matrix is a few KB); no HBM roofline applies.
// Every offset that comes from mask_off, frame_next or pair_off is clamped or checked before it indexes anything.
#include "assign.h"

#define TV_LDS 8192               // weights of a link up to this many pairs sit in LDS, larger ones are read from L2 (k_bev_assign's seam)

// masks of frame f: [m0, m0 + M), inside [0, n_masks] whatever mask_off holds
static __device__ __forceinline__ void track_frame_masks(const int32_t *__restrict__ mask_off, int f, int n_masks, int &m0, int &M)
{
    const int a = mask_off[f], b = mask_off[f + 1];
    m0 = a < 0 ? 0 : a > n_masks ? n_masks : a;
    const int m1 = b < m0 ? m0 : b > n_masks ? n_masks : b;
    M = m1 - m0;
}

// link slot f: the following frame n, both mask ranges, dt; ok = the rule's link with both frames inside the solver's capacity
struct TrackLink { int n, f0, Mf, n0, Mn; double dt; bool ok, over; };
static __device__ __forceinline__ TrackLink track_link(int f, const int32_t *__restrict__ mask_off, int n_frames, int n_masks,
                                                       const int32_t *__restrict__ frame_next, const double *__restrict__ frame_time,
                                                       double max_dt)
{
    TrackLink L;
    L.n = frame_next[f];
    L.ok = L.n >= 0 && L.n < n_frames;           // (outside [-1, F): status bit 0, by k_track_init)
    L.over = false;
    L.f0 = L.n0 = L.Mf = L.Mn = 0;
    L.dt = 0.0;
    if (!L.ok) return L;
    L.dt = frame_time[L.n] - frame_time[f];
    L.ok = L.dt > 0.0 && L.dt <= max_dt;
    if (!L.ok) return L;
    track_frame_masks(mask_off, f, n_masks, L.f0, L.Mf);
    track_frame_masks(mask_off, L.n, n_masks, L.n0, L.Mn);
    L.over = L.Mf > CM3D_MAX_MASKS_PER_FRAME || L.Mn > CM3D_MAX_MASKS_PER_FRAME;
    L.ok = !L.over;
    return L;
}

// the slot's pairs as the host laid them out: exactly Mf * Mn of them, inside [0, total_pairs]
static __device__ __forceinline__ bool track_slot_ok(const TrackLink &L, int64_t lo, int64_t hi, int64_t total_pairs)
{
    return lo >= 0 && hi <= total_pairs && hi - lo == (int64_t)L.Mf * L.Mn;
}

__global__ __launch_bounds__(256) void k_track_init(const int32_t *__restrict__ mask_off, int n_frames, int n_masks,
                                                    const int32_t *__restrict__ frame_next, int32_t *__restrict__ next_match,
                                                    int32_t *__restrict__ prev_match, double *__restrict__ vel,
                                                    int32_t *__restrict__ vel_src, int32_t *__restrict__ mask_frame,
                                                    int32_t *__restrict__ status)
{
    const int t = blockIdx.x * 256 + threadIdx.x;
    if (t < n_masks) {
        next_match[t] = -1; prev_match[t] = -1;
        vel[2 * (int64_t)t] = 0.0; vel[2 * (int64_t)t + 1] = 0.0;
        vel_src[t] = 0;
        int lo = 0, hi = n_frames;              // last f with mask_off[f] <= t: frame f owns [mask_off[f], mask_off[f+1])
        while (hi - lo > 1) {
            const int mid = (lo + hi) >> 1;
            if (mask_off[mid] <= t) lo = mid; else hi = mid;
        }
        mask_frame[t] = lo;
    }
    if (t < n_frames) {
        const int n = frame_next[t];
        if (n < -1 || n >= n_frames) atomicOr(status, 1);
    }
}

static __device__ __forceinline__ int track_weight(const double *__restrict__ box, const int32_t *__restrict__ flags,
                                                   const int32_t *__restrict__ class_id, const int32_t *__restrict__ track_group,
                                                   const double *__restrict__ max_speed, int n_classes, int n_groups, int i, int j,
                                                   double dt)
{
    if ((flags[i] & 3) != 3 || (flags[j] & 3) != 3) return 0;
    const int ci = class_id[i], cj = class_id[j];
    if (ci < 0 || ci >= n_classes || cj < 0 || cj >= n_classes) return 0;
    const int g = track_group[ci];
    if (g != track_group[cj] || g < 0 || g >= n_groups) return 0;
    const double *bf = box + (int64_t)i * CM3D_BOX_STRIDE, *bn = box + (int64_t)j * CM3D_BOX_STRIDE;
    const double dx = bn[0] - bf[0], dy = bn[1] - bf[1];
    const double d2 = (dx * dx) + (dy * dy);      // (-ffp-contract=off: every operation rounded on its own)
    const double gate = max_speed[g] * dt;
    if (!(gate > 0.0 && d2 <= gate * gate)) return 0;
    const double r = sqrt(d2) / gate;
    if (!(r <= 1.0)) return 0;
    return 1 + (int)((1.0 - r) * (double)(ASSIGN_KMAX - 1));
}

__global__ __launch_bounds__(256) void k_track_weight(const double *__restrict__ box, const int32_t *__restrict__ flags,
                                                      const int32_t *__restrict__ mask_off, int n_frames, int n_masks,
                                                      const int32_t *__restrict__ class_id, const int32_t *__restrict__ track_group,
                                                      const double *__restrict__ max_speed, int n_classes, int n_groups,
                                                      const int32_t *__restrict__ frame_next, const double *__restrict__ frame_time,
                                                      double max_dt, const int64_t *__restrict__ pair_off,
                                                      const int32_t *__restrict__ blk_link, int64_t total_pairs,
                                                      int32_t *__restrict__ weight)
{
    const int64_t t = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (t >= total_pairs) return;
    // assign_locate's walk; the column count of a slot comes from the following frame's masks, not from a second offset array
    int f = blk_link[blockIdx.x];
    f = f < 0 ? 0 : f >= n_frames ? n_frames - 1 : f;
    while (f + 1 < n_frames && pair_off[f + 1] <= t) ++f;      // a block spans few slots
    const TrackLink L = track_link(f, mask_off, n_frames, n_masks, frame_next, frame_time, max_dt);
    const int64_t lo = pair_off[f], r = t - lo;
    if (!L.ok || !track_slot_ok(L, lo, pair_off[f + 1], total_pairs) || r < 0 || r >= (int64_t)L.Mf * L.Mn) return;
    const int p = (int)(r / L.Mn);
    const int g = (int)(r - (int64_t)p * L.Mn);
    weight[t] = track_weight(box, flags, class_id, track_group, max_speed, n_classes, n_groups, L.f0 + p, L.n0 + g, L.dt);
}

template <int CPL>
__global__ __launch_bounds__(64) void k_track_assign(const int32_t *__restrict__ mask_off, int n_frames, int n_masks,
                                                     const int32_t *__restrict__ frame_next, const double *__restrict__ frame_time,
                                                     double max_dt, const int64_t *__restrict__ pair_off, int64_t total_pairs,
                                                     const int32_t *__restrict__ weight, int32_t *__restrict__ next_match,
                                                     int32_t *__restrict__ prev_match, int32_t *__restrict__ status)
{
    __shared__ int s_w[TV_LDS];
    const int f = blockIdx.x, lane = threadIdx.x;
    const TrackLink L = track_link(f, mask_off, n_frames, n_masks, frame_next, frame_time, max_dt);
    const int64_t lo = pair_off[f];
    if (CPL == 1 && (L.over || (L.ok && !track_slot_ok(L, lo, pair_off[f + 1], total_pairs)))) {      // once per slot
        if (lane == 0) atomicOr(status, 2);
        return;
    }
    if (!L.ok || !track_slot_ok(L, lo, pair_off[f + 1], total_pairs)) return;
    const int P = L.Mf, G = L.Mn;
    const int big = P > G ? P : G;
    if (P <= 0 || G <= 0) return;
    if (!assign_instance_takes<CPL>(big)) return;                 // another instance's link
    const int32_t *__restrict__ Wm = weight + lo;
    const bool tr = P > G;                       // rows = the smaller side
    const int n = tr ? G : P, m = tr ? P : G;
    const bool in_lds = n * m <= TV_LDS;
    if (in_lds) {                                // LDS image: row-major [n][m] in (row, column) order of the search
        for (int q = lane; q < n * m; q += 64) {
            const int i = q / m, j = q - i * m;
            s_w[q] = tr ? Wm[(int64_t)j * G + i] : Wm[(int64_t)i * G + j];
        }
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
        __builtin_amdgcn_wave_barrier();
        __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
    }
    auto wgt = [&](int i, int j) -> int {        // weight of row i, column j (1-based)
        if (in_lds) return s_w[(i - 1) * m + (j - 1)];
        return tr ? Wm[(int64_t)(j - 1) * G + (i - 1)] : Wm[(int64_t)(i - 1) * G + (j - 1)];
    };
    AssignSolver<CPL> S;
    S.solve(n, m, wgt, [](int) {});
#pragma unroll
    for (int k = 0; k < CPL; ++k) {
        const int col = k * 64 + lane + 1;
        if (col <= m && S.p[k] != 0) {
            const int i = S.p[k];
            if (i <= n && wgt(i, col) > 0) {     // weight 0 (gated out, another group, not kept): not a match
                const int pi = tr ? col - 1 : i - 1, gi = tr ? i - 1 : col - 1;
                next_match[L.f0 + pi] = L.n0 + gi;
                prev_match[L.n0 + gi] = L.f0 + pi;
            }
        }
    }
}

__global__ __launch_bounds__(256) void k_track_velocity(const double *__restrict__ box, const int32_t *__restrict__ flags, int n_frames,
                                                        int n_masks, const double *__restrict__ frame_time, double max_dt,
                                                        const int32_t *__restrict__ mask_frame,
                                                        const int32_t *__restrict__ next_match, const int32_t *__restrict__ prev_match,
                                                        double *__restrict__ vel, int32_t *__restrict__ vel_src)
{
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= n_masks || (flags[i] & 3) != 3) return;              // (not kept: the zeros of k_track_init stand)
    int nm = next_match[i], pm = prev_match[i];
    nm = nm >= 0 && nm < n_masks ? nm : -1;
    pm = pm >= 0 && pm < n_masks ? pm : -1;
    auto time_of = [&](int m) -> double {
        const int f = mask_frame[m];
        return frame_time[f < 0 ? 0 : f >= n_frames ? n_frames - 1 : f];
    };
    const double *b = box + (int64_t)i * CM3D_BOX_STRIDE;
    const double *bp = box + (int64_t)(nm >= 0 ? nm : i) * CM3D_BOX_STRIDE, *bm = box + (int64_t)(pm >= 0 ? pm : i) * CM3D_BOX_STRIDE;
    const double t = time_of(i), tp = time_of(nm >= 0 ? nm : i), tm = time_of(pm >= 0 ? pm : i);
    double vx = 0.0, vy = 0.0;
    int src = 0;
    if (nm >= 0 && pm >= 0 && tp - tm <= max_dt) {
        const double span = tp - tm;
        vx = (bp[0] - bm[0]) / span; vy = (bp[1] - bm[1]) / span; src = 3;
    } else if (nm >= 0 && tp - t <= max_dt) {
        const double span = tp - t;
        vx = (bp[0] - b[0]) / span; vy = (bp[1] - b[1]) / span; src = 1;
    } else if (pm >= 0 && t - tm <= max_dt) {
        const double span = t - tm;
        vx = (b[0] - bm[0]) / span; vy = (b[1] - bm[1]) / span; src = 2;
    }
    vel[2 * (int64_t)i] = vx; vel[2 * (int64_t)i + 1] = vy;
    vel_src[i] = src;
}

extern "C" int64_t cm3d_box_velocity_workspace_bytes(int64_t total_pairs, int32_t n_masks)
{
    return assign_workspace_bytes(total_pairs) + (int64_t)(n_masks > 0 ? n_masks : 1) * (int64_t)sizeof(int32_t);
}

extern "C" int cm3d_box_velocity(const double *box, const int32_t *flags, const int32_t *mask_off, int32_t n_frames, int32_t n_masks,
                                 const int32_t *class_id, const int32_t *track_group, const double *max_speed, int32_t n_classes,
                                 int32_t n_groups, const int32_t *frame_next, const double *frame_time, double max_dt,
                                 const int64_t *pair_off, int32_t n_links, int64_t total_pairs, int32_t *next_match,
                                 int32_t *prev_match, double *vel, int32_t *vel_src, int32_t *status, void *workspace,
                                 int64_t workspace_bytes, cm3d_stream_t stream)
{
    if (!mask_off || !frame_next || !frame_time || !pair_off || !track_group || !max_speed || !status) return CM3D_ERR_ARG;
    if (n_frames <= 0 || n_masks < 0 || n_classes <= 0 || n_groups <= 0 || n_links != n_frames || total_pairs < 0) return CM3D_ERR_ARG;
    if (!(max_dt > 0.0)) return CM3D_ERR_ARG;
    if (n_masks > 0 && (!box || !flags || !class_id || !next_match || !prev_match || !vel || !vel_src)) return CM3D_ERR_ARG;
    if (total_pairs >= ((int64_t)1 << 31) * 256) return CM3D_ERR_ARG;
    if (!workspace || workspace_bytes < cm3d_box_velocity_workspace_bytes(total_pairs, n_masks)) return CM3D_ERR_WORKSPACE;
    hipStream_t st = (hipStream_t)stream;
    const int64_t n_w = total_pairs > 0 ? total_pairs : 1;
    const int64_t n_blocks = (total_pairs + 255) / 256;
    int32_t *weight = (int32_t *)workspace;
    int32_t *blk_link = weight + n_w;
    int32_t *mask_frame = blk_link + (n_w + 255) / 256;
    const int n_init = n_masks > n_frames ? n_masks : n_frames;
    hipLaunchKernelGGL(k_track_init, dim3((n_init + 255) / 256), dim3(256), 0, st, mask_off, n_frames, n_masks, frame_next, next_match,
                       prev_match, vel, vel_src, mask_frame, status);
    CM3D_CHECK_LAUNCH();
    if (total_pairs == 0 || n_masks == 0) return CM3D_OK;         // no pair: no match, the zeros stand
    hipLaunchKernelGGL(k_assign_block_owner, dim3((unsigned)((n_blocks + 255) / 256)), dim3(256), 0, st, pair_off, n_links, n_blocks,
                       blk_link);
    CM3D_CHECK_LAUNCH();
    hipLaunchKernelGGL(k_track_weight, dim3((unsigned)n_blocks), dim3(256), 0, st, box, flags, mask_off, n_frames, n_masks, class_id,
                       track_group, max_speed, n_classes, n_groups, frame_next, frame_time, max_dt, pair_off, blk_link, total_pairs,
                       weight);
    CM3D_CHECK_LAUNCH();
#define TV_ASSIGN(C)                                                                                                                \
    hipLaunchKernelGGL(k_track_assign<C>, dim3(n_frames), dim3(64), 0, st, mask_off, n_frames, n_masks, frame_next, frame_time, max_dt, \
                       pair_off, total_pairs, weight, next_match, prev_match, status);                                             \
    CM3D_CHECK_LAUNCH()
    TV_ASSIGN(1); TV_ASSIGN(2); TV_ASSIGN(4); TV_ASSIGN(16);
#undef TV_ASSIGN
    hipLaunchKernelGGL(k_track_velocity, dim3((n_masks + 255) / 256), dim3(256), 0, st, box, flags, n_frames, n_masks, frame_time, max_dt,
                       mask_frame, next_match, prev_match, vel, vel_src);
    CM3D_CHECK_LAUNCH();
    return CM3D_OK;
}
