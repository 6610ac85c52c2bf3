// Box size from the fitted extents, pooled over each track (include/cm3d_hip.h: cm3d_box_size; host statement cm3d_amd/boxsize.py).
// cm3d_bev_fit leaves the extents of a vehicle's points at the fitted heading, cm3d_box_tracks the track of every kept box; here an
// order statistic of a track's extent / prior ratios becomes the size of its boxes, cm3d_box_place's rule hangs that size on the
// rectangle again, and the velocity is taken on the new centres.  All float64, every product, quotient, sum and difference rounded on
// its own (-ffp-contract=off), no library call: the host statement gives the same bits.
//
// Launches (one thread per mask each):
//   k_size_observe   membership, the validated follower and predecessor, the frame time and the two observed ratios (NaN: none) into
//                    the workspace; initialises the six pure outputs
//   k_size_pool      a member walks its track once from the head along the validated followers, both dimensions in the one walk:
//                    it counts the observations and the rank of its own ratio among them (L steps per thread; no head doing L^2
//                    work, no sort).  Ranks are unique, so the one member of rank k stores the track's ratio into the head's
//                    workspace row; with fewer than min_obs observations nobody does, and the 1.0 the first launch put into every
//                    row stands.  No race, no atomic but the status's.
//   k_size_apply     a member reads its head's two ratios, writes size and ratio, and -- placed members -- its own centre.  It reads no
//                    other mask's centre.
//   k_size_velocity  the two-neighbour or the least-squares velocity on the centres the third launch left
// Latency bound like tracks.hip: a walk is a chain of dependent 4-byte loads of the validated follower; the 16-byte observation it
// reads per step hangs off the chain, not in it.  Neither bytes nor arithmetic bound it; no HBM roofline applies.
// box: k_size_observe reads columns 0, 1 and 8 of its own row; k_size_apply writes columns 0, 1 of its own row, computed from fit_rect
// and the sensor alone; k_size_velocity only reads.  Each hazard lies across a launch boundary of one stream.
// Every index that comes from mask_frame, track_id, next_match or prev_match is checked before it addresses anything.
#include "common.h"

#define SZ_NOT_MEMBER 0
#define SZ_MEMBER     1           // a member whose track's walk did not reach it, or whose head is none: ratios 1.0, not pooled
#define SZ_ON_TRACK   2

static __device__ __forceinline__ bool sz_finite(double v) { return fabs(v) < INFINITY; }      // (NaN fails the comparison)

static __device__ __forceinline__ bool sz_member(int i, const int32_t *__restrict__ mask_frame, const int32_t *__restrict__ track_id,
                                                 const int32_t *__restrict__ track_pos, const int32_t *__restrict__ track_len, int n_masks,
                                                 int n_frames)
{
    const int L = track_len[i], h = track_id[i], p = track_pos[i], f = mask_frame[i];
    return L > 0 && h >= 0 && h < n_masks && p >= 0 && p < L && f >= 0 && f < n_frames;
}

static __device__ __forceinline__ int sz_class(double b8, int n_classes) { return b8 >= 0.0 && b8 < (double)n_classes ? (int)b8 : 0; }

struct SizeWs {                   // the workspace: the doubles first, the int32 arrays need no padding behind them
    double *time, *obs, *ratio;   // [M], [M][2] observed ratios, [M][2] the track's ratios in the head's row
    int32_t *vnext, *vprev, *state;
};

static __host__ __device__ __forceinline__ SizeWs size_ws(void *workspace, int n_masks)
{
    SizeWs w;
    w.time = (double *)workspace; w.obs = w.time + n_masks; w.ratio = w.obs + 2 * (int64_t)n_masks;
    w.vnext = (int32_t *)(w.ratio + 2 * (int64_t)n_masks); w.vprev = w.vnext + n_masks; w.state = w.vprev + n_masks;
    return w;
}

__global__ __launch_bounds__(256) void k_size_observe(const double *__restrict__ box, const int32_t *__restrict__ mask_frame,
                                                      const double *__restrict__ fit_rect, const int32_t *__restrict__ place_src,
                                                      const double *__restrict__ prior_wlh, int n_classes,
                                                      const int32_t *__restrict__ next_match, const int32_t *__restrict__ prev_match,
                                                      const int32_t *__restrict__ track_id, const int32_t *__restrict__ track_pos,
                                                      const int32_t *__restrict__ track_len, const double *__restrict__ frame_time,
                                                      int n_masks, int n_frames, double lo, double hi, SizeWs w,
                                                      double *__restrict__ size_wlh, int32_t *__restrict__ size_src,
                                                      double *__restrict__ size_ratio, int32_t *__restrict__ size_obs,
                                                      double *__restrict__ size_placed, double *__restrict__ size_vel,
                                                      int32_t *__restrict__ status)
{
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= n_masks) return;
    const double *b = box + (int64_t)i * CM3D_BOX_STRIDE;
    const double bx = b[0], by = b[1];
    const int c = sz_class(b[8], n_classes);
    const double wid0 = prior_wlh[3 * c], len0 = prior_wlh[3 * c + 1], hgt0 = prior_wlh[3 * c + 2];
    size_wlh[3 * (int64_t)i] = wid0; size_wlh[3 * (int64_t)i + 1] = len0; size_wlh[3 * (int64_t)i + 2] = hgt0;
    size_src[i] = 0;
    size_ratio[2 * (int64_t)i] = 0.0; size_ratio[2 * (int64_t)i + 1] = 0.0;
    size_obs[2 * (int64_t)i] = 0; size_obs[2 * (int64_t)i + 1] = 0;
    size_placed[2 * (int64_t)i] = bx; size_placed[2 * (int64_t)i + 1] = by;
    size_vel[2 * (int64_t)i] = 0.0; size_vel[2 * (int64_t)i + 1] = 0.0;

    const bool member = sz_member(i, mask_frame, track_id, track_pos, track_len, n_masks, n_frames);
    int vn = -1, vp = -1, bits = 0;
    double t = 0.0, rl = NAN, rw = NAN;
    if (member) {
        t = frame_time[mask_frame[i]];
        const int h = track_id[i], p = track_pos[i];
        const int j = next_match[i], q = prev_match[i];
        if (j >= 0 && j < n_masks && sz_member(j, mask_frame, track_id, track_pos, track_len, n_masks, n_frames) && track_id[j] == h &&
            track_pos[j] == p + 1)                                // (p < track_len[i]: p + 1 does not overflow)
            vn = j;
        else if (j != -1) bits |= 1;
        if (q >= 0 && q < n_masks && sz_member(q, mask_frame, track_id, track_pos, track_len, n_masks, n_frames) && track_id[q] == h &&
            track_pos[q] == p - 1)
            vp = q;
        else if (q != -1) bits |= 1;
        if (place_src[i] != 0) {
            const double a = fit_rect[(int64_t)i * CM3D_MATCH_BOX_STRIDE + 2], bb = fit_rect[(int64_t)i * CM3D_MATCH_BOX_STRIDE + 3];
            if (len0 > 0.0) { const double r = a / len0; if (lo <= r && r <= hi) rl = r; }
            if (wid0 > 0.0) { const double r = bb / wid0; if (lo <= r && r <= hi) rw = r; }
        }
    }
    w.time[i] = t; w.vnext[i] = vn; w.vprev[i] = vp; w.state[i] = member ? SZ_MEMBER : SZ_NOT_MEMBER;
    w.obs[2 * (int64_t)i] = rl; w.obs[2 * (int64_t)i + 1] = rw;
    w.ratio[2 * (int64_t)i] = 1.0; w.ratio[2 * (int64_t)i + 1] = 1.0;
    if (bits) atomicOr(status, bits);
}

__global__ __launch_bounds__(256) void k_size_pool(const int32_t *__restrict__ track_id, const int32_t *__restrict__ track_pos,
                                                   int n_masks, int n_frames, double q, int min_obs, SizeWs w,
                                                   int32_t *__restrict__ size_obs, int32_t *__restrict__ status)
{
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= n_masks || w.state[i] == SZ_NOT_MEMBER) return;
    const int h = track_id[i];                                    // in [0, n_masks): i is a member
    // (members of this launch raise their own state from SZ_MEMBER to SZ_ON_TRACK: either value reads as a member here)
    if (w.state[h] == SZ_NOT_MEMBER || track_id[h] != h || track_pos[h] != 0) { atomicOr(status, 1); return; }   // no head: no track
    const double ml = w.obs[2 * (int64_t)i], mw = w.obs[2 * (int64_t)i + 1];
    const bool has_l = ml == ml, has_w = mw == mw;
    int nl = 0, nw = 0, rank_l = 0, rank_w = 0, m = h, k = 0;
    bool met = false;
    // followers raise track_pos by one: no cycle; a track of what cm3d_box_tracks wrote has at most n_frames members
    while (m >= 0 && k < n_frames) {
        const int nx = w.vnext[m];                                // the chain's load first: the record's hangs off it
        const double vl = w.obs[2 * (int64_t)m], vw = w.obs[2 * (int64_t)m + 1];
        if (m == i) met = true;
        else {                                                    // in front of the member an equal value comes first
            if (vl == vl) { ++nl; if (has_l && (met ? vl < ml : vl <= ml)) ++rank_l; }
            if (vw == vw) { ++nw; if (has_w && (met ? vw < mw : vw <= mw)) ++rank_w; }
        }
        ++k; m = nx;
    }
    int bits = m >= 0 ? 2 : 0;                                    // cut at n_frames steps
    if (!met) bits |= 1;                                          // the walk of its track does not reach the member
    if (bits) atomicOr(status, bits);
    if (!met) return;
    if (has_l) ++nl;
    if (has_w) ++nw;
    size_obs[2 * (int64_t)i] = nl; size_obs[2 * (int64_t)i + 1] = nw;
    w.state[i] = SZ_ON_TRACK;
    // (below min_obs the 1.0 of k_size_observe stands in the head's row)
    if (has_l && nl >= min_obs && rank_l == (int)(q * (double)(nl - 1))) w.ratio[2 * (int64_t)h] = ml;
    if (has_w && nw >= min_obs && rank_w == (int)(q * (double)(nw - 1))) w.ratio[2 * (int64_t)h + 1] = mw;
}

// box is written in columns 0, 1 of the thread's own row and not read
template <bool WAYMO>
__global__ __launch_bounds__(256) void k_size_apply(double *__restrict__ box, const int32_t *__restrict__ mask_frame,
                                                    const double *__restrict__ fit_rect, const int32_t *__restrict__ place_src,
                                                    const double *__restrict__ ego_xyz, double thin, const int32_t *__restrict__ track_id,
                                                    int n_masks, int min_obs, SizeWs w, double *__restrict__ size_wlh,
                                                    int32_t *__restrict__ size_src, double *__restrict__ size_ratio,
                                                    const int32_t *__restrict__ size_obs)
{
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= n_masks) return;
    const int state = w.state[i];
    if (state == SZ_NOT_MEMBER) return;
    double r_len = 1.0, r_wid = 1.0;
    int src = 0;
    if (state == SZ_ON_TRACK) {
        const int h = track_id[i];
        r_len = w.ratio[2 * (int64_t)h]; r_wid = w.ratio[2 * (int64_t)h + 1];
        src = (size_obs[2 * (int64_t)i] >= min_obs ? 1 : 0) | (size_obs[2 * (int64_t)i + 1] >= min_obs ? 2 : 0);
    }
    size_ratio[2 * (int64_t)i] = r_len; size_ratio[2 * (int64_t)i + 1] = r_wid;
    if (place_src[i] == 0) return;                                // kept the lane's yaw: the prior row and 0 of k_size_observe stand
    const double wid0 = size_wlh[3 * (int64_t)i], len0 = size_wlh[3 * (int64_t)i + 1];     // the class's row, as k_size_observe left it
    const double len = r_len * len0, wid = r_wid * wid0;
    size_wlh[3 * (int64_t)i] = wid; size_wlh[3 * (int64_t)i + 1] = len;
    size_src[i] = src;
    const double *fr = fit_rect + (int64_t)i * CM3D_MATCH_BOX_STRIDE;
    const double cx = fr[0], cy = fr[1], ra = fr[2], rb = fr[3], hc = fr[4], hs = fr[5];
    const int f = mask_frame[i];                                  // in [0, n_frames): i is a member
    const double sx = WAYMO ? 0.0 : ego_xyz[3 * (int64_t)f], sy = WAYMO ? 0.0 : ego_xyz[3 * (int64_t)f + 1];
    if (!(sz_finite(sx) && sz_finite(sy) && sz_finite(cx) && sz_finite(cy) && sz_finite(ra) && sz_finite(rb) && sz_finite(hc) && sz_finite(hs)))
        return;                                                   // cm3d_box_place places no such mask: the centre stays
    const double ex = sx - cx, ey = sy - cy;
    const double pu = (ex * hc) + (ey * hs), pv = (ey * hc) - (ex * hs);
    const double su = pu >= 0.0 ? 1.0 : -1.0, sv = pv >= 0.0 ? 1.0 : -1.0;
    const bool au = rb >= thin, av = ra >= thin;
    const double du = au ? su * ((ra - len) * 0.5) : 0.0;
    const double dv = av ? sv * ((rb - wid) * 0.5) : 0.0;
    double *b = box + (int64_t)i * CM3D_BOX_STRIDE;
    b[0] = ((du * hc) - (dv * hs)) + cx;
    b[1] = ((du * hs) + (dv * hc)) + cy;
}

__global__ __launch_bounds__(256) void k_size_velocity(const double *__restrict__ box, const int32_t *__restrict__ track_pos,
                                                       const int32_t *__restrict__ track_len, int n_masks, int n_frames, double max_dt,
                                                       int smooth_window, SizeWs w, double *__restrict__ size_vel,
                                                       int32_t *__restrict__ status)
{
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= n_masks || w.state[i] == SZ_NOT_MEMBER) return;      // (the zeros of k_size_observe stand)
    const double *bi = box + (int64_t)i * CM3D_BOX_STRIDE;
    const double t = w.time[i];
    double vx = 0.0, vy = 0.0;
    if (smooth_window == 0) {                                     // cm3d_box_velocity's rule on the validated links
        const int nm = w.vnext[i], pm = w.vprev[i];
        const double *bp = box + (int64_t)(nm >= 0 ? nm : i) * CM3D_BOX_STRIDE, *bm = box + (int64_t)(pm >= 0 ? pm : i) * CM3D_BOX_STRIDE;
        const double tp = w.time[nm >= 0 ? nm : i], tm = w.time[pm >= 0 ? pm : i];
        if (nm >= 0 && pm >= 0 && tp - tm <= max_dt) {
            const double span = tp - tm;
            vx = (bp[0] - bm[0]) / span; vy = (bp[1] - bm[1]) / span;
        } else if (nm >= 0 && tp - t <= max_dt) {
            const double span = tp - t;
            vx = (bp[0] - bi[0]) / span; vy = (bp[1] - bi[1]) / span;
        } else if (pm >= 0 && t - tm <= max_dt) {
            const double span = t - tm;
            vx = (bi[0] - bm[0]) / span; vy = (bi[1] - bm[1]) / span;
        }
    } else {                                                      // cm3d_box_tracks' rule: the window of W members on either side
        const int W = smooth_window < n_frames ? smooth_window : n_frames;
        const int p = track_pos[i], L = track_len[i];             // 0 <= p < L: i is a member
        const int back = p < W ? p : W;
        const int ahead = L - 1 - p < W ? L - 1 - p : W;
        int want = (int64_t)back + 1 + ahead > n_frames ? n_frames + 1 : back + 1 + ahead;
        if (want > n_frames) { want = n_frames; atomicOr(status, 2); }     // (a track_len above n_frames)
        int m = i;
        for (int s = 0; s < back; ++s) {
            const int pv = w.vprev[m];
            if (pv < 0) break;
            m = pv;
        }
        const double xi = bi[0], yi = bi[1];
        double St = 0.0, Stt = 0.0, Sx = 0.0, Sy = 0.0, Stx = 0.0, Sty = 0.0;
        int n = 0;
        while (n < want && m >= 0) {
            const int nx = w.vnext[m];
            const double *bm = box + (int64_t)m * CM3D_BOX_STRIDE;
            const double tt = w.time[m] - t, x = bm[0] - xi, y = bm[1] - yi;
            St = St + tt; Stt = Stt + (tt * tt);
            Sx = Sx + x; Sy = Sy + y;
            Stx = Stx + (tt * x); Sty = Sty + (tt * y);
            ++n; m = nx;
        }
        if (n >= 2) {
            const double dn = (double)n;
            const double den = (dn * Stt) - (St * St);
            if (den > 0.0) {
                vx = ((dn * Stx) - (St * Sx)) / den;
                vy = ((dn * Sty) - (St * Sy)) / den;
            }
        }
    }
    size_vel[2 * (int64_t)i] = vx; size_vel[2 * (int64_t)i + 1] = vy;
}

extern "C" int64_t cm3d_box_size_workspace_bytes(int32_t n_masks)
{
    return (int64_t)(n_masks > 0 ? n_masks : 1) * (int64_t)(5 * sizeof(double) + 3 * sizeof(int32_t));
}

extern "C" int cm3d_box_size(double *box, int32_t *flags, const int32_t *mask_frame, const double *fit_rect, const int32_t *place_src,
                             const double *prior_wlh, int32_t n_classes, const double *ego_xyz, int32_t waymo, double thin,
                             const int32_t *next_match, const int32_t *prev_match, const int32_t *track_id, const int32_t *track_pos,
                             const int32_t *track_len, const double *frame_time, int32_t n_masks, int32_t n_frames, double max_dt,
                             int32_t smooth_window, double q, int32_t min_obs, double lo, double hi, double *size_wlh, int32_t *size_src,
                             double *size_ratio, int32_t *size_obs, double *size_placed, double *size_vel, int32_t *status, void *workspace,
                             int64_t workspace_bytes, cm3d_stream_t stream)
{
    if (n_masks < 0 || n_frames <= 0 || n_classes <= 0 || min_obs < 1 || smooth_window < 0) return CM3D_ERR_ARG;
    if (!(q >= 0.0 && q <= 1.0) || !(max_dt > 0.0)) return CM3D_ERR_ARG;                   // (NaN fails the comparisons)
    if (!(thin >= 0.0) || !(thin < INFINITY) || !(lo > 0.0) || !(lo <= hi) || !(hi < INFINITY)) return CM3D_ERR_ARG;
    if (!frame_time || !prior_wlh || !status || (!waymo && !ego_xyz)) return CM3D_ERR_ARG;
    if (n_masks > 0 && (!box || !flags || !mask_frame || !fit_rect || !place_src || !next_match || !prev_match || !track_id || !track_pos ||
                        !track_len || !size_wlh || !size_src || !size_ratio || !size_obs || !size_placed || !size_vel))
        return CM3D_ERR_ARG;
    if (!workspace || workspace_bytes < cm3d_box_size_workspace_bytes(n_masks)) return CM3D_ERR_WORKSPACE;
    if (n_masks == 0) return CM3D_OK;
    hipStream_t st = (hipStream_t)stream;
    const SizeWs w = size_ws(workspace, n_masks);
    const dim3 grid((n_masks + 255) / 256), block(256);
    hipLaunchKernelGGL(k_size_observe, grid, block, 0, st, box, mask_frame, fit_rect, place_src, prior_wlh, n_classes, next_match, prev_match,
                       track_id, track_pos, track_len, frame_time, n_masks, n_frames, lo, hi, w, size_wlh, size_src, size_ratio, size_obs,
                       size_placed, size_vel, status);
    CM3D_CHECK_LAUNCH();
    hipLaunchKernelGGL(k_size_pool, grid, block, 0, st, track_id, track_pos, n_masks, n_frames, q, min_obs, w, size_obs, status);
    CM3D_CHECK_LAUNCH();
    if (waymo)
        hipLaunchKernelGGL(k_size_apply<true>, grid, block, 0, st, box, mask_frame, fit_rect, place_src, ego_xyz, thin, track_id, n_masks,
                           min_obs, w, size_wlh, size_src, size_ratio, size_obs);
    else
        hipLaunchKernelGGL(k_size_apply<false>, grid, block, 0, st, box, mask_frame, fit_rect, place_src, ego_xyz, thin, track_id, n_masks,
                           min_obs, w, size_wlh, size_src, size_ratio, size_obs);
    CM3D_CHECK_LAUNCH();
    hipLaunchKernelGGL(k_size_velocity, grid, block, 0, st, box, track_pos, track_len, n_masks, n_frames, max_dt, smooth_window, w, size_vel,
                       status);
    CM3D_CHECK_LAUNCH();
    return CM3D_OK;
}
