// Box tracks from the velocity stage's matches (include/cm3d_hip.h: cm3d_box_tracks; host statement cm3d_amd/tracks.py).
// The velocity stage leaves next_match / prev_match behind the pass; this stage follows them: track ids, positions and lengths, four
// statistics per track, a least-squares velocity over a window of the track, a track score and a length filter.
//
// Launches (one thread per mask each):
//   k_tracks_links   validates the mask's two links into the workspace (vnext, vprev, the mask's frame time) and initialises the five
//                    pure outputs
//   k_tracks_walk    a head (a kept mask without a valid previous link) walks its track: id and position of every member, and the four
//                    statistics in track order into the head's row
//   k_tracks_apply   a member reads its head's length and statistics, walks at most W links each way for the window sums, then
//                    rewrites its own score and flag
// Latency bound: a walk is a chain of dependent 4-byte loads of vnext (the box rows and times it reads hang off the chain, not in
// it); no HBM roofline applies.  The third launch changes box[.][7], box[.][9] and flags, so it reads validity from the workspace only
// and of other masks' rows only columns 0 and 1, which nothing here writes.
// Every index that comes from mask_frame, next_match or prev_match is checked before it addresses anything.
#include "common.h"

#define TR_NOT_KEPT (-2)          // vprev of a mask that is not kept (a kept mask without a valid link holds -1)

__global__ __launch_bounds__(256) void k_tracks_links(const int32_t *__restrict__ flags, const int32_t *__restrict__ mask_frame,
                                                      const int32_t *__restrict__ next_match, const int32_t *__restrict__ prev_match,
                                                      const double *__restrict__ frame_time, int n_masks, int n_frames,
                                                      int32_t *__restrict__ track_id, int32_t *__restrict__ track_pos,
                                                      int32_t *__restrict__ track_len, double *__restrict__ track_stat,
                                                      double *__restrict__ vel_smooth, double *__restrict__ w_time,
                                                      int32_t *__restrict__ vnext, int32_t *__restrict__ vprev,
                                                      int32_t *__restrict__ status)
{
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= n_masks) return;
    track_id[i] = -1; track_pos[i] = -1; track_len[i] = 0;
    double *st = track_stat + 4 * (int64_t)i;
    st[0] = 0.0; st[1] = 0.0; st[2] = 0.0; st[3] = 0.0;
    if (vel_smooth) { vel_smooth[2 * (int64_t)i] = 0.0; vel_smooth[2 * (int64_t)i + 1] = 0.0; }
    const int f = mask_frame[i];
    const bool in_frame = f >= 0 && f < n_frames;
    bool kept = (flags[i] & 3) == 3;
    int bits = 0;
    if (kept && !in_frame) { bits |= 1; kept = false; }
    int vn = -1, vp = kept ? -1 : TR_NOT_KEPT;
    double t = 0.0;
    if (kept) {
        t = frame_time[f];
        auto kept_time = [&](int j, double &tj) -> bool {         // j in [0, n_masks)
            const int fj = mask_frame[j];
            if ((flags[j] & 3) != 3 || fj < 0 || fj >= n_frames) return false;
            tj = frame_time[fj];
            return true;
        };
        const int j = next_match[i], p = prev_match[i];
        double tj = 0.0;
        if (j < -1 || j >= n_masks) bits |= 2;
        else if (j >= 0) {
            if (kept_time(j, tj) && prev_match[j] == i && tj > t) vn = j; else bits |= 4;
        }
        if (p < -1 || p >= n_masks) bits |= 2;
        else if (p >= 0) {
            if (kept_time(p, tj) && next_match[p] == i && tj < t) vp = p; else bits |= 4;
        }
    }
    w_time[i] = t; vnext[i] = vn; vprev[i] = vp;
    if (bits) atomicOr(status, bits);
}

__global__ __launch_bounds__(256) void k_tracks_walk(const double *__restrict__ box, int n_masks, int n_frames,
                                                     const double *__restrict__ w_time, const int32_t *__restrict__ vnext,
                                                     const int32_t *__restrict__ vprev, int32_t *__restrict__ track_id,
                                                     int32_t *__restrict__ track_pos, int32_t *__restrict__ track_len,
                                                     double *__restrict__ track_stat)
{
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= n_masks || vprev[i] != -1) return;                   // heads only
    int m = i, last = i, k = 0;
    double sum = 0.0, mx = 0.0;
    // links run strictly forward in time: a track has at most n_frames members and no cycle; the bound only restates that
    while (m >= 0 && k < n_frames) {
        const int nx = vnext[m];                                  // the chain's load first: the row's hangs off it
        const double s = box[(int64_t)m * CM3D_BOX_STRIDE + 7];
        sum = sum + s;
        if (k == 0 || s > mx) mx = s;
        track_id[m] = i; track_pos[m] = k;
        last = m; ++k; m = nx;
    }
    const double *b0 = box + (int64_t)i * CM3D_BOX_STRIDE, *b1 = box + (int64_t)last * CM3D_BOX_STRIDE;
    const double dx = b1[0] - b0[0], dy = b1[1] - b0[1];
    double *st = track_stat + 4 * (int64_t)i;
    track_len[i] = k;
    st[0] = sum; st[1] = mx; st[2] = w_time[last] - w_time[i]; st[3] = sqrt((dx * dx) + (dy * dy));
}

// box is read (columns 0, 1 of the window's members) and written (columns 7, 9 of the thread's own row): no __restrict__
__global__ __launch_bounds__(256) void k_tracks_apply(double *box, int32_t *__restrict__ flags, int n_masks, int min_length,
                                                      int score_mode, int smooth_window, const double *__restrict__ w_time,
                                                      const int32_t *__restrict__ vnext, const int32_t *__restrict__ vprev,
                                                      const int32_t *__restrict__ track_id, const int32_t *__restrict__ track_pos,
                                                      int32_t *track_len, double *track_stat, double *__restrict__ vel_smooth)
{
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= n_masks || vprev[i] == TR_NOT_KEPT) return;          // (not kept: the values of k_tracks_links stand)
    const int h = track_id[i], p = track_pos[i];
    if (h < 0 || h >= n_masks || p < 0) return;                   // (every kept mask has a head: never taken)
    const int L = track_len[h];
    const double *hs = track_stat + 4 * (int64_t)h;
    const double s0 = hs[0], s1 = hs[1], s2 = hs[2], s3 = hs[3];
    if (i != h) {                                                 // the head's row is read by its members and written by nobody here
        double *st = track_stat + 4 * (int64_t)i;
        track_len[i] = L;
        st[0] = s0; st[1] = s1; st[2] = s2; st[3] = s3;
    }
    double *bi = box + (int64_t)i * CM3D_BOX_STRIDE;
    if (smooth_window > 0) {
        const int back = p < smooth_window ? p : smooth_window;
        const int ahead = L - 1 - p < smooth_window ? L - 1 - p : smooth_window;
        const int n = back + 1 + ahead;
        double vx = 0.0, vy = 0.0;
        if (n >= 2) {
            int m = i;
            for (int q = 0; q < back && m >= 0; ++q) m = vprev[m];
            const double ti = w_time[i], xi = bi[0], yi = bi[1];
            double St = 0.0, Stt = 0.0, Sx = 0.0, Sy = 0.0, Stx = 0.0, Sty = 0.0;
            for (int q = 0; q < n && m >= 0; ++q) {
                const int nx = vnext[m];
                const double *bm = box + (int64_t)m * CM3D_BOX_STRIDE;
                const double t = w_time[m] - ti, x = bm[0] - xi, y = bm[1] - yi;
                St = St + t; Stt = Stt + (t * t);
                Sx = Sx + x; Sy = Sy + y;
                Stx = Stx + (t * x); Sty = Sty + (t * y);
                m = nx;
            }
            const double dn = (double)n;
            const double den = (dn * Stt) - (St * St);
            if (den > 0.0) {
                vx = ((dn * Stx) - (St * Sx)) / den;
                vy = ((dn * Sty) - (St * Sy)) / den;
            }
        }
        vel_smooth[2 * (int64_t)i] = vx; vel_smooth[2 * (int64_t)i + 1] = vy;
    }
    if (score_mode == 1) bi[7] = s0 / (double)L;
    else if (score_mode == 2) bi[7] = s1;
    if (L < min_length) {
        const int fl = flags[i] & ~2;
        flags[i] = fl;
        bi[9] = (double)fl;
    }
}

extern "C" int64_t cm3d_box_tracks_workspace_bytes(int32_t n_masks)
{
    return (int64_t)(n_masks > 0 ? n_masks : 1) * (int64_t)(sizeof(double) + 2 * sizeof(int32_t));
}

extern "C" int cm3d_box_tracks(double *box, int32_t *flags, const int32_t *mask_frame, const int32_t *next_match,
                               const int32_t *prev_match, const double *frame_time, int32_t n_masks, int32_t n_frames,
                               int32_t min_length, int32_t score_mode, int32_t smooth_window, int32_t *track_id, int32_t *track_pos,
                               int32_t *track_len, double *track_stat, double *vel_smooth, int32_t *status, void *workspace,
                               int64_t workspace_bytes, cm3d_stream_t stream)
{
    if (n_masks < 0 || n_frames <= 0 || min_length < 1 || score_mode < 0 || score_mode > 2 || smooth_window < 0) return CM3D_ERR_ARG;
    if (smooth_window > 0 && !vel_smooth) return CM3D_ERR_ARG;
    if (!frame_time || !status) return CM3D_ERR_ARG;
    if (n_masks > 0 && (!box || !flags || !mask_frame || !next_match || !prev_match || !track_id || !track_pos || !track_len || !track_stat))
        return CM3D_ERR_ARG;
    if (!workspace || workspace_bytes < cm3d_box_tracks_workspace_bytes(n_masks)) return CM3D_ERR_WORKSPACE;
    if (n_masks == 0) return CM3D_OK;
    hipStream_t st = (hipStream_t)stream;
    double *w_time = (double *)workspace;                         // the doubles first: the int32 arrays need no padding behind them
    int32_t *vnext = (int32_t *)(w_time + n_masks);
    int32_t *vprev = vnext + n_masks;
    const dim3 grid((n_masks + 255) / 256), block(256);
    hipLaunchKernelGGL(k_tracks_links, grid, block, 0, st, flags, mask_frame, next_match, prev_match, frame_time, n_masks, n_frames,
                       track_id, track_pos, track_len, track_stat, vel_smooth, w_time, vnext, vprev, status);
    CM3D_CHECK_LAUNCH();
    hipLaunchKernelGGL(k_tracks_walk, grid, block, 0, st, box, n_masks, n_frames, w_time, vnext, vprev, track_id, track_pos, track_len,
                       track_stat);
    CM3D_CHECK_LAUNCH();
    hipLaunchKernelGGL(k_tracks_apply, grid, block, 0, st, box, flags, n_masks, min_length, score_mode, smooth_window, w_time, vnext,
                       vprev, track_id, track_pos, track_len, track_stat, vel_smooth);
    CM3D_CHECK_LAUNCH();
    return CM3D_OK;
}
