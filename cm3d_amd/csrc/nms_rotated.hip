// Greedy rotated-box NMS: bird's-eye-view overlap of the boxes themselves instead of the centre distance of circle_nms.
//   reference: the rotated-rectangle nms(rrects, scores, ...) the reference carries as dead code, src/kitti/2d_to_3d.py:359-599
//   (strict > at :596, nms_threshold 0.4 at :531-534); there the polygons are rasterised on an integer pixel grid, here the overlap
//   is the float64 clip of bev_iou.h.
// The rule (cm3d_amd/nms.py restates it on the host, bit for bit):
//   order  descending score, ties by descending index (the pinned tie-break of nms_phase, boxes.hip);
//   pass   the box of rank r, unless suppressed, is kept and suppresses every later-ranked, not yet suppressed box j of its group (any
//          group when class_agnostic) with measure(i, j) > thr[group[j]];
//   iou    bev_iou(rec_i, rec_j);   cover   bev_inter_area(rec_i, rec_j) / (l_j * w_j), clamped to 1 -- the kept box is the FIRST
//          argument: the clip runs in coordinates relative to its centre;
//   a box without a positive float64 area or with a non-finite centre neither suppresses nor is suppressed.
// All float64 and latency-bound like k_box_nms: one workgroup per frame, no HBM roofline applies.
#include "common.h"
#include "bev_iou.h"

#define RN_MAX CM3D_MAX_MASKS_PER_FRAME
#define RN_THREADS 256                      // of a launch that may meet frames of more than 64 boxes; 64 when none has

// where a launch's records come from
#define RN_SRC_REC 0                        // double[n][6] records (cm3d_rotated_nms)
#define RN_SRC_NUSC 1                       // box rows, rotation [qw, 0, 0, qz] (cm3d_box_rotated_nms, waymo == 0)
#define RN_SRC_WAYMO 2                      // box rows, heading in column 3

struct RnArgs {
    const double *rec;                      // RN_SRC_REC
    const double *score;
    const int32_t *group;
    int32_t *keep;
    double *box;                            // RN_SRC_NUSC / RN_SRC_WAYMO
    int32_t *flags;
    const double *prior_wlh;
    const int32_t *nms_group;
    int n_classes;
    const int32_t *off;                     // frame_off / mask_off
    const double *thr;
    int n_groups, class_agnostic, cap, src;
};

template <int MEASURE>
static __device__ __forceinline__ double rn_measure(const double *__restrict__ ki, const double *__restrict__ bj)
{
    if (MEASURE == 0) return bev_iou(ki, bj);
    const double area_j = bj[2] * bj[3];
    if (!(area_j > 0.0)) return 0.0;
    const double c = bev_inter_area(ki, bj) / area_j;
    return c > 1.0 ? 1.0 : c;
}

// takes part in the overlap tests: positive area (NaN fails the comparison), finite centre
static __device__ __forceinline__ bool rn_live(const double *r)
{
    return r[2] * r[3] > 0.0 && fabs(r[0]) < INFINITY && fabs(r[1]) < INFINITY;
}

// Box m of the launch: its record, score and group; false when it does not take part in the NMS at all (a mask without a box).
static __device__ __forceinline__ bool rn_load(const RnArgs &a, int m, double *r, double &score, int &grp)
{
    bool part = true;
    if (a.src == RN_SRC_REC) {
#pragma unroll
        for (int q = 0; q < 6; ++q) r[q] = a.rec[(size_t)m * 6 + q];
        score = a.score[m];
        grp = a.group[m];
    } else {
        const double *b = a.box + (size_t)m * CM3D_BOX_STRIDE;
        part = (a.flags[m] & 1) != 0;
        const double b0 = b[0], b1 = b[1], b3 = b[3], b4 = b[4], b8 = b[8];
        score = b[7];
        int cls = b8 >= 0.0 && b8 < (double)a.n_classes ? (int)b8 : 0;
        // the [w, l, h] table: length along the heading
        r[0] = b0; r[1] = b1; r[2] = a.prior_wlh[3 * cls + 1]; r[3] = a.prior_wlh[3 * cls + 0];
        if (a.src == RN_SRC_WAYMO) { r[4] = cos(b3); r[5] = sin(b3); }
        else { const double ww = b3 * b3, zz = b4 * b4; r[4] = ww - zz; r[5] = (2.0 * b3) * b4; }      // axis of the rotation [qw, 0, 0, qz]
        grp = a.nms_group[cls];
    }
    if (grp < 0 || grp >= a.n_groups) grp = 0;
    return part;
}

static __device__ __forceinline__ void rn_store(const RnArgs &a, int m, bool keep)
{
    if (a.src == RN_SRC_REC) { a.keep[m] = keep ? 1 : 0; return; }
    const int fl = (a.flags[m] & ~2) | (keep ? 2 : 0);
    a.flags[m] = fl;
    a.box[(size_t)m * CM3D_BOX_STRIDE + 9] = (double)fl;
}

// LDS of a launch whose frames have up to `cap` boxes: none up to 64 (one wave's registers); else per box six doubles of the
// record, score and threshold, group, rank, the box at each rank, and two flag bytes
static inline size_t rn_lds_bytes(int cap) { return cap <= 64 ? 0 : (size_t)((cap + 7) & ~7) * (8 * sizeof(double) + 3 * sizeof(int) + 2); }

// One workgroup per frame.  A frame of up to 64 boxes runs in wave 0 alone: lane j keeps box j, ranks come from readlanes, the
// suppressed set is a 64-bit ballot mask, and in the step of a kept box lane j clips its own box against the broadcast one.  A larger
// frame (up to RN_MAX boxes; the launch then has RN_THREADS threads and rn_lds_bytes of LDS) sorts its records into LDS by rank and
// takes the same greedy steps with the threads striding over the later ranks: a step costs (later ranks / threads) clips, and only
// pairs (kept box, later box) are ever clipped -- a pairwise suppression matrix would clip all n^2 / 2 pairs up front, two to three
// times the work when a third of the boxes goes, for a scan that is serial either way.
template <int MEASURE>
__global__ __launch_bounds__(RN_THREADS) void k_rotated_nms(const RnArgs a)
{
    extern __shared__ __align__(8) double s_rn[];
    const int f = blockIdx.x;
    const int m0 = a.off[f];
    const int n_all = a.off[f + 1] - m0;
    const int nm = min(min(n_all, a.cap), RN_MAX);
    const int tid = threadIdx.x, nt = blockDim.x;
    // boxes beyond the bound take no part: keep 0
    for (int k = nm + tid; k < n_all; k += nt) rn_store(a, m0 + k, false);
    if (nm <= 0) return;
    if (nm <= 64) {
        if (tid >= 64) return;                                  // (no barrier on this path)
        double r[6] = {0.0, 0.0, 0.0, 0.0, 1.0, 0.0}, sc = 0.0, thr_j = 0.0;
        int grp = 0;
        bool part = false;
        if (tid < nm) {
            part = rn_load(a, m0 + tid, r, sc, grp);
            thr_j = a.thr[grp];
        }
        const bool live = part && rn_live(r);
        const uint64_t pmask = __ballot(part), lmask = __ballot(live);
        int rank = 0;
        for (int j = 0; j < nm; ++j) {                          // (uniform j: two readlanes, no LDS)
            const double sj = cm3d_readlane_t(sc, j);
            if ((pmask >> j) & 1) rank += (sj > sc || (sj == sc && j > tid)) ? 1 : 0;
        }
        const int nv = (int)__popcll(pmask);
        uint64_t sup = 0;
        for (int rr = 0; rr < nv; ++rr) {
            const uint64_t sel = __ballot(part && rank == rr);
            if (!sel) continue;                                 // (NaN scores: ranks that nobody holds)
            const int i = (int)__builtin_ctzll(sel);
            if (((sup >> i) & 1) || !((lmask >> i) & 1)) continue;
            const bool cand = live && rank > rr && !((sup >> tid) & 1) && (a.class_agnostic || grp == __builtin_amdgcn_readlane(grp, i));
            if (!__ballot(cand)) continue;
            double ki[6];
#pragma unroll
            for (int q = 0; q < 6; ++q) ki[q] = cm3d_readlane_t(r[q], i);
            bool hit = false;
            if (cand) hit = rn_measure<MEASURE>(ki, r) > thr_j;
            sup |= __ballot(hit);
        }
        if (tid < nm) rn_store(a, m0 + tid, part && !((sup >> tid) & 1));
        return;
    }
    // ---- more than 64 boxes: records in LDS, in rank order
    const int cap8 = (min(a.cap, RN_MAX) + 7) & ~7;
    double *const s_r = s_rn;                                   // [6][cap8], by rank
    double *const s_sc = s_r + 6 * cap8, *const s_thr = s_sc + cap8;        // score by box; threshold by rank
    int *const s_grp = reinterpret_cast<int *>(s_thr + cap8), *const s_rank = s_grp + cap8, *const s_at = s_rank + cap8;   // group by rank; rank by box; box by rank
    unsigned char *const s_sup = reinterpret_cast<unsigned char *>(s_at + cap8), *const s_live = s_sup + cap8;             // by rank
    for (int k = tid; k < nm; k += nt) {
        // (the score alone first: the ranks need every box's; a box that takes no part gets NaN there and compares false with everyone)
        double r[6], sc; int grp;
        const bool part = rn_load(a, m0 + k, r, sc, grp);
        s_sc[k] = part ? sc : NAN;
        s_rank[k] = part ? 0 : -1;
        s_at[k] = -1; s_sup[k] = 0; s_live[k] = 0;
    }
    __syncthreads();
    for (int k = tid; k < nm; k += nt) {
        if (s_rank[k] < 0) continue;
        const double sk = s_sc[k];
        int rank = 0;
        for (int j = 0; j < nm; ++j) {
            const double sj = s_sc[j];                          // (NaN: a box that takes no part, or a NaN score -- counted by nobody)
            rank += (sj > sk || (sj == sk && j > k)) ? 1 : 0;
        }
        s_rank[k] = rank;                                       // rank < number of boxes that take part <= nm
        double r[6], sc; int grp;
        rn_load(a, m0 + k, r, sc, grp);
#pragma unroll
        for (int q = 0; q < 6; ++q) s_r[q * cap8 + rank] = r[q];
        s_thr[rank] = a.thr[grp]; s_grp[rank] = grp; s_live[rank] = rn_live(r) ? 1 : 0;
        s_at[rank] = k;                                         // (two boxes at one rank only with NaN scores: one of them owns it)
    }
    __syncthreads();
    for (int rr = 0; rr < nm; ++rr) {
        // (uniform: every thread reads the same LDS bytes, written before the last barrier)
        if (s_at[rr] < 0 || s_sup[rr] || !s_live[rr]) continue;
        double ki[6];
#pragma unroll
        for (int q = 0; q < 6; ++q) ki[q] = s_r[q * cap8 + rr];
        const int gi = s_grp[rr];
        for (int r2 = rr + 1 + tid; r2 < nm; r2 += nt) {
            if (s_at[r2] < 0 || s_sup[r2] || !s_live[r2]) continue;
            if (!a.class_agnostic && s_grp[r2] != gi) continue;
            double bj[6];
#pragma unroll
            for (int q = 0; q < 6; ++q) bj[q] = s_r[q * cap8 + r2];
            if (rn_measure<MEASURE>(ki, bj) > s_thr[r2]) s_sup[r2] = 1;
        }
        __syncthreads();
    }
    for (int k = tid; k < nm; k += nt) {
        const int rank = s_rank[k];
        rn_store(a, m0 + k, rank >= 0 && s_at[rank] == k && !s_sup[rank]);
    }
}

static int rn_launch(const RnArgs &a, int n_frames, int measure, hipStream_t st)
{
    const int cap = a.cap < RN_MAX ? a.cap : RN_MAX;
    const size_t lds = rn_lds_bytes(cap);
    static bool attr_set = false;
    if (lds > 48 * 1024 && !attr_set) {
        const int most = (int)rn_lds_bytes(RN_MAX);
        if (hipFuncSetAttribute((const void *)k_rotated_nms<0>, hipFuncAttributeMaxDynamicSharedMemorySize, most) != hipSuccess ||
            hipFuncSetAttribute((const void *)k_rotated_nms<1>, hipFuncAttributeMaxDynamicSharedMemorySize, most) != hipSuccess)
            return CM3D_ERR_LAUNCH;
        attr_set = true;
    }
    const int threads = cap <= 64 ? 64 : RN_THREADS;
    if (measure == 0) hipLaunchKernelGGL(k_rotated_nms<0>, dim3(n_frames), dim3(threads), lds, st, a);
    else hipLaunchKernelGGL(k_rotated_nms<1>, dim3(n_frames), dim3(threads), lds, st, a);
    CM3D_CHECK_LAUNCH();
    return CM3D_OK;
}

extern "C" int cm3d_rotated_nms(const double *rec, const double *score, const int32_t *group, const int32_t *frame_off, int32_t n_frames,
                                const double *thr, int32_t n_groups, int32_t measure, int32_t class_agnostic, int32_t *keep,
                                cm3d_stream_t stream)
{
    if (!rec || !score || !group || !frame_off || !thr || !keep) return CM3D_ERR_ARG;
    if (n_frames <= 0 || n_groups <= 0 || (measure != 0 && measure != 1)) return CM3D_ERR_ARG;
    RnArgs a = {};
    a.rec = rec; a.score = score; a.group = group; a.keep = keep; a.off = frame_off; a.thr = thr; a.n_groups = n_groups;
    a.class_agnostic = class_agnostic ? 1 : 0; a.cap = RN_MAX; a.src = RN_SRC_REC;
    return rn_launch(a, n_frames, measure, (hipStream_t)stream);
}

extern "C" int cm3d_box_rotated_nms(double *box, int32_t *flags, const int32_t *mask_off, int32_t n_frames, int32_t n_masks,
                                    const int32_t *class_id, const double *prior_wlh, const int32_t *nms_group, int32_t n_classes,
                                    const double *thr, int32_t n_groups, int32_t measure, int32_t class_agnostic, int32_t waymo,
                                    int32_t max_masks_per_frame, cm3d_stream_t stream)
{
    if (!box || !flags || !mask_off || !class_id || !prior_wlh || !nms_group || !thr) return CM3D_ERR_ARG;
    if (n_frames <= 0 || n_masks <= 0 || n_classes <= 0 || n_groups <= 0 || max_masks_per_frame <= 0) return CM3D_ERR_ARG;
    if (measure != 0 && measure != 1) return CM3D_ERR_ARG;
    RnArgs a = {};
    a.box = box; a.flags = flags; a.prior_wlh = prior_wlh; a.nms_group = nms_group; a.n_classes = n_classes; a.off = mask_off; a.thr = thr;
    a.n_groups = n_groups; a.class_agnostic = class_agnostic ? 1 : 0; a.cap = max_masks_per_frame; a.src = waymo ? RN_SRC_WAYMO : RN_SRC_NUSC;
    return rn_launch(a, n_frames, measure, (hipStream_t)stream);
}
