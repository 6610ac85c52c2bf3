// The greedy class-aware circle NMS of one frame, one wave: the LDS form (nms_phase) and the register form (nms_regs).  Shared by
// k_box_nms and k_circle_nms (boxes.hip) and k_box_place (place.hip): one statement of the rule, reference circle_nms
// src/nuscenes/2d_to_3d.py:309-332.
#ifndef CM3D_CIRCLE_NMS_H
#define CM3D_CIRCLE_NMS_H
#include "common.h"

#define BN_MAX CM3D_MAX_MASKS_PER_FRAME

// Greedy class-aware circle NMS over the LDS arrays of one frame (one wave).
static __device__ __forceinline__ void nms_phase(int nm, int lane_id, const double *__restrict__ nms_thr, const double *s_x,
                                                 const double *s_y, const double *s_s, const int *s_lab, int *s_order,
                                                 const unsigned char *s_valid, unsigned char *s_sup, unsigned char *s_keep)
{
    __syncthreads();
    // order: descending score, ties by descending index (pinned tie-break, SURVEY hard part 4)
    int nv = 0;
    for (int k = 0; k < nm; ++k) nv += s_valid[k];
    for (int k = lane_id; k < nm; k += 64) {
        if (!s_valid[k]) continue;
        int rank = 0;
        const double sk = s_s[k];
        for (int j = 0; j < nm; ++j) {
            if (!s_valid[j]) continue;
            const double sj = s_s[j];
            rank += (sj > sk || (sj == sk && j > k)) ? 1 : 0;
        }
        s_order[rank] = k;
    }
    __syncthreads();
    for (int r = 0; r < nv; ++r) {
        const int i = s_order[r];
        if (!s_sup[i]) {            // uniform: every lane reads the same LDS word
            if (lane_id == 0) s_keep[i] = 1;
            const double xi = s_x[i], yi = s_y[i];
            const int li = s_lab[i];
            for (int r2 = r + 1 + lane_id; r2 < nv; r2 += 64) {
                const int j = s_order[r2];
                if (s_sup[j]) continue;
                const double dx = xi - s_x[j], dy = yi - s_y[j];
                const double dist = dx * dx + dy * dy;
                if (dist <= nms_thr[s_lab[j]] && s_lab[j] == li) s_sup[j] = 1;
            }
        }
        __syncthreads();
    }
}

// One lane of a wave reads a double of lane `src` (wave-uniform).
static __device__ __forceinline__ double bn_readlane(double v, int src)
{
    return __hiloint2double(__builtin_amdgcn_readlane(__double2hiint(v), src), __builtin_amdgcn_readlane(__double2loint(v), src));
}

// The same greedy pass as nms_phase for a frame of nm <= 64 masks, lane k = mask k (r_valid false in the lanes from nm on): order =
// descending score, ties by descending index; the box of rank r, unless suppressed, is kept and suppresses every later box of its group
// within that box's own threshold r_thr = nms_thr[r_lab].  Same comparisons on the same float64 values, so the same flags.  Returns the
// kept masks, bit k = mask k.  Collective: call with all 64 lanes.
static __device__ __forceinline__ uint64_t nms_regs(int nm, int lane_id, bool r_valid, double r_x, double r_y, double r_s, int r_lab,
                                                    double r_thr)
{
    const uint64_t vmask = __ballot(r_valid);
    int rank = 0;
    for (int j = 0; j < nm; ++j) {                       // (uniform j: two readlanes, no LDS)
        const double sj = bn_readlane(r_s, j);
        if ((vmask >> j) & 1) rank += (sj > r_s || (sj == r_s && j > lane_id)) ? 1 : 0;
    }
    const int nv = (int)__popcll(vmask);
    uint64_t sup = 0, keep = 0;
    for (int r = 0; r < nv; ++r) {
        const uint64_t sel = __ballot(r_valid && rank == r);
        if (!sel) continue;                              // (NaN scores: ranks that nobody holds)
        const int i = (int)__builtin_ctzll(sel);
        if ((sup >> i) & 1) continue;
        keep |= 1ull << i;
        const double xi = bn_readlane(r_x, i), yi = bn_readlane(r_y, i);
        const int li = __builtin_amdgcn_readlane(r_lab, i);
        const double dx = xi - r_x, dy = yi - r_y;
        const double dist = dx * dx + dy * dy;
        sup |= __ballot(r_valid && rank > r && dist <= r_thr && r_lab == li);
    }
    return keep;
}

// LDS of a one-wave launch for frames of up to `cap` masks: nms_phase's arrays one behind the other; none for cap <= 64 (a wave's registers)
static inline size_t bn_lds_bytes(int cap) { return cap <= 64 ? 0 : (size_t)((cap + 7) & ~7) * (3 * sizeof(double) + 2 * sizeof(int) + 3); }
#endif
