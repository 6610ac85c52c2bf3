// Box height and z from the in-mask points (opt-in): cm3d_box_vertical of include/cm3d_hip.h, which states the rule;
// cm3d_amd/boxvertical.py is the host statement, to the bit.  Two order statistics of every list's z, then one lane per mask judges
// the seen extent against the class's prior height and rewrites column 2 of the box.
//   k_box_vertical  workgroups of VT_WAVES waves, VT_WAVES masks each.
//     lane route    a list of up to VT_LANE_MAX points sits one point per lane of its mask's wave: 32 ballots over the key bits, most
//                   significant first, narrow the candidate lanes of both order statistics at once.  No LDS, no barrier.
//     block route   a longer list is selected by all the waves of the workgroup together, one such list after the other: a radix select
//                   over four 8-bit digits, most significant first, with integer LDS counters (ds_add of ones: the counts do not depend
//                   on the order of the adds), both order statistics in the same passes.  The first pass reads the list, tests it for
//                   non-finite values and, up to VT_LDS_KEYS points, stages the keys in LDS; a longer list is read again from memory
//                   in each later pass.  Four waves walk a long list, not one: one wave's walk of the longest list would set the tail.
//     apply         the lane that holds a mask's two values, float64 without a library call.
// Per point one 4-byte load of column 2 (the memory system moves the whole 64-byte lines: all 16 bytes of a row cross it).
// Every offset read from `off` is clamped into [0, idx_cap] first (vt_range): nothing at or beyond idx_cap is read whatever the offsets
// hold; outputs are written for masks below n_masks only.  Plain stores, no global atomic, no allocation.
#include "common.h"

#define VT_WAVES 4
#define VT_THREADS (64 * VT_WAVES)
#define VT_LANE_MAX CM3D_VERT_LANE_MAX
#define VT_LDS_KEYS CM3D_VERT_LDS_KEYS
static_assert(VT_LANE_MAX == 64, "the lane route holds one point per lane");
static_assert(VT_THREADS == 256, "the block route's scan gives every thread one of the 256 counters");

struct VtRange { int lo, n; };
static __device__ __forceinline__ VtRange vt_range(const int32_t *off, int m, int idx_cap)
{
    int lo = off[m], hi = off[m + 1];
    lo = lo < 0 ? 0 : (lo > idx_cap ? idx_cap : lo);
    hi = hi < lo ? lo : (hi > idx_cap ? idx_cap : hi);
    return VtRange{lo, hi - lo};
}

static __device__ __forceinline__ bool vt_finite(float v) { return fabsf(v) <= 3.402823466e38f; }      // (false for NaN)
static __device__ __forceinline__ bool vt_finite(double v) { return fabs(v) < INFINITY; }
static __device__ __forceinline__ uint32_t vt_key(float z)
{
    const uint32_t b = __float_as_uint(z);
    return b ^ ((b >> 31) ? 0xFFFFFFFFu : 0x80000000u);
}
static __device__ __forceinline__ float vt_value(uint32_t k) { return __uint_as_float(k ^ ((k >> 31) ? 0x80000000u : 0xFFFFFFFFu)); }

struct VtOut {
    double *box;
    const int32_t *flags;
    const double *prior_wlh;
    int n_classes;
    double lo, hi;
    double *vert_z, *vert_h;
    int32_t *vert_src, *vert_status;
    double *vert_entry_z;
};

// one lane per mask: the status and the two values out, then the rule's table
static __device__ __forceinline__ void vt_apply(const VtOut &o, int m, int status, float fzb, float fzt)
{
    const double zb = status == 0 ? (double)fzb : 0.0, zt = status == 0 ? (double)fzt : 0.0;
    double *const b = o.box + (size_t)m * CM3D_BOX_STRIDE;
    const int fl = o.flags[m];
    const double ez = b[2], b8 = b[8];
    const int cls = b8 >= 0.0 && b8 < (double)o.n_classes ? (int)b8 : 0;             // what cm3d_box_place reads of the record
    const double h0 = o.prior_wlh[3 * cls + 2];
    o.vert_status[m] = status;
    o.vert_z[2 * (size_t)m] = zb, o.vert_z[2 * (size_t)m + 1] = zt;
    o.vert_entry_z[m] = ez;
    double h = h0;
    int src = 0;
    if ((fl & 1) && status == 0 && vt_finite(h0) && h0 > 0.0) {
        const double ext = zt - zb, r = ext / h0;
        if (r < o.lo) {
            src = 2;
            b[2] = zt - (h0 * 0.5);
        } else if (r <= o.hi) {
            src = 1, h = ext;
            b[2] = zb + (ext * 0.5);
        }
    }
    o.vert_h[m] = h;
    o.vert_src[m] = src;
}

__global__ __launch_bounds__(VT_THREADS) void k_box_vertical(const float *__restrict__ xyz, const int32_t *__restrict__ off, int n_masks,
                                                             int idx_cap, double q_bot, double q_top, int min_points, VtOut o)
{
    __shared__ uint32_t s_key[VT_LDS_KEYS];
    __shared__ int s_hist[2][256];
    __shared__ int s_part[2][VT_WAVES];
    __shared__ int s_sel[2][2];                  // per order statistic: the digit, and the rank inside it
    const int t = threadIdx.x, lane = cm3d_lane(), wave = t >> 6;
    const int base = blockIdx.x * VT_WAVES;

    // ---- lane route: the wave's own mask (m and n are the same in every lane of the wave)
    {
        const int m = base + wave;
        const VtRange r = m < n_masks ? vt_range(off, m, idx_cap) : VtRange{0, VT_LANE_MAX + 1};
        const int n = r.n;
        if (n <= VT_LANE_MAX) {
            int status = n == 0 ? 2 : n < min_points ? 1 : 0;
            uint32_t key_b = 0, key_t = 0;
            if (status == 0) {
                const float v = lane < n ? xyz[(size_t)(r.lo + lane) * 4 + 2] : 0.0f;      // (the lanes beyond the list hold a finite value)
                if (__ballot(!vt_finite(v)) != 0) {
                    status = 4;
                } else {
                    const uint32_t key = vt_key(v);
                    uint64_t cand_b = n == 64 ? ~0ull : (1ull << n) - 1ull, cand_t = cand_b;
                    int kb = (int)(q_bot * (double)(n - 1)), kt = (int)(q_top * (double)(n - 1));
                    for (int bit = 31; bit >= 0; --bit) {
                        const uint64_t ones = __ballot((key >> bit) & 1u);
                        const uint64_t zb = cand_b & ~ones, zt = cand_t & ~ones;
                        const int nb = __popcll(zb), nt = __popcll(zt);
                        if (kb < nb) cand_b = zb; else kb -= nb, cand_b &= ones, key_b |= 1u << bit;
                        if (kt < nt) cand_t = zt; else kt -= nt, cand_t &= ones, key_t |= 1u << bit;
                    }
                }
            }
            if (lane == 0) vt_apply(o, m, status, vt_value(key_b), vt_value(key_t));
        }
    }

    // ---- block route: the workgroup's longer lists, one after the other (m and n are the same in every thread: each branch that
    //      holds a barrier is taken by all of them)
    for (int j = 0; j < VT_WAVES; ++j) {
        const int m = base + j;
        if (m >= n_masks) break;
        const VtRange r = vt_range(off, m, idx_cap);
        const int n = r.n;
        if (n <= VT_LANE_MAX) continue;
        if (n < min_points) {
            if (t == 0) vt_apply(o, m, 1, 0.0f, 0.0f);
            continue;
        }
        const float *const z = xyz + (size_t)r.lo * 4 + 2;
        const bool staged = n <= VT_LDS_KEYS;
        int kb = (int)(q_bot * (double)(n - 1)), kt = (int)(q_top * (double)(n - 1));
        uint32_t pb = 0, pt = 0;                 // the digits found so far, in place
        bool any_bad = false;
        for (int pass = 0; pass < 4; ++pass) {
            const int shift = 24 - 8 * pass;
            s_hist[0][t] = 0, s_hist[1][t] = 0;
            __syncthreads();
            int bad = 0;
            if (pass == 0) {
                for (int i = t; i < n; i += VT_THREADS) {
                    const float v = z[(size_t)i * 4];
                    bad |= !vt_finite(v);
                    const uint32_t key = vt_key(v);
                    if (staged) s_key[i] = key;
                    atomicAdd(&s_hist[0][key >> 24], 1);
                    atomicAdd(&s_hist[1][key >> 24], 1);
                }
                if (__syncthreads_or(bad)) {
                    any_bad = true;
                    break;
                }
            } else {
                const uint32_t ub = pb >> (shift + 8), ut = pt >> (shift + 8);
                for (int i = t; i < n; i += VT_THREADS) {
                    const uint32_t key = staged ? s_key[i] : vt_key(z[(size_t)i * 4]);
                    const uint32_t up = key >> (shift + 8);
                    const int d = (int)((key >> shift) & 255u);
                    if (up == ub) atomicAdd(&s_hist[0][d], 1);
                    if (up == ut) atomicAdd(&s_hist[1][d], 1);
                }
                __syncthreads();
            }
            // the digit whose counter range holds the rank: an exclusive scan over the 256 counters, one per thread
            const int cb = s_hist[0][t], ct = s_hist[1][t];
            const int ib = cm3d_wave_incl_scan(cb), it = cm3d_wave_incl_scan(ct);
            if (lane == 63) s_part[0][wave] = ib, s_part[1][wave] = it;
            __syncthreads();
            int eb = ib - cb, et = it - ct;
            for (int w = 0; w < wave; ++w) eb += s_part[0][w], et += s_part[1][w];
            if (eb <= kb && kb < eb + cb) s_sel[0][0] = t, s_sel[0][1] = kb - eb;
            if (et <= kt && kt < et + ct) s_sel[1][0] = t, s_sel[1][1] = kt - et;
            __syncthreads();
            pb |= (uint32_t)s_sel[0][0] << shift, kb = s_sel[0][1];
            pt |= (uint32_t)s_sel[1][0] << shift, kt = s_sel[1][1];
        }
        if (t == 0) vt_apply(o, m, any_bad ? 4 : 0, vt_value(pb), vt_value(pt));
    }
}

extern "C" int cm3d_box_vertical(const float *xyz, const int32_t *off, int32_t n_masks, int32_t idx_cap, double *box, const int32_t *flags,
                                 const double *prior_wlh, int32_t n_classes, double q_bot, double q_top, int32_t min_points, double lo,
                                 double hi, double *vert_z, double *vert_h, int32_t *vert_src, int32_t *vert_status, double *vert_entry_z,
                                 cm3d_stream_t stream)
{
    if (!(q_bot >= 0.0 && q_bot <= q_top && q_top <= 1.0)) return CM3D_ERR_ARG;                   // (a NaN fails a comparison)
    if (min_points < 1 || !(lo > 0.0 && lo <= hi && hi < INFINITY)) return CM3D_ERR_ARG;
    if (n_masks < 0 || idx_cap < 0 || n_classes < 0) return CM3D_ERR_ARG;
    if (n_masks == 0) return CM3D_OK;
    if (n_classes == 0 || (!xyz && idx_cap > 0) || !off || !box || !flags || !prior_wlh || !vert_z || !vert_h || !vert_src || !vert_status ||
        !vert_entry_z)
        return CM3D_ERR_ARG;
    const VtOut o{box, flags, prior_wlh, n_classes, lo, hi, vert_z, vert_h, vert_src, vert_status, vert_entry_z};
    hipLaunchKernelGGL(k_box_vertical, dim3((n_masks + VT_WAVES - 1) / VT_WAVES), dim3(VT_THREADS), 0, (hipStream_t)stream, xyz, off, n_masks,
                       idx_cap, q_bot, q_top, min_points, o);
    CM3D_CHECK_LAUNCH();
    return CM3D_OK;
}
