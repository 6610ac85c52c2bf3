// nuScenes detection matching (the greedy loop of eval_custom.py's accumulate_object_class / accumulate_with_recall, restricted to
// one sample at a time; host side and the rules: cm3d_amd/nusc_eval.py) for every alpha of the SAM3D fusion grid search.
//
// Input: "groups" = one sample (class-agnostic scoring) or one (sample, class), each with its candidates in file order and its
// ground truth.  Per alpha a candidate is active or not and has a float64 score (fusion.fuse):
//   kind 0 unmatched prediction: score p           kind 1 unmatched SAM3D box: score clip(s * alpha, 0, 1)
//   kind 2 prediction of a pair: score p, active iff !(s * alpha > p)     kind 3 its SAM3D box: clip(s * alpha, 0, 1), iff s * alpha > p
// Per (group, alpha, threshold) the active candidates are walked by descending score, equal scores by descending position, and
// each takes the nearest ground-truth box nobody took before it (d2 = dx * dx + dy * dy in float64, lowest index on equal d2) if
// d2 < th * th.  The output is integer: which thresholds a candidate is a true positive at, and which box it took.
//
// Launch: k_nusc_match, one wave per (group, slice of alphas).  Ground truth j sits in lane j % 64, slot j / 64, coordinates in
// registers.  Per alpha: the candidates' score keys into LDS, rank sort, the permutation into LDS, then the walk in chunks of 64
// ranks (lane l fetches the coordinates of rank base + l; the wave reads them lane by lane).  A candidate's d2 row is computed
// once and serves the T thresholds, each with its own taken mask.
#include "common.h"

#define NM_SLOTS (CM3D_NUSC_MAX_GT / 64)
#define NM_TARGET_WAVES 8192             // the alphas of a call are cut into slices until about this many waves run

static_assert(NM_SLOTS * 64 == CM3D_NUSC_MAX_GT && NM_SLOTS * CM3D_NUSC_MAX_TH <= 32, "taken bits of a lane fit one word");
static_assert(CM3D_NUSC_MAX_CAND <= 65536, "the permutation is 16-bit");

static __device__ __forceinline__ void nm_wave_sync()        // LDS written by some lanes of the wave is read by others
{
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}

// ascending key = descending score; -0 equals +0; ~0 is kept for "inactive"
static __device__ __forceinline__ unsigned long long nm_score_key(double score)
{
    const unsigned long long b = (unsigned long long)__double_as_longlong(score + 0.0);
    const unsigned long long k = ~(b ^ ((b >> 63) ? ~0ull : 0x8000000000000000ull));
    return k == ~0ull ? ~0ull - 1 : k;
}

static __device__ __forceinline__ unsigned long long nm_key(int kind, double p, double s, double alpha)
{
    const double prod = s * alpha;
    const bool sam = prod > p;
    const bool active = kind == 0 || kind == 1 || (kind == 2 && !sam) || (kind == 3 && sam);
    const double clipped = prod < 0.0 ? 0.0 : (prod > 1.0 ? 1.0 : prod);
    return active ? nm_score_key((kind == 0 || kind == 2) ? p : clipped) : ~0ull;
}

__global__ __launch_bounds__(64) void k_nusc_match(const double *__restrict__ cand_xy, const int32_t *__restrict__ cand_kind,
                                                   const double *__restrict__ cand_p, const double *__restrict__ cand_s,
                                                   const int32_t *__restrict__ cand_off, const double *__restrict__ gt_xy,
                                                   const int32_t *__restrict__ gt_off, const double *__restrict__ alphas, int n_alphas,
                                                   int per_slice, const double *__restrict__ dist_th, int T, int64_t n_cand,
                                                   uint8_t *__restrict__ tp_bits, int32_t *__restrict__ match_idx,
                                                   int32_t *__restrict__ status)
{
    __shared__ unsigned long long s_key[CM3D_NUSC_MAX_CAND];
    __shared__ unsigned short s_perm[CM3D_NUSC_MAX_CAND];
    const int g = blockIdx.x, slice = blockIdx.y, lane = threadIdx.x;
    const int c0 = cand_off[g], g0 = gt_off[g];
    const int C = cand_off[g + 1] - c0, G = gt_off[g + 1] - g0;
    if (C < 0 || G < 0 || C > CM3D_NUSC_MAX_CAND || G > CM3D_NUSC_MAX_GT) {
        if (slice == 0 && lane == 0) atomicOr(status, 1);
        return;
    }
    const int a_lo = slice * per_slice;
    const int a_hi = a_lo + per_slice < n_alphas ? a_lo + per_slice : n_alphas;
    if (C == 0 || a_lo >= a_hi) return;

    const double inf = __builtin_huge_val();
    const int n_slots = (G + 63) >> 6;
    double gx[NM_SLOTS], gy[NM_SLOTS];
#pragma unroll
    for (int k = 0; k < NM_SLOTS; ++k) {
        const int j = k * 64 + lane;
        gx[k] = gy[k] = 0.0;
        if (j < G) { gx[k] = gt_xy[2 * (int64_t)(g0 + j)]; gy[k] = gt_xy[2 * (int64_t)(g0 + j) + 1]; }
    }
    double th2[CM3D_NUSC_MAX_TH];
#pragma unroll
    for (int t = 0; t < CM3D_NUSC_MAX_TH; ++t) {
        const double th = t < T ? dist_th[t] : 0.0;
        th2[t] = th * th;
    }
    // the first 64 candidates' records stay in registers over the alphas; later chunks are read again per alpha
    int kind0 = -1;
    double p0 = 0.0, s0 = 0.0;
    if (lane < C) { kind0 = cand_kind[c0 + lane]; p0 = cand_p[c0 + lane]; s0 = cand_s[c0 + lane]; }

    for (int a = a_lo; a < a_hi; ++a) {
        const double alpha = alphas[a];
        uint8_t *__restrict__ out_bits = tp_bits + (int64_t)a * n_cand + c0;
        int32_t *__restrict__ out_idx = match_idx ? match_idx + ((int64_t)a * n_cand + c0) * T : nullptr;
        // keys; an inactive candidate's output is written here
        int n_active = 0;
        for (int base = 0; base < C; base += 64) {
            const int c = base + lane;
            if (c < C) {
                const unsigned long long key = base == 0 ? nm_key(kind0, p0, s0, alpha)
                                                         : nm_key(cand_kind[c0 + c], cand_p[c0 + c], cand_s[c0 + c], alpha);
                s_key[c] = key;
                const bool active = key != ~0ull;
                n_active += active;
                if (!active || G == 0) {
                    out_bits[c] = active ? 0x80 : 0;
                    if (out_idx)
                        for (int t = 0; t < T; ++t) out_idx[(int64_t)c * T + t] = -1;
                }
            }
        }
        if (G == 0) continue;                    // no ground truth: the active bits are written, nothing can match
        n_active = cm3d_wave_sum(n_active);
        nm_wave_sync();
        // rank = number of candidates walked before this one: smaller key, or the same key at a higher position
        for (int base = 0; base < C; base += 64) {
            const int c = base + lane;
            const unsigned long long key = c < C ? s_key[c] : ~0ull;
            int rank = 0;
            for (int j = 0; j < C; ++j) {
                const unsigned long long kj = s_key[j];
                rank += (kj < key) | ((kj == key) & (j > c));
            }
            if (key != ~0ull) s_perm[rank] = (unsigned short)c;        // active: rank < n_active <= C
        }
        nm_wave_sync();
        // the walk
        unsigned taken = 0;                       // bit t * NM_SLOTS + k: this lane's box of slot k is taken at threshold t
        for (int base = 0; base < n_active; base += 64) {
            const int n_here = n_active - base < 64 ? n_active - base : 64;
            int my_c = 0;
            double my_x = 0.0, my_y = 0.0;
            if (lane < n_here) {
                my_c = s_perm[base + lane];
                my_x = cand_xy[2 * (int64_t)(c0 + my_c)];
                my_y = cand_xy[2 * (int64_t)(c0 + my_c) + 1];
            }
            int my_bits = 0x80;
            int my_idx[CM3D_NUSC_MAX_TH];
#pragma unroll
            for (int t = 0; t < CM3D_NUSC_MAX_TH; ++t) my_idx[t] = -1;
            for (int i = 0; i < n_here; ++i) {
                const double cx = cm3d_readlane_t(my_x, i), cy = cm3d_readlane_t(my_y, i);
                double d2[NM_SLOTS];
#pragma unroll
                for (int k = 0; k < NM_SLOTS; ++k) {
                    d2[k] = inf;
                    if (k < n_slots) {
                        const double dx = cx - gx[k], dy = cy - gy[k];
                        const double v = dx * dx + dy * dy;
                        d2[k] = k * 64 + lane < G ? v : inf;
                    }
                }
#pragma unroll
                for (int t = 0; t < CM3D_NUSC_MAX_TH; ++t) {
                    if (t >= T) break;
                    double best = inf;
                    int bj = 0x7fffffff;
#pragma unroll
                    for (int k = 0; k < NM_SLOTS; ++k)
                        if (k < n_slots && !((taken >> (t * NM_SLOTS + k)) & 1u) && d2[k] < best) { best = d2[k]; bj = k * 64 + lane; }
                    const Cm3dDistIdx r = cm3d_wave_argmin(best, bj);
                    const bool hit = r.s < th2[t];
                    if (hit && lane == (r.j & 63)) taken |= 1u << (t * NM_SLOTS + (r.j >> 6));
                    if (hit && lane == i) { my_bits |= 1 << t; my_idx[t] = r.j; }
                }
            }
            if (lane < n_here) {
                out_bits[my_c] = (uint8_t)my_bits;
                if (out_idx) {
#pragma unroll
                    for (int t = 0; t < CM3D_NUSC_MAX_TH; ++t)
                        if (t < T) out_idx[(int64_t)my_c * T + t] = my_idx[t];
                }
            }
        }
        nm_wave_sync();                          // the next alpha overwrites the keys and the permutation
    }
}

extern "C" int64_t cm3d_nusc_match_workspace_bytes(int32_t n_groups, int64_t n_cand, int32_t n_alphas)
{
    (void)n_groups; (void)n_cand; (void)n_alphas;
    return 0;                                    // keys and permutation live in LDS
}

extern "C" int cm3d_nusc_match(const double *cand_xy, const int32_t *cand_kind, const double *cand_p, const double *cand_s,
                               const int32_t *cand_off, const double *gt_xy, const int32_t *gt_off, int32_t n_groups, int64_t n_cand,
                               const double *alphas, int32_t n_alphas, const double *dist_th, int32_t n_th, uint8_t *tp_bits,
                               int32_t *match_idx, int32_t *status, void *workspace, int64_t workspace_bytes, cm3d_stream_t stream)
{
    (void)workspace;
    if (!cand_off || !gt_off || !alphas || !dist_th || !status || n_groups < 0 || n_cand < 0 || n_alphas < 1 ||
        n_alphas > CM3D_NUSC_MAX_ALPHAS || n_th < 1 || n_th > CM3D_NUSC_MAX_TH)
        return CM3D_ERR_ARG;
    if (n_cand > 0 && (!cand_xy || !cand_kind || !cand_p || !cand_s || !gt_xy || !tp_bits)) return CM3D_ERR_ARG;
    if (workspace_bytes < cm3d_nusc_match_workspace_bytes(n_groups, n_cand, n_alphas)) return CM3D_ERR_WORKSPACE;
    if (n_groups == 0 || n_cand == 0) return CM3D_OK;
    // few groups: more slices of fewer alphas, so that the device fills; many groups: one wave walks all alphas of its group
    int slices = NM_TARGET_WAVES / n_groups;
    slices = slices < 1 ? 1 : (slices > n_alphas ? n_alphas : slices);
    const int per_slice = (n_alphas + slices - 1) / slices;
    slices = (n_alphas + per_slice - 1) / per_slice;
    hipLaunchKernelGGL(k_nusc_match, dim3(n_groups, slices), dim3(64), 0, (hipStream_t)stream, cand_xy, cand_kind, cand_p, cand_s, cand_off,
                       gt_xy, gt_off, alphas, n_alphas, per_slice, dist_th, n_th, n_cand, tp_bits, match_idx, status);
    CM3D_CHECK_LAUNCH();
    return CM3D_OK;
}
