// a18 (KITTI): yaw of the oriented bounding box of every mask's in-mask points -- reference src/kitti/2d_to_3d.py:855-876 (Open3D's
// get_oriented_bounding_box: PCA of the convex-hull vertices) and the as_euler('zyx')[0] of :1524; the host restatement is
// cm3d_amd.kitti.obb_yaw / obb_canonical.
//
// One single-wave workgroup per mask, everything that decides a result in float64 on coordinates shifted to the list's AABB centre.
//  1. Hull vertices = the extreme points of the list, by an incremental (beneath-beyond / Quickhull-style) construction:
//     - the initial simplex is taken from extreme points (lexicographic minimum and maximum, then the extreme points along the
//       direction away from their line and away from their plane); a flat, collinear or single-point list has no simplex -> status 2;
//     - every point outside the current hull (distance above the outside tolerance, Qhull-like: OB_EPS_K * DBL_EPSILON * the list's
//       half extent) belongs to one facet it lies above (its "owner"); the others are dropped for good;
//     - each step takes the facet that owns the first live point and adds the point EXTREME along that facet's normal (ties broken
//       along a fixed generic direction, then by the lowest position): an exposed face's extreme point is a vertex of the hull of the
//       whole list, so points in the relative interior of a face or an edge (box surfaces, duplicated rows) never become vertices;
//     - the facets the new point sees are removed, the horizon edges (edges of a visible facet whose reverse is no visible facet's
//       edge) are joined to the point, and the points the removed facets owned are handed to the new facets or dropped.
//     Facets live in LDS (OB_FCAP) while the hull is small; a larger hull moves to the list's own region of the workspace: 3 n + 64
//     facets for a list of n points at facet 3 hit_off[m] + 64 m -- room for any hull of the list (a triangulated hull of h vertices has
//     2 h - 4 facets, a horizon at most h edges, and every vertex is a point of the list), placed by the offsets alone: no allocator,
//     nothing that depends on the order in which masks run.  The live points live in the workspace (8 bytes per list position) until
//     they fit in LDS (OB_LCAP).  Every workspace offset is checked: a list whose visible set or horizon exceeds OB_VCAP in one step
//     (or whose construction degenerates numerically) gets status 4 and NaN results, nothing is written out of range.
//  2. Mean and population covariance of the vertices (ascending list position per lane, lanes combined in a fixed order: the same
//     result on every run), 3x3 cyclic Jacobi, the canonical eigenvector signs (each unit eigenvector negated so that its component of
//     largest magnitude is positive, the first one on a tie), columns by descending eigenvalue, det fix, the axis re-ordering by AABB
//     extent (stable), det fix, and scipy's quaternion-based as_euler('zyx') including its gimbal-lock branch.
#include "common.h"

#include <float.h>
#include <math.h>

#define OB_THREADS 64
#define OB_FCAP 256          // facets in LDS (12 KiB)
#define OB_LCAP 512          // live points in LDS (4 KiB)
#define OB_VCAP 512          // visible facets / horizon edges per step
#define OB_EPS_K 16.0        // outside tolerance = OB_EPS_K * DBL_EPSILON * half extent of the list
#define OB_FSLACK 64         // facets per list beyond 3 n in the list's workspace region

#define OB_ST_FIT 0
#define OB_ST_SKIP 1
#define OB_ST_FLAT 2
#define OB_ST_OVERFLOW 4

struct ObFacet {
    double nx, ny, nz, off;   // unit outward normal, offset: distance of p = n.p - off
    int v0, v1, v2;           // list positions of the corners (v0 < 0: removed)
    int aux;                  // new slot during a compaction
};

struct ObKey {               // lexicographic maximum of (a, b, c), then the lowest position
    double a, b, c;
    int pos, pad;
};

static __device__ __forceinline__ ObKey ob_key_max(ObKey x, ObKey y)
{
    if (y.a != x.a) return y.a > x.a ? y : x;
    if (y.b != x.b) return y.b > x.b ? y : x;
    if (y.c != x.c) return y.c > x.c ? y : x;
    return y.pos < x.pos ? y : x;
}

static __device__ __forceinline__ ObKey ob_wave_key_max(ObKey k)
{
    return cm3d_wave_reduce_t(k, [](ObKey x, ObKey y) { return ob_key_max(x, y); });
}

// fixed generic direction for tie-breaks between points equally far along a facet normal
#define OB_DX 0.2672612419124244
#define OB_DY 0.5345224838248488
#define OB_DZ 0.8017837257372732
static __device__ __forceinline__ double ob_tie(double x, double y, double z) { return OB_DX * x + OB_DY * y + OB_DZ * z; }

struct ObPt { double x, y, z; };

static __device__ __forceinline__ ObPt ob_load(const float4 *__restrict__ xyz, int i, double cx, double cy, double cz)
{
    const float4 q = xyz[i];
    return {(double)q.x - cx, (double)q.y - cy, (double)q.z - cz};
}

static __device__ __forceinline__ double ob_dist(const ObFacet &f, const ObPt &p)
{
    return f.nx * p.x + f.ny * p.y + f.nz * p.z - f.off;
}

// plane through a, b, c (counter-clockwise seen from outside); false if the three are (numerically) collinear
static __device__ __forceinline__ bool ob_plane(const ObPt &a, const ObPt &b, const ObPt &c, ObFacet &f)
{
    const double ux = b.x - a.x, uy = b.y - a.y, uz = b.z - a.z;
    const double vx = c.x - a.x, vy = c.y - a.y, vz = c.z - a.z;
    double nx = uy * vz - uz * vy, ny = uz * vx - ux * vz, nz = ux * vy - uy * vx;
    const double len = sqrt(nx * nx + ny * ny + nz * nz);
    if (!(len > 0.0)) return false;
    nx /= len; ny /= len; nz /= len;
    f.nx = nx; f.ny = ny; f.nz = nz;
    f.off = nx * a.x + ny * a.y + nz * a.z;
    return true;
}

// ---- scipy 1.15 Rotation.from_matrix(R).as_euler('zyx')[0] (extrinsic z-y-x), restated: Markley's matrix -> quaternion, then the
// quaternion -> Euler method of Bernardes & Viollet with scipy's gimbal-lock branch (|second angle| or |second angle - pi| <= 1e-7:
// third angle set to 0, the first takes the whole rotation).  R row-major.
static __device__ double ob_euler_zyx_yaw(const double *R)
{
    double q[4];
    const double tr = R[0] + R[4] + R[8];
    double dec[4] = {R[0], R[4], R[8], tr};
    int ch = 0;
    for (int k = 1; k < 4; ++k)
        if (dec[k] > dec[ch]) ch = k;                // np.argmax: first maximum
    if (ch != 3) {
        const int i = ch, j = (i + 1) % 3, k = (j + 1) % 3;
        q[i] = 1.0 - tr + 2.0 * R[i * 3 + i];
        q[j] = R[j * 3 + i] + R[i * 3 + j];
        q[k] = R[k * 3 + i] + R[i * 3 + k];
        q[3] = R[k * 3 + j] - R[j * 3 + k];
    } else {
        q[0] = R[2 * 3 + 1] - R[1 * 3 + 2];
        q[1] = R[0 * 3 + 2] - R[2 * 3 + 0];
        q[2] = R[1 * 3 + 0] - R[0 * 3 + 1];
        q[3] = 1.0 + tr;
    }
    const double nq = sqrt(q[0] * q[0] + q[1] * q[1] + q[2] * q[2] + q[3] * q[3]);
    for (int k = 0; k < 4; ++k) q[k] /= nq;
    // 'zyx' extrinsic: i = 2, j = 1, k = 0, not proper, sign = -1
    const double a = q[3] - q[1], b = q[2] - q[0], c = q[1] + q[3], d = -q[0] - q[2];
    const double ang1 = 2.0 * atan2(hypot(c, d), hypot(a, b));
    const bool case1 = fabs(ang1) <= 1e-7, case2 = fabs(ang1 - M_PI) <= 1e-7;
    const double half_sum = atan2(b, a), half_diff = atan2(d, c);
    double ang0;
    if (!case1 && !case2) ang0 = half_sum - half_diff;
    else if (case1) ang0 = 2.0 * half_sum;
    else ang0 = -2.0 * half_diff;
    if (ang0 < -M_PI) ang0 += 2.0 * M_PI;
    else if (ang0 > M_PI) ang0 -= 2.0 * M_PI;
    return ang0;
}

// ---- PCA box of the vertices -> Rm, yaw (steps 2-6 of the contract in cm3d_hip.h)
static __device__ double ob_fit(const double cov[6], const double size[3], double Rm[9])
{
    // cyclic Jacobi on the symmetric 3x3 (a00 a11 a22 a01 a02 a12)
    double A[3][3] = {{cov[0], cov[3], cov[4]}, {cov[3], cov[1], cov[5]}, {cov[4], cov[5], cov[2]}};
    double V[3][3] = {{1, 0, 0}, {0, 1, 0}, {0, 0, 1}};
    for (int sweep = 0; sweep < 50; ++sweep) {
        const double offd = fabs(A[0][1]) + fabs(A[0][2]) + fabs(A[1][2]);
        if (offd == 0.0) break;
        for (int r = 0; r < 3; ++r) {
            const int p = r == 2 ? 1 : 0, qq = r == 0 ? 1 : 2;
            const double apq = A[p][qq];
            if (fabs(apq) <= 1e-300 || fabs(apq) <= DBL_EPSILON * 1e-3 * (fabs(A[p][p]) + fabs(A[qq][qq]))) {
                A[p][qq] = A[qq][p] = 0.0;
                continue;
            }
            const double theta = (A[qq][qq] - A[p][p]) / (2.0 * apq);
            const double t = (theta >= 0 ? 1.0 : -1.0) / (fabs(theta) + sqrt(theta * theta + 1.0));
            const double c = 1.0 / sqrt(t * t + 1.0), s = t * c;
            for (int k = 0; k < 3; ++k) {            // A <- J^T A J
                const double akp = A[k][p], akq = A[k][qq];
                A[k][p] = c * akp - s * akq;
                A[k][qq] = s * akp + c * akq;
            }
            for (int k = 0; k < 3; ++k) {
                const double apk = A[p][k], aqk = A[qq][k];
                A[p][k] = c * apk - s * aqk;
                A[qq][k] = s * apk + c * aqk;
            }
            A[p][qq] = A[qq][p] = 0.0;
            for (int k = 0; k < 3; ++k) {
                const double vkp = V[k][p], vkq = V[k][qq];
                V[k][p] = c * vkp - s * vkq;
                V[k][qq] = s * vkp + c * vkq;
            }
        }
    }
    // columns by descending eigenvalue (eigh ascending, reversed)
    int ord[3] = {0, 1, 2};
    const double ev[3] = {A[0][0], A[1][1], A[2][2]};
    for (int i = 0; i < 3; ++i)
        for (int j = i + 1; j < 3; ++j)
            if (ev[ord[j]] > ev[ord[i]]) { const int t = ord[i]; ord[i] = ord[j]; ord[j] = t; }
    double E[3][3];                                  // E[col][row]
    for (int cidx = 0; cidx < 3; ++cidx) {
        double v0 = V[0][ord[cidx]], v1 = V[1][ord[cidx]], v2 = V[2][ord[cidx]];
        const double nv = sqrt(v0 * v0 + v1 * v1 + v2 * v2);
        v0 /= nv; v1 /= nv; v2 /= nv;
        // canonical sign: the component of largest magnitude positive (the first on an exact tie)
        int kb = 0;
        double mb = fabs(v0);
        if (fabs(v1) > mb) { kb = 1; mb = fabs(v1); }
        if (fabs(v2) > mb) kb = 2;
        const double big = kb == 0 ? v0 : (kb == 1 ? v1 : v2);
        const double sg = big < 0 ? -1.0 : 1.0;
        E[cidx][0] = sg * v0; E[cidx][1] = sg * v1; E[cidx][2] = sg * v2;
    }
    auto det = [](const double (*C)[3]) {            // det of the matrix whose COLUMNS are C[0], C[1], C[2]
        return C[0][0] * (C[1][1] * C[2][2] - C[2][1] * C[1][2]) - C[1][0] * (C[0][1] * C[2][2] - C[2][1] * C[0][2]) +
               C[2][0] * (C[0][1] * C[1][2] - C[1][1] * C[0][2]);
    };
    if (det(E) < 0) for (int k = 0; k < 3; ++k) E[2][k] = -E[2][k];
    // stable ascending ranks of the extents: Rm = [col rank(z), col rank(y), col rank(x)]
    int rank[3];
    for (int i = 0; i < 3; ++i) {
        int r = 0;
        for (int j = 0; j < 3; ++j) r += (size[j] < size[i]) || (size[j] == size[i] && j < i);
        rank[i] = r;
    }
    double C[3][3];
    for (int k = 0; k < 3; ++k) { C[0][k] = E[rank[2]][k]; C[1][k] = E[rank[1]][k]; C[2][k] = E[rank[0]][k]; }
    if (det(C) < 0) for (int k = 0; k < 3; ++k) C[0][k] = -C[0][k];
    for (int r = 0; r < 3; ++r)
        for (int c = 0; c < 3; ++c) Rm[r * 3 + c] = C[c][r];
    return ob_euler_zyx_yaw(Rm);
}

static __device__ __forceinline__ void ob_write_result(int m, int st, double yaw_v, const double *Rm, double *yaw, int32_t *status, double *rot)
{
    yaw[m] = yaw_v;
    status[m] = st;
    if (rot)
        for (int k = 0; k < 9; ++k) rot[(size_t)m * 9 + k] = Rm[k];
}

__global__ __launch_bounds__(OB_THREADS) void k_obb(const float4 *__restrict__ xyz_all, const int32_t *__restrict__ hit_off, int n_masks,
                                                    int idx_cap, double *__restrict__ yaw, int32_t *__restrict__ status,
                                                    double *__restrict__ rot, uint8_t *__restrict__ vmark, char *__restrict__ ws,
                                                    int64_t n_facets)
{
    __shared__ ObFacet s_fac[OB_FCAP];
    __shared__ int2 s_live[OB_LCAP];
    __shared__ int s_vis[OB_VCAP];
    __shared__ int2 s_hor[OB_VCAP];
    __shared__ double s_part[OB_THREADS][4];
    __shared__ int s_bad;
    const int m = blockIdx.x, lane = threadIdx.x;
    const double qnan = __longlong_as_double(0x7FF8000000000000LL);
    const double nanR[9] = {qnan, qnan, qnan, qnan, qnan, qnan, qnan, qnan, qnan};
    const double eyeR[9] = {1, 0, 0, 0, 1, 0, 0, 0, 1};
    const int o = hit_off[m];
    int n = hit_off[m + 1] - o;
    if (o < 0 || o > idx_cap) n = 0;
    n = max(0, min(n, idx_cap - max(o, 0)));
    if (vmark)
        for (int i = lane; i < n; i += OB_THREADS) vmark[o + i] = 0;
    if (n <= 3) {                                    // :1479-1480
        if (lane == 0) ob_write_result(m, OB_ST_SKIP, qnan, nanR, yaw, status, rot);
        return;
    }
    const float4 *xyz = xyz_all + o;
    int2 *g_live = (int2 *)ws + o;                   // 8 bytes per list position, inside [0, idx_cap)
    // the list's facet region: [3 o + 64 m, 3 (o + n) + 64 (m + 1)), inside [0, n_facets) since o + n <= idx_cap and m < n_masks
    const int64_t g_fac0 = 3 * (int64_t)o + (int64_t)OB_FSLACK * m, g_fcap = 3 * (int64_t)n + OB_FSLACK;
    ObFacet *g_fac = (ObFacet *)(ws + (size_t)idx_cap * sizeof(int2)) + g_fac0;

    // -- AABB (f32 values, exact), centre, tolerance
    float mn[3] = {INFINITY, INFINITY, INFINITY}, mx[3] = {-INFINITY, -INFINITY, -INFINITY};
    for (int i = lane; i < n; i += OB_THREADS) {
        const float4 q = xyz[i];
        mn[0] = fminf(mn[0], q.x); mn[1] = fminf(mn[1], q.y); mn[2] = fminf(mn[2], q.z);
        mx[0] = fmaxf(mx[0], q.x); mx[1] = fmaxf(mx[1], q.y); mx[2] = fmaxf(mx[2], q.z);
    }
    double size[3], ctr[3], half = 0.0;
    for (int k = 0; k < 3; ++k) {
        mn[k] = cm3d_wave_reduce_t(mn[k], [](float a, float b) { return fminf(a, b); });
        mx[k] = cm3d_wave_reduce_t(mx[k], [](float a, float b) { return fmaxf(a, b); });
        size[k] = (double)mx[k] - (double)mn[k];
        ctr[k] = 0.5 * ((double)mn[k] + (double)mx[k]);
        half = fmax(half, 0.5 * size[k]);
    }
    const double cx = ctr[0], cy = ctr[1], cz = ctr[2];
    const double eps = OB_EPS_K * DBL_EPSILON * half;
    if (!(half > 0.0) || !isfinite(half)) {          // a single distinct point (or non-finite input): Qhull raises -> identity box
        if (lane == 0) ob_write_result(m, OB_ST_FLAT, 0.0, eyeR, yaw, status, rot);
        return;
    }

    // -- initial simplex from extreme points
    auto argmax_pts = [&](auto keyf) {
        ObKey best = {-INFINITY, -INFINITY, -INFINITY, 0x7FFFFFFF, 0};
        for (int i = lane; i < n; i += OB_THREADS) {
            const ObPt p = ob_load(xyz, i, cx, cy, cz);
            ObKey k = keyf(p);
            k.pos = i;
            best = ob_key_max(best, k);
        }
        return ob_wave_key_max(best);
    };
    const ObKey k0 = argmax_pts([](const ObPt &p) { return ObKey{-p.x, -p.y, -p.z, 0, 0}; });
    const ObKey k1 = argmax_pts([](const ObPt &p) { return ObKey{p.x, p.y, p.z, 0, 0}; });
    const ObPt P0 = {-k0.a, -k0.b, -k0.c}, P1 = {k1.a, k1.b, k1.c};
    const double ux = P1.x - P0.x, uy = P1.y - P0.y, uz = P1.z - P0.z, uu = ux * ux + uy * uy + uz * uz;
    // farthest from the line P0 P1, then the extreme point along the direction away from the line through it
    const ObKey kr = argmax_pts([&](const ObPt &p) {
        const double wx = p.x - P0.x, wy = p.y - P0.y, wz = p.z - P0.z, t = (wx * ux + wy * uy + wz * uz) / uu;
        const double ex = wx - t * ux, ey = wy - t * uy, ez = wz - t * uz;
        return ObKey{ex * ex + ey * ey + ez * ez, ob_tie(p.x, p.y, p.z), 0.0, 0, 0};
    });
    int v[4] = {k0.pos, k1.pos, -1, -1};
    ObPt Pv[4];
    Pv[0] = P0; Pv[1] = P1;
    bool flat = !(sqrt(kr.a) > eps);
    if (!flat) {
        const ObPt R = ob_load(xyz, kr.pos, cx, cy, cz);
        const double wx = R.x - P0.x, wy = R.y - P0.y, wz = R.z - P0.z, t = (wx * ux + wy * uy + wz * uz) / uu;
        const double ex = wx - t * ux, ey = wy - t * uy, ez = wz - t * uz;
        const ObKey k2 = argmax_pts([&](const ObPt &p) { return ObKey{ex * p.x + ey * p.y + ez * p.z, ob_tie(p.x, p.y, p.z), 0.0, 0, 0}; });
        v[2] = k2.pos;
        Pv[2] = ob_load(xyz, k2.pos, cx, cy, cz);
        ObFacet base;
        flat = !ob_plane(Pv[0], Pv[1], Pv[2], base);
        if (!flat) {
            const ObKey k3r = argmax_pts([&](const ObPt &p) { return ObKey{fabs(ob_dist(base, p)), ob_tie(p.x, p.y, p.z), 0.0, 0, 0}; });
            const ObPt R3 = ob_load(xyz, k3r.pos, cx, cy, cz);
            const double s = ob_dist(base, R3);
            flat = !(fabs(s) > eps);
            if (!flat) {
                const double sg = s > 0 ? 1.0 : -1.0;
                const ObKey k3 = argmax_pts([&](const ObPt &p) {
                    return ObKey{sg * (base.nx * p.x + base.ny * p.y + base.nz * p.z), ob_tie(p.x, p.y, p.z), 0.0, 0, 0};
                });
                v[3] = k3.pos;
                Pv[3] = ob_load(xyz, k3.pos, cx, cy, cz);
                flat = !(fabs(ob_dist(base, Pv[3])) > eps);
            }
        }
    }
    if (flat) {                                      // Qhull: "initial simplex is flat" -> the caller's identity box (:1481-1484)
        if (lane == 0) ob_write_result(m, OB_ST_FLAT, 0.0, eyeR, yaw, status, rot);
        return;
    }

    // -- the tetrahedron, outward oriented
    ObFacet *fac = s_fac;
    int fcap = OB_FCAP, F = 0;
    bool overflow = false;
    if (lane < 4) {
        const int tri[4][4] = {{0, 1, 2, 3}, {0, 1, 3, 2}, {0, 2, 3, 1}, {1, 2, 3, 0}};
        int a = tri[lane][0], b = tri[lane][1], c = tri[lane][2];
        const int d = tri[lane][3];
        ObFacet f;
        ob_plane(Pv[a], Pv[b], Pv[c], f);
        if (ob_dist(f, Pv[d]) > 0) {
            const int t = b; b = c; c = t;
            ob_plane(Pv[a], Pv[b], Pv[c], f);
        }
        f.v0 = v[a]; f.v1 = v[b]; f.v2 = v[c]; f.aux = 0;
        s_fac[lane] = f;
    }
    F = 4;
    if (lane == 0) s_bad = 0;
    __syncthreads();

    // -- owners of the points outside the tetrahedron (first facet they lie above), the others dropped
    int2 *live = n <= OB_LCAP ? s_live : g_live;
    int live_n = 0;
    for (int base0 = 0; base0 < n; base0 += OB_THREADS) {
        const int i = base0 + lane;
        int own = -1;
        if (i < n) {
            const ObPt p = ob_load(xyz, i, cx, cy, cz);
            for (int j = 0; j < 4 && own < 0; ++j)
                if (ob_dist(s_fac[j], p) > eps) own = j;
        }
        const uint64_t bal = __ballot(own >= 0);
        if (own >= 0) live[live_n + cm3d_mbcnt(bal)] = make_int2(i, own);
        live_n += __popcll(bal);
    }
    __syncthreads();

    for (int iter = 0; live_n > 0 && !overflow; ++iter) {
        if (iter > n + 8) { overflow = true; break; }
        // the facet that owns the first live point; the point extreme along its normal
        const ObFacet fs = fac[live[0].y];
        ObKey best = {-INFINITY, -INFINITY, -INFINITY, 0x7FFFFFFF, 0};
        for (int t = lane; t < live_n; t += OB_THREADS) {
            const int i = live[t].x;
            const ObPt p = ob_load(xyz, i, cx, cy, cz);
            best = ob_key_max(best, ObKey{fs.nx * p.x + fs.ny * p.y + fs.nz * p.z, ob_tie(p.x, p.y, p.z), 0.0, i, 0});
        }
        best = ob_wave_key_max(best);
        const int q = best.pos;
        const ObPt Q = ob_load(xyz, q, cx, cy, cz);
        // visible facets
        int nv = 0;
        for (int base0 = 0; base0 < F; base0 += OB_THREADS) {
            const int j = base0 + lane;
            bool vis = false;
            if (j < F) {
                const ObFacet f = fac[j];
                vis = f.v0 >= 0 && ob_dist(f, Q) > eps;
            }
            const uint64_t bal = __ballot(vis);
            const int slot = nv + cm3d_mbcnt(bal);
            if (vis && slot < OB_VCAP) s_vis[slot] = j;
            nv += __popcll(bal);
        }
        if (nv > OB_VCAP || nv == 0) { overflow = true; break; }
        __syncthreads();
        // horizon: edges (a, b) of visible facets whose reverse (b, a) is no visible facet's edge
        int nh = 0;
        for (int base0 = 0; base0 < 3 * nv; base0 += OB_THREADS) {
            const int e = base0 + lane;
            bool hor = false;
            int a = 0, b = 0;
            if (e < 3 * nv) {
                const ObFacet f = fac[s_vis[e / 3]];
                const int r = e % 3;
                a = r == 0 ? f.v0 : (r == 1 ? f.v1 : f.v2);
                b = r == 0 ? f.v1 : (r == 1 ? f.v2 : f.v0);
                hor = true;
                for (int u = 0; u < nv && hor; ++u) {
                    const ObFacet g = fac[s_vis[u]];
                    hor = !((g.v0 == b && g.v1 == a) || (g.v1 == b && g.v2 == a) || (g.v2 == b && g.v0 == a));
                }
            }
            const uint64_t bal = __ballot(hor);
            const int slot = nh + cm3d_mbcnt(bal);
            if (hor && slot < OB_VCAP) s_hor[slot] = make_int2(a, b);
            nh += __popcll(bal);
        }
        if (nh > OB_VCAP || nh < 3) { overflow = true; break; }
        __syncthreads();
        for (int t = lane; t < nv; t += OB_THREADS) fac[s_vis[t]].v0 = -1;
        __syncthreads();
        // room for nh new facets: drop the removed ones first, then move from LDS to the list's workspace region
        if (F + nh > fcap) {
            int nf = 0;
            for (int base0 = 0; base0 < F; base0 += OB_THREADS) {
                const int j = base0 + lane;
                const bool alive = j < F && fac[j].v0 >= 0;
                const uint64_t bal = __ballot(alive);
                if (j < F) fac[j].aux = alive ? nf + cm3d_mbcnt(bal) : -1;
                nf += __popcll(bal);
            }
            __syncthreads();
            for (int t = lane; t < live_n; t += OB_THREADS) {
                const int2 e = live[t];
                live[t] = make_int2(e.x, fac[e.y].aux);
            }
            __syncthreads();
            for (int base0 = 0; base0 < F; base0 += OB_THREADS) {
                const int j = base0 + lane;
                ObFacet f;
                f.v0 = -1;
                if (j < F) f = fac[j];
                __syncthreads();
                if (j < F && f.v0 >= 0) fac[f.aux] = f;
                __syncthreads();
            }
            F = nf;
            if (F + nh > fcap) {
                if (fac != s_fac || (int64_t)F + nh > g_fcap || g_fac0 + g_fcap > n_facets) { overflow = true; break; }
                for (int j = lane; j < F; j += OB_THREADS) g_fac[j] = fac[j];
                __syncthreads();
                fac = g_fac;
                fcap = (int)g_fcap;
            }
        }
        // the cone from the new point over the horizon
        const int F0 = F;
        for (int t = lane; t < nh; t += OB_THREADS) {
            const int2 e = s_hor[t];
            ObFacet f;
            if (!ob_plane(ob_load(xyz, e.x, cx, cy, cz), ob_load(xyz, e.y, cx, cy, cz), Q, f)) s_bad = 1;
            f.v0 = e.x; f.v1 = e.y; f.v2 = q; f.aux = 0;
            fac[F0 + t] = f;
        }
        F = F0 + nh;
        __syncthreads();
        if (s_bad) { overflow = true; break; }          // a new facet without a plane (three collinear corners): no reliable hull
        // points of the removed facets: to the first new facet they lie above, or dropped (the new point itself included)
        int kept = 0;
        for (int base0 = 0; base0 < live_n; base0 += OB_THREADS) {
            const int t = base0 + lane;
            int2 e = make_int2(0, -1);
            if (t < live_n) {
                e = live[t];
                if (e.y < 0 || fac[e.y].v0 < 0) {
                    const ObPt p = ob_load(xyz, e.x, cx, cy, cz);
                    int own = -1;
                    if (e.x != q)
                        for (int j = F0; j < F && own < 0; ++j)
                            if (ob_dist(fac[j], p) > eps) own = j;
                    e.y = own;
                }
            }
            const uint64_t bal = __ballot(e.y >= 0);
            const int slot = kept + cm3d_mbcnt(bal);
            __syncthreads();                          // every lane has read its entry before any entry of this chunk is written
            if (e.y >= 0) live[slot] = e;
            kept += __popcll(bal);
        }
        live_n = kept;
        __syncthreads();
        if (live != s_live && live_n <= OB_LCAP) {   // small enough for LDS
            for (int t = lane; t < live_n; t += OB_THREADS) s_live[t] = live[t];
            __syncthreads();
            live = s_live;
        }
    }
    if (overflow) {
        if (lane == 0) ob_write_result(m, OB_ST_OVERFLOW, qnan, nanR, yaw, status, rot);
        return;
    }

    // -- vertex marks (list positions), then mean and covariance over the vertices in ascending position per lane
    int *mark = n <= 2 * OB_LCAP ? (int *)s_live : (int *)g_live;
    for (int i = lane; i < n; i += OB_THREADS) mark[i] = 0;
    __syncthreads();
    for (int j = lane; j < F; j += OB_THREADS) {
        const ObFacet f = fac[j];
        if (f.v0 >= 0) { mark[f.v0] = 1; mark[f.v1] = 1; mark[f.v2] = 1; }
    }
    __syncthreads();
    double sx = 0, sy = 0, sz = 0, cntl = 0;
    for (int i = lane; i < n; i += OB_THREADS)
        if (mark[i]) {
            const ObPt p = ob_load(xyz, i, cx, cy, cz);
            sx += p.x; sy += p.y; sz += p.z; cntl += 1.0;
            if (vmark) vmark[o + i] = 1;
        }
    s_part[lane][0] = sx; s_part[lane][1] = sy; s_part[lane][2] = sz; s_part[lane][3] = cntl;
    __syncthreads();
    double mean[3] = {0, 0, 0}, h = 0;
    for (int l = 0; l < OB_THREADS; ++l) { mean[0] += s_part[l][0]; mean[1] += s_part[l][1]; mean[2] += s_part[l][2]; h += s_part[l][3]; }
    mean[0] /= h; mean[1] /= h; mean[2] /= h;
    __syncthreads();
    double c6[6] = {0, 0, 0, 0, 0, 0};
    for (int i = lane; i < n; i += OB_THREADS)
        if (mark[i]) {
            const ObPt p = ob_load(xyz, i, cx, cy, cz);
            const double dx = p.x - mean[0], dy = p.y - mean[1], dz = p.z - mean[2];
            c6[0] += dx * dx; c6[1] += dy * dy; c6[2] += dz * dz; c6[3] += dx * dy; c6[4] += dx * dz; c6[5] += dy * dz;
        }
    double cov[6];
    for (int k = 0; k < 6; k += 3) {                 // two rounds through the 4-wide partial buffer
        __syncthreads();
        s_part[lane][0] = c6[k]; s_part[lane][1] = c6[k + 1]; s_part[lane][2] = c6[k + 2];
        __syncthreads();
        double a0 = 0, a1 = 0, a2 = 0;
        for (int l = 0; l < OB_THREADS; ++l) { a0 += s_part[l][0]; a1 += s_part[l][1]; a2 += s_part[l][2]; }
        cov[k] = a0 / h; cov[k + 1] = a1 / h; cov[k + 2] = a2 / h;
    }
    if (lane == 0) {
        double Rm[9];
        const double yv = ob_fit(cov, size, Rm);
        ob_write_result(m, OB_ST_FIT, yv, Rm, yaw, status, rot);
    }
}

__global__ void k_obb_selftest_yaw(const double *__restrict__ R, int n, double *__restrict__ yaw)
{
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    double r[9];
    for (int k = 0; k < 9; ++k) r[k] = R[(size_t)i * 9 + k];
    yaw[i] = ob_euler_zyx_yaw(r);
}

// facets of the workspace: every list's region (3 n + OB_FSLACK), the lists' points summing to at most idx_cap
static int64_t ob_facets(int32_t n_masks, int32_t idx_cap) { return 3 * (int64_t)idx_cap + (int64_t)OB_FSLACK * n_masks; }

extern "C" int64_t cm3d_obb_workspace_bytes(int32_t n_masks, int32_t idx_cap)
{
    if (n_masks <= 0 || idx_cap <= 0) return 0;
    return (int64_t)idx_cap * (int64_t)sizeof(int2) + ob_facets(n_masks, idx_cap) * (int64_t)sizeof(ObFacet);
}

extern "C" int cm3d_obb(const float *hit_xyz, const int32_t *hit_off, int32_t n_masks, int32_t idx_cap, double *yaw, int32_t *obb_status,
                        double *rot_opt, uint8_t *vertex_opt, void *workspace, int64_t workspace_bytes, cm3d_stream_t stream)
{
    if (!hit_xyz || !hit_off || !yaw || !obb_status || !workspace) return CM3D_ERR_ARG;
    if (n_masks <= 0 || idx_cap <= 0) return CM3D_ERR_ARG;
    if ((uintptr_t)hit_xyz & 15 || (uintptr_t)workspace & 7) return CM3D_ERR_ARG;
    if (workspace_bytes < cm3d_obb_workspace_bytes(n_masks, idx_cap)) return CM3D_ERR_WORKSPACE;
    hipStream_t st = (hipStream_t)stream;
    hipLaunchKernelGGL(k_obb, dim3(n_masks), dim3(OB_THREADS), 0, st, (const float4 *)hit_xyz, hit_off, n_masks, idx_cap, yaw, obb_status,
                       rot_opt, vertex_opt, (char *)workspace, ob_facets(n_masks, idx_cap));
    CM3D_CHECK_LAUNCH();
    return CM3D_OK;
}

extern "C" int cm3d_selftest_obb_yaw(const double *R, int32_t n, double *yaw, cm3d_stream_t stream)
{
    if (!R || !yaw || n <= 0) return CM3D_ERR_ARG;
    hipLaunchKernelGGL(k_obb_selftest_yaw, dim3((n + 255) / 256), dim3(256), 0, (hipStream_t)stream, R, n, yaw);
    CM3D_CHECK_LAUNCH();
    return CM3D_OK;
}
