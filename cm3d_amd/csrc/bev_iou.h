// Rotated-rectangle intersection in float64, shared by fusion.hip (bird's-eye-view IoU of the SAM3D matching) and
// waymo_metrics.hip (3D IoU of the Waymo evaluator).
#pragma once
#include "common.h"

// Box record: cx, cy, length, width, cos(heading), sin(heading) (float64).
// Intersection by clipping A against the four edges of B (both counter-clockwise), in coordinates
// relative to A's centre so that global-frame magnitudes cancel before the products.
//
// Clip buffer capacity.  Exact clipping of a rectangle by four half-planes leaves at most 8 vertices, but the signs here
// are rounded: nearly identical boxes reach 9 and 10 (tests/iou_cases.py HIGH_VERTEX).  One clip of an n-gon emits one
// vertex per point inside and one per sign change; with m points inside there are at most 2 min(m, n - m) changes, so
// at most floor(1.5 n) vertices whatever the signs: 4 -> 6 -> 9 -> 13 -> 19.  The first three clips are stored (13
// slots); the fourth clip's vertices go straight into the shoelace sum, in the order and with the products the stored
// polygon would give, so its 19 need no buffer.  (20 stored slots would push the arrays out of registers into scratch.)
#define BEV_CLIP_CAP 13
static __device__ void bev_corners(const double *__restrict__ b, double ox, double oy, double *X, double *Y)
{
    const double hl = b[2] * 0.5, hw = b[3] * 0.5, c = b[4], s = b[5];
    const double dx = b[0] - ox, dy = b[1] - oy;
    const double lc = hl * c, ls = hl * s, wc = hw * c, wsn = hw * s;
    X[0] = (dx + lc) - wsn; Y[0] = (dy + ls) + wc;
    X[1] = (dx - lc) - wsn; Y[1] = (dy - ls) + wc;
    X[2] = (dx - lc) + wsn; Y[2] = (dy - ls) - wc;
    X[3] = (dx + lc) + wsn; Y[3] = (dy + ls) - wc;
}

// Area of the intersection of A and B (0 when their circumscribed circles are apart).
static __device__ double bev_inter_area(const double *__restrict__ a, const double *__restrict__ b)
{
    {   // circumscribed circles apart: the intersection is empty
        const double dx = b[0] - a[0], dy = b[1] - a[1];
        const double ra2 = a[2] * a[2] + a[3] * a[3], rb2 = b[2] * b[2] + b[3] * b[3];
        const double r = 0.5 * (sqrt(ra2) + sqrt(rb2));
        if (dx * dx + dy * dy > r * r) return 0.0;
    }
    double px[BEV_CLIP_CAP], py[BEV_CLIP_CAP], qx[BEV_CLIP_CAP], qy[BEV_CLIP_CAP], bx[4], by[4];
    bev_corners(a, a[0], a[1], px, py);
    bev_corners(b, a[0], a[1], bx, by);
    int n = 4;
    double acc = 0.0, fx = 0.0, fy = 0.0, lx = 0.0, ly = 0.0;      // shoelace sum over the last clip's vertices
    for (int e = 0; e < 4 && n > 0; ++e) {
        const double x1 = bx[e], y1 = by[e], ex = bx[(e + 1) & 3] - x1, ey = by[(e + 1) & 3] - y1;
        int k = 0;
        auto emit = [&](double x, double y) {
            if (e < 3) { qx[k] = x; qy[k] = y; }
            else if (k == 0) { fx = x; fy = y; }
            else acc += lx * y - x * ly;                             // term (k - 1, k) of the stored polygon's sum
            lx = x; ly = y;
            ++k;
        };
        double prx = px[n - 1], pry = py[n - 1];
        double dp = ex * (pry - y1) - ey * (prx - x1);
        for (int i = 0; i < n; ++i) {
            const double cx = px[i], cy = py[i];
            const double dc = ex * (cy - y1) - ey * (cx - x1);
            if ((dc >= 0.0) != (dp >= 0.0)) {
                const double t = dp / (dp - dc);
                emit(prx + t * (cx - prx), pry + t * (cy - pry));
            }
            if (dc >= 0.0) emit(cx, cy);
            prx = cx; pry = cy; dp = dc;
        }
        n = k;
        if (e < 3)
            for (int i = 0; i < n; ++i) { px[i] = qx[i]; py[i] = qy[i]; }
    }
    if (n < 3) return 0.0;                                           // n >= 3: the fourth clip ran
    acc += lx * fy - fx * ly;                                        // term (n - 1, 0)
    return 0.5 * fabs(acc);
}

static __device__ __attribute__((unused)) double bev_iou(const double *__restrict__ a, const double *__restrict__ b)
{
    const double area_a = a[2] * a[3], area_b = b[2] * b[3];
    if (!(area_a > 0.0) || !(area_b > 0.0)) return 0.0;       // zeros(D) = "no box" (linear_matching.py:65)
    const double inter = bev_inter_area(a, b);
    const double uni = (area_a + area_b) - inter;
    if (!(uni > 0.0)) return 0.0;
    const double iou = inter / uni;
    return iou > 1.0 ? 1.0 : iou;
}
