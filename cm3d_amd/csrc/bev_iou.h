// Rotated-rectangle intersection in float64, shared by fusion.hip (bird's-eye-view IoU of the SAM3D matching) and
// waymo_metrics.hip (3D IoU of the Waymo evaluator).
#pragma once
#include "common.h"

// Box record: cx, cy, length, width, cos(heading), sin(heading) (float64).
// Intersection by clipping A against the four edges of B (both counter-clockwise), in coordinates
// relative to A's centre so that global-frame magnitudes cancel before the products.
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
    double px[12], py[12], qx[12], qy[12], bx[4], by[4];
    bev_corners(a, a[0], a[1], px, py);
    bev_corners(b, a[0], a[1], bx, by);
    int n = 4;
    for (int e = 0; e < 4 && n > 0; ++e) {
        const double x1 = bx[e], y1 = by[e], ex = bx[(e + 1) & 3] - x1, ey = by[(e + 1) & 3] - y1;
        int k = 0;
        double prx = px[n - 1], pry = py[n - 1];
        double dp = ex * (pry - y1) - ey * (prx - x1);
        for (int i = 0; i < n; ++i) {
            const double cx = px[i], cy = py[i];
            const double dc = ex * (cy - y1) - ey * (cx - x1);
            if ((dc >= 0.0) != (dp >= 0.0)) {
                const double t = dp / (dp - dc);
                qx[k] = prx + t * (cx - prx);
                qy[k] = pry + t * (cy - pry);
                ++k;
            }
            if (dc >= 0.0) { qx[k] = cx; qy[k] = cy; ++k; }
            prx = cx; pry = cy; dp = dc;
        }
        n = k;
        for (int i = 0; i < n; ++i) { px[i] = qx[i]; py[i] = qy[i]; }
    }
    if (n < 3) return 0.0;
    double acc = 0.0;
    for (int i = 0; i < n; ++i) {
        const int j = (i + 1 == n) ? 0 : i + 1;
        acc += px[i] * py[j] - px[j] * py[i];
    }
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
