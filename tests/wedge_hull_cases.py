"""numpy restatement of the view wedges on each camera's mask-column hull (csrc/project.hip: wedge_compose, wedge_setup,
k_frame_tables), shared by tests/test_wedge_hull_host.py and tests/test_gpu_wedge_hull.py.  Host only.

float64 composition, planes cast to float32, the plane test evaluated in float32 in the kernels' fma order."""
import numpy as np

from cm3d_amd import geometry as geo
from tests.camera_cases import CAM_K, culling_gates
from tests.magnitude_cases import _compose

f32 = np.float32


def hull_pad(record, W, min_dist):
    """The camera's pixel bound on the exact chain's column, or None where wedge_compose derives none (zmin <= 0.1, a composition
    that is no rotation to 1e-5, a record the derivation does not cover)."""
    g = culling_gates(record, W, 0, min_dist)
    if not (g["wedge"] and g["zmin"] > f32(0.1) and g["dev"] < 1e-5):
        return None
    K = np.asarray(record, f32)[CAM_K:CAM_K + 9]
    delta = f32(f32(f32(1e-6) * g["omax"]) + f32(1e-4))
    t = f32(max(K[2], f32(f32(W) - K[2])) / K[0])
    pd = f32(1.0) + np.ceil(f32(f32(f32(max(f32(2.0), f32(f32(1.0) + t)) * max(K[0], K[4])) * delta) / g["zmin"]))
    return int(min(pd, 32768))


def issue_pad_floor(record, W, min_dist):
    """1 + ceil(2 max(fx, fy) delta / zmin): the least a pad may be."""
    g = culling_gates(record, W, 0, min_dist)
    K = np.asarray(record, f32)[CAM_K:CAM_K + 9]
    delta = 1e-6 * float(g["omax"]) + 1e-4
    return 1 + int(np.ceil(2.0 * float(max(K[0], K[4])) * delta / float(g["zmin"])))


def camera_interval(record, W, min_dist, boxes):
    """[u_lo, u_hi] the planes of a camera stand on.  boxes: (x0, y0, x1, y1) of its masks' ERODED pixels (empty ones: x1 < x0 or
    y1 < y0, left out)."""
    pad = hull_pad(record, W, min_dist)
    live = [b for b in boxes if b[2] >= b[0] and b[3] >= b[1]]
    if pad is None or not live:
        return 0, W
    lo, hi = min(b[0] for b in live), max(b[2] for b in live)
    return max(lo - pad, 0), min(min(hi, W) + 1 + pad, W)


def wedge_planes(record, W, min_dist, u_lo, u_hi):
    """float32[8]: wedge_setup's planes on [u_lo, u_hi]; (0, 0, 0, 1) twice for a record outside the derivation."""
    rec = np.asarray(record, f32)
    out = np.array([0, 0, 0, 1, 0, 0, 0, 1], f32)
    g = culling_gates(rec, W, 0, min_dist)
    if not g["wedge"]:
        return out
    M, c = _compose(rec)
    fx, cx = float(rec[CAM_K]), float(rec[CAM_K + 2])
    margin = 1e-6 * float(g["omax"]) + 1e-3
    for e, (nx, nz) in enumerate(((fx, cx - u_lo), (-fx, u_hi - cx))):
        ln = np.sqrt(nx * nx + nz * nz)
        a, b = nx / ln, nz / ln
        out[4 * e:4 * e + 3] = (M[0] * a + M[2] * b).astype(f32)
        out[4 * e + 3] = f32(a * c[0] + b * c[2] + margin)
    return out


def _fma32(a, b, c):
    """float32 fma through float64: the product of two float32 is exact there."""
    return (np.asarray(a, np.float64) * np.asarray(b, np.float64) + np.asarray(c, np.float64)).astype(f32)


def wedge_min(planes, P):
    """min(l, r) per row of P (n, 3) float32 global points, in k_project_q's order: fma(n0, X, fma(n1, Y, fma(n2, Z, d)))."""
    P = np.asarray(P, f32)
    w = np.asarray(planes, f32)
    side = []
    for e in (0, 4):
        s = _fma32(w[e + 2], P[:, 2], np.full(P.shape[0], w[e + 3], f32))
        s = _fma32(w[e + 1], P[:, 1], s)
        side.append(_fma32(w[e], P[:, 0], s))
    return np.minimum(side[0], side[1])


def back_project(record, u, v, z):
    """float64 global points whose image under the composed camera is column u, row v at axial distance z (arrays)."""
    rec = np.asarray(record, f32)
    M, c = _compose(rec)
    K = geo.cam_K(rec).astype(np.float64)
    q = np.stack([np.asarray(u, np.float64), np.asarray(v, np.float64), np.ones(np.size(u))], 1) @ np.linalg.inv(K).T
    pc = q * (np.asarray(z, np.float64) / q[:, 2])[:, None]
    return (pc - c) @ np.linalg.inv(M).T


def to_sensor_rows(fr, pg, intensity=9.0):
    """Global float64 points as (n, 5) float32 rows of sweep 0's sensor frame (the inverse of sensor -> ego -> global)."""
    xf = np.asarray(fr.sweep_xf[0], np.float64)
    R_cs, t_cs, R_ego, t_ego = xf[0:9].reshape(3, 3), xf[9:12], xf[12:21].reshape(3, 3), xf[21:24]
    out = np.zeros((pg.shape[0], 5), f32)
    out[:, :3] = (((pg - t_ego) @ R_ego - t_cs) @ R_cs).astype(f32)
    out[:, 3] = intensity
    return out


def eroded_box(x0, y0, x1, y1):
    """Bounds of a filled rectangle's pixels after the 3x3 erosion (away from the image border)."""
    return x0 + 1, y0 + 1, x1 - 1, y1 - 1
