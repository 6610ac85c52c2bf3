"""Host side of the opt-in yaw fit (include/cm3d_hip.h: cm3d_bev_fit, cm3d_yaw_select, cm3d_yaw_fit_boxes; a stage of
cm3d_lift_pass_opt).

On nuScenes and Waymo a box's heading is the yaw of the nearest lane point (2d_to_3d.py:295): the in-mask points are never looked at.
What stands here is a heading fitted to them: search-based L-shape fitting with the closeness criterion (Zhang, Xu, Dolan, Gong: "Efficient
L-shape fitting for vehicle detection using laser scanners", IV 2017) on the bird's-eye view of one mask's list.  This module is the
statement of the rule, to the bit (bev_fit_host, yaw_select_host), and the switches of the fitted pass (YawFit).  The device result is
held against it, never the other way round.  The area criterion is deliberately not offered: for two perpendicular faces the bounding
rectangle's area is the same at the true angle and at the diagonal's.

What the fit does to label quality has not been measured, and none of the defaults below has been tuned.
"""
from dataclasses import dataclass

import numpy as np

FITTED, FEW_POINTS, EMPTY, SHORT, NON_FINITE = 0, 1, 2, 3, 4      # fit_status
SRC_LANE, SRC_FIT = 0, 1                                           # yaw_src
MODES = ("lane", "fit")                                            # --yaw


def _check(angles, min_points, min_length, d0, lane_min_dist=0.0):
    if int(angles) != angles or int(angles) % 64 or not 64 <= int(angles) <= 256:
        raise ValueError("angles: a multiple of 64 in 64..256")
    if int(min_points) != min_points or int(min_points) < 2:
        raise ValueError("min_points: an integer >= 2")
    if not (np.isfinite(min_length) and min_length >= 0.0):
        raise ValueError("min_length: finite and >= 0")
    if not (np.isfinite(d0) and d0 > 0.0):
        raise ValueError("d0: finite and > 0")
    if not lane_min_dist >= 0.0:                   # (NaN fails the comparison; +inf: the fit is never used)
        raise ValueError("lane_min_dist >= 0")


@dataclass
class YawFit:
    """The opt-in yaw fit of a LiftEngine: the heading axis of every vehicle mask is fitted to its in-mask points on a grid of `angles`
    directions over a quarter turn (closeness criterion, deviations floored at `d0` metres), the nearest lane point only says which way
    along the axis; lists of fewer than `min_points` points or a fitted length below `min_length` metres keep the lane's yaw, and so do
    masks nearer than `lane_min_dist` metres to a lane (0: the fit is always used).  None of the defaults has been tuned."""
    angles: int = 128
    min_points: int = 20
    min_length: float = 1.0
    d0: float = 0.05
    lane_min_dist: float = 0.0

    def __post_init__(self):
        _check(self.angles, self.min_points, self.min_length, self.d0, self.lane_min_dist)
        self.angles, self.min_points = int(self.angles), int(self.min_points)
        self.min_length, self.d0, self.lane_min_dist = float(self.min_length), float(self.d0), float(self.lane_min_dist)

    @property
    def active(self):
        return True

    @staticmethod
    def from_args(mode="lane", angles=None, min_points=None, min_length=None, d0=None, lane_min_dist=None):
        """From an entry point's flags; None for --yaw lane (the default: the path without the fit)."""
        if mode not in MODES:
            raise ValueError(f"yaw: one of {MODES}")
        if mode == "lane":
            return None
        return YawFit(128 if angles is None else angles, 20 if min_points is None else min_points, 1.0 if min_length is None else min_length,
                      0.05 if d0 is None else d0, 0.0 if lane_min_dist is None else lane_min_dist)


def add_arguments(ap):
    """The flags every nuScenes / Waymo lifting entry point carries; --yaw lane (the default) is the path without the fit."""
    ap.add_argument("--yaw", choices=MODES, default="lane",
                    help="lane: a box's heading is the nearest lane point's yaw; fit: the heading axis of a vehicle is fitted to its in-mask "
                         "points (L-shape fit, closeness criterion) and the lane only says which way along it.  Untuned, quality not measured")
    ap.add_argument("--yaw-fit-angles", type=int, default=128, metavar="K", help="directions over a quarter turn: 64, 128, 192 or 256")
    ap.add_argument("--yaw-fit-min-points", type=int, default=20, metavar="N", help="shorter lists keep the lane's yaw")
    ap.add_argument("--yaw-fit-min-length", type=float, default=1.0, metavar="M", help="a fitted length below M metres keeps the lane's yaw")
    ap.add_argument("--yaw-fit-d0", type=float, default=0.05, metavar="M", help="floor of a point's deviation from the rectangle, metres")
    ap.add_argument("--yaw-fit-lane-min-dist", type=float, default=0.0, metavar="M",
                    help="masks nearer than M metres to a lane keep the lane's yaw (0: the fit is always used)")


def from_namespace(args):
    return YawFit.from_args(args.yaw, args.yaw_fit_angles, args.yaw_fit_min_points, args.yaw_fit_min_length, args.yaw_fit_d0,
                            args.yaw_fit_lane_min_dist)


def angle_table(K=128):
    """angle_cs of cm3d_bev_fit: float64 (K, 2) = cos, sin of k * pi / (2 K).  Computed here and handed to the device, so that both
    sides use the same bits."""
    K = int(K)
    if K % 64 or not 64 <= K <= 256:
        raise ValueError("angles: a multiple of 64 in 64..256")
    th = np.arange(K, dtype=np.float64) * np.pi / (2.0 * K)
    return np.ascontiguousarray(np.stack([np.cos(th), np.sin(th)], 1))


def bev_fit_host(xyz, angles=128, d0=0.05, min_points=20, min_length=1.0, table=None):
    """The statement cm3d_bev_fit is held against, for one list: xyz (n, >=2) float32 in list order (z is not used).
    Returns (k, rect (6,) float64 = cx, cy, length, width, cos, sin, status).  Every product and sum is rounded on its own, and the sum
    over the points runs in list order (np.cumsum adds sequentially; np.sum does not)."""
    _check(angles, min_points, min_length, d0)
    cs = angle_table(angles) if table is None else np.asarray(table, np.float64).reshape(int(angles), 2)
    p = np.asarray(xyz, np.float32)
    p = p.reshape(-1, p.shape[-1] if p.ndim > 1 else 3)[:, :2]
    n = p.shape[0]
    none = lambda st: (-1, np.zeros(6), st)
    if n == 0:
        return none(EMPTY)
    if n < int(min_points):
        return none(FEW_POINTS)
    if not np.isfinite(p).all():                   # up front: min / max never see a NaN
        return none(NON_FINITE)
    x0, y0 = np.float64(p[0, 0]), np.float64(p[0, 1])
    x, y = (p[:, 0].astype(np.float64) - x0)[:, None], (p[:, 1].astype(np.float64) - y0)[:, None]
    c, s = cs[None, :, 0], cs[None, :, 1]
    c1 = (x * c) + (y * s)
    c2 = (y * c) - (x * s)
    lo1, hi1, lo2, hi2 = c1.min(0), c1.max(0), c2.min(0), c2.max(0)
    d = np.maximum(np.minimum(np.minimum(hi1 - c1, c1 - lo1), np.minimum(hi2 - c2, c2 - lo2)), np.float64(d0))
    q = np.cumsum(1.0 / d, axis=0)[-1]             # q_k = (((0 + 1/d_0) + 1/d_1) + ...)
    k = int(np.argmax(q))                          # the first of the greatest
    a, b = hi1[k] - lo1[k], hi2[k] - lo2[k]
    ck, sk = cs[k, 0], cs[k, 1]
    length, width = (a, b) if a >= b else (b, a)
    if length < np.float64(min_length):
        return none(SHORT)
    m1, m2 = (lo1[k] + hi1[k]) * 0.5, (lo2[k] + hi2[k]) * 0.5
    cx = ((m1 * ck) - (m2 * sk)) + x0
    cy = ((m1 * sk) + (m2 * ck)) + y0
    hc, hs = (ck, sk) if a >= b else (-sk, ck)
    return k, np.array([cx, cy, length, width, hc, hs], np.float64), FITTED


def bev_fit_lists(hit_off, hit_xyz, angles=128, d0=0.05, min_points=20, min_length=1.0):
    """bev_fit_host over the lists of a batch: (fit_k (M,), fit_rect (M, 6), fit_status (M,))."""
    hit_off = np.asarray(hit_off, np.int64)
    M = hit_off.size - 1
    tab = angle_table(angles)
    fk, fr, fs = np.full(M, -1, np.int32), np.zeros((M, 6)), np.zeros(M, np.int32)
    for m in range(M):
        fk[m], fr[m], fs[m] = bev_fit_host(np.asarray(hit_xyz)[int(hit_off[m]):int(hit_off[m + 1])], angles, d0, min_points, min_length, tab)
    return fk, fr, fs


def select_dot(rect, lane_yaw, pose_rt=None):
    """(cg, sg, dot) of yaw_select_host for one mask: the fitted axis in the lane's frame and its product with the lane direction."""
    c, s = np.float64(rect[4]), np.float64(rect[5])
    if pose_rt is not None:
        R = np.asarray(pose_rt, np.float32).reshape(-1)[:9].astype(np.float64)
        c, s = R[0] * c + R[1] * s, R[3] * c + R[4] * s
    yl = np.float64(np.float32(lane_yaw))
    return c, s, c * np.cos(yl) + s * np.sin(yl)


def yaw_select_host(fit_rect, fit_status, medoid_pos, class_id, is_vehicle, lane_dist, lane_yaw, lane_min_dist=0.0, pose_rt=None,
                    mask_frame=None):
    """The statement cm3d_yaw_select is held against.  lane_yaw (M,) float32: the yaw of each mask's nearest lane point (anything for a
    mask without a medoid: it gets 0); pose_rt (F, 12) float32 with mask_frame (M,) on Waymo, where the lists are in the vehicle frame.
    Returns (yaw (M,) float32, yaw_src (M,) int32)."""
    M = len(medoid_pos)
    is_vehicle = np.asarray(is_vehicle)
    yaw, src = np.zeros(M, np.float32), np.zeros(M, np.int32)
    for m in range(M):
        if medoid_pos[m] < 0:
            continue
        cls = int(class_id[m])
        cls = cls if 0 <= cls < is_vehicle.size else 0
        yaw[m] = np.float32(lane_yaw[m])
        if fit_status[m] != FITTED or not is_vehicle[cls] or not lane_dist[m] >= lane_min_dist:
            continue
        cg, sg, dot = select_dot(fit_rect[m], lane_yaw[m], None if pose_rt is None else np.asarray(pose_rt)[int(mask_frame[m])])
        if dot < 0:
            cg, sg = -cg, -sg
        yaw[m], src[m] = np.float32(np.arctan2(sg, cg)), SRC_FIT
    return yaw, src
