"""Case tables of the yaw fit (cm3d_bev_fit, cm3d_yaw_select; host statements in cm3d_amd/bevfit.py).  Numpy only; nothing here touches
the device.  tests/test_bev_fit_host.py asserts that the tables hold what they are for.

standalone()      name -> (xyz (n, 4) float32, meta): lists at global magnitude (600 / 1200 m; one group near 10 km) of every length at
                  which the kernel takes another turn -- 0, 1, 2, min_points -+ 1, the wave, two waves, the LDS chunk -+ 1, about 1000,
                  about 5000 --, lists of every status, a NaN row, duplicated rows, collinear points, a square blob, and two-face
                  "cars" at 41 yaws over (-pi, pi], noise-free and with 3 cm of noise.
select_table(w)   the inputs of cm3d_yaw_select for nuScenes (w False) and for Waymo poses (w True): fitted axes on either side of
                  the perpendicular of the lane direction, every fit status, vehicle and other classes, masks without a medoid,
                  lane distances below, on and above the thresholds in LANE_MIN_DISTS.
"""
import numpy as np

from cm3d_amd._lib import BEV_FIT_CHUNK

MIN_POINTS, MIN_LENGTH, D0 = 20, 1.0, 0.05             # the defaults of bevfit.YawFit
ANGLES = (64, 128, 256)
CAR_L, CAR_W = 4.5, 1.9
CAR_YAWS = np.linspace(-np.pi, np.pi, 42)[1:]          # 41 yaws over (-pi, pi]
LENGTHS = (0, 1, 2, MIN_POINTS - 1, MIN_POINTS, 63, 64, 65, 127, 128, 129, BEV_FIT_CHUNK - 1, BEV_FIT_CHUNK, BEV_FIT_CHUNK + 1, 1000, 5003)
LANE_MIN_DISTS = (0.0, 2.0, 3.0)
IS_VEHICLE = np.array([1, 1, 1, 1, 1, 0, 0, 0, 0, 1], np.int32)     # lifting.ClassTable.nuscenes().is_vehicle


def _rows(xy):
    out = np.zeros((len(xy), 4), np.float32)
    if len(xy):
        out[:, :2] = np.asarray(xy, np.float64)
        out[:, 2] = 1.5                            # z is not used
    return out


def car(yaw, n_long=90, n_short=60, centre=(600.0, 1200.0), noise=0.0, rng=None, shuffle=True):
    """Two perpendicular faces of a CAR_L x CAR_W rectangle of heading `yaw` that meet in a corner: evenly spaced points, the long face
    first, then (shuffle) mixed by a fixed permutation -- a compaction lists points in row order, not face by face."""
    u = np.concatenate([np.linspace(-CAR_L / 2, CAR_L / 2, n_long), np.full(n_short, CAR_L / 2)])
    v = np.concatenate([np.full(n_long, -CAR_W / 2), np.linspace(-CAR_W / 2, CAR_W / 2, n_short)])
    x = centre[0] + u * np.cos(yaw) - v * np.sin(yaw)
    y = centre[1] + u * np.sin(yaw) + v * np.cos(yaw)
    if noise:
        x, y = x + noise * rng.standard_normal(x.size), y + noise * rng.standard_normal(y.size)
    xy = np.stack([x, y], 1)
    if shuffle:
        xy = xy[np.random.default_rng(x.size).permutation(x.size)]
    return _rows(xy)


def _blob(n, rng, centre=(612.25, 1187.5), scale=(2.2, 0.9), yaw=0.4):
    """n points scattered over a rotated rectangle (a status-0 list of any length, no exact structure)."""
    u, v = rng.uniform(-scale[0], scale[0], n), rng.uniform(-scale[1], scale[1], n)
    return _rows(np.stack([centre[0] + u * np.cos(yaw) - v * np.sin(yaw), centre[1] + u * np.sin(yaw) + v * np.cos(yaw)], 1))


_STANDALONE = None


def standalone():
    global _STANDALONE
    if _STANDALONE is not None:
        return _STANDALONE
    rng = np.random.default_rng(20)
    out = {}
    for n in LENGTHS:
        out[f"len_{n}"] = (_blob(n, rng), dict(kind="length", n=n))
    nan_row = _blob(40, rng)
    nan_row[17, 1] = np.nan
    out["nan_row"] = (nan_row, dict(kind="nan"))
    inf_first = _blob(40, rng)
    inf_first[0, 0] = np.inf
    out["inf_first_row"] = (inf_first, dict(kind="nan"))
    out["short"] = (_blob(30, rng, scale=(0.2, 0.1)), dict(kind="short"))
    dup = _blob(25, rng)
    out["duplicates"] = (np.concatenate([dup, dup[::2], dup[:5], dup[:1]], 0), dict(kind="duplicates"))
    out["all_the_same_point"] = (np.repeat(_blob(1, rng), 33, 0), dict(kind="short"))
    out["collinear"] = (_rows(np.stack([600.0 + 0.125 * np.arange(40), np.full(40, 1200.0)], 1)), dict(kind="collinear"))
    g = 0.5 * np.arange(5)
    out["square"] = (_rows(np.stack([600.0 + np.repeat(g, 5), 1200.0 + np.tile(g, 5)], 1)), dict(kind="square"))
    for i, yaw in enumerate(CAR_YAWS):
        out[f"car_{i:02d}"] = (car(yaw), dict(kind="car", yaw=float(yaw), lmax=CAR_L))
        out[f"car_noisy_{i:02d}"] = (car(yaw, noise=0.03, rng=rng), dict(kind="car_noisy", yaw=float(yaw), lmax=CAR_L))
    for i, yaw in enumerate(CAR_YAWS[::5]):        # near 10 km: the float32 grid is 1 mm there
        out[f"car_far_{i:02d}"] = (car(yaw, centre=(-9950.0, 10100.0)), dict(kind="car_far", yaw=float(yaw), lmax=CAR_L))
    out["len_far_200"] = (_blob(200, rng, centre=(9970.5, -10020.25)), dict(kind="length", n=200))
    for v in out.values():
        v[0].setflags(write=False)
    _STANDALONE = out
    return out


def pack(lists):
    """(xyz (total, 4), off (M + 1,)) of lists back to back."""
    off = np.concatenate([[0], np.cumsum([len(p) for p in lists])]).astype(np.int32)
    xyz = np.concatenate(lists, 0) if lists else np.zeros((0, 4), np.float32)
    return np.ascontiguousarray(xyz, np.float32), off


def axis_error(rect, yaw):
    """Angle between the record's axis and `yaw`, modulo pi / 2 (the rule cannot tell the faces apart), in [0, pi / 4]."""
    a = np.arctan2(rect[5], rect[4]) - yaw
    return abs((a + np.pi / 4) % (np.pi / 2) - np.pi / 4)


def known_answer_bound(K, lmax=CAR_L, d0=D0):
    """delta + asin(d0 / Lmax): the grid step, and the angle below which every point's deviation from its face saturates at d0 -- inside
    it the criterion cannot tell two grid angles apart.  Derived, not measured."""
    return np.pi / (2 * K) + np.arcsin(d0 / lmax)


# ------------------------------------------------------------------------------------------------ cm3d_yaw_select
def _pose_rt(yaw, t):
    from cm3d_amd import geometry as geo
    R = geo.rot_z(yaw) @ geo.quat_to_rotmat([1.0, 0.004, -0.003, 0.0])
    return np.concatenate([R.reshape(9), np.asarray(t, np.float64)]).astype(np.float32)


_SELECT = {}


def select_table(waymo):
    """dict: fit_rect (M, 6), fit_status, medoid_pos, class_id, lane_dist, mask_frame, lane (L, 3) float32, lane_off, frame_lane,
    lane_idx, lane_yaw (M,) float32 (the gather yaw_select_host takes), pose_rt (F, 12) float32 or None, is_vehicle."""
    if waymo in _SELECT:
        return _SELECT[waymo]
    rng = np.random.default_rng(7 + int(waymo))
    pose_yaws = (0.3, np.pi / 2 + 0.013, np.pi - 0.011)          # one pose rotated by about 90 degrees, one by about 180
    F = len(pose_yaws)
    pose_rt = np.stack([_pose_rt(y, (5000.0 + 40 * i, -3000.0, 20.0)) for i, y in enumerate(pose_yaws)]) if waymo else None
    # two lane tables; frames 0 and 2 use table 1, frame 1 table 0
    lane_yaws = [np.float32(v) for v in (0.0, 0.7, 1.5707964, -2.4, 3.1415927, -0.05, 2.2, -1.3)]
    lane = np.zeros((16, 3), np.float32)
    lane[:, :2] = rng.uniform(-50, 50, (16, 2))
    lane[:, 2] = lane_yaws + lane_yaws[::-1]
    lane_off, frame_lane = np.array([0, 7, 16], np.int32), np.array([1, 0, 1], np.int32)
    rows = []
    side = (-0.2, 0.2, 0.02, -0.02)                # the lane direction this far from the axis' perpendicular, either side
    k = 0
    for f in range(F):
        t0, tn = int(lane_off[frame_lane[f]]), int(lane_off[frame_lane[f] + 1] - lane_off[frame_lane[f]])
        for li in range(tn):
            yl = float(lane[t0 + li, 2])
            for quarter in (1, -1):
                for ds in side:
                    # the axis in the lane's frame: quarter * pi / 2 + ds off the lane direction, then back into the list's frame
                    a = yl + quarter * np.pi / 2 + ds - (pose_yaws[f] if waymo else 0.0)
                    rows.append(dict(f=f, li=li, a=a, status=0, cls=(0, 1, 2, 9, 4)[k % 5], mp=k % 7, ld=(0.0, 1.0, 2.0, 3.0, 7.5)[k % 5]))
                    k += 1
            # along the lane and against it, and what must not take the fit
            rows.append(dict(f=f, li=li, a=yl + 0.1, status=0, cls=0, mp=3, ld=2.0))
            rows.append(dict(f=f, li=li, a=yl + np.pi - 0.1, status=0, cls=3, mp=0, ld=2.5))
            rows.append(dict(f=f, li=li, a=yl + 1.4, status=0, cls=(5, 6, 7, 8)[li % 4], mp=1, ld=4.0))       # not a vehicle
            rows.append(dict(f=f, li=li, a=yl + 1.4, status=1 + li % 4, cls=0, mp=2, ld=4.0))                 # not fitted
            rows.append(dict(f=f, li=li, a=yl + 1.4, status=0, cls=0, mp=-1, ld=np.inf))                      # no medoid
    rows.append(dict(f=0, li=0, a=0.5, status=0, cls=-3, mp=0, ld=9.0))                # a class outside the table reads as class 0
    rows.append(dict(f=1, li=2, a=0.5, status=0, cls=77, mp=0, ld=9.0))
    M = len(rows)
    rect = np.zeros((M, 6))
    for m, r in enumerate(rows):
        if r["status"] == 0:
            rect[m] = [10.0 * m, -3.0 * m, 4.0, 1.7, np.cos(r["a"]), np.sin(r["a"])]
    g = lambda key, dt: np.array([r[key] for r in rows], dt)
    mask_frame, lane_idx = g("f", np.int32), g("li", np.int32)
    lane_idx[g("mp", np.int32) < 0] = -1           # what cm3d_lane_nn leaves for a mask without a medoid
    lane_yaw = lane[np.maximum(lane_off[frame_lane[mask_frame]] + lane_idx, 0), 2]
    out = dict(fit_rect=rect, fit_status=g("status", np.int32), medoid_pos=g("mp", np.int32), class_id=g("cls", np.int32),
               lane_dist=g("ld", np.float64), mask_frame=mask_frame, lane=lane, lane_off=lane_off, frame_lane=frame_lane, lane_idx=lane_idx,
               lane_yaw=lane_yaw, pose_rt=pose_rt, is_vehicle=IS_VEHICLE)
    for v in out.values():
        if isinstance(v, np.ndarray):
            v.setflags(write=False)
    _SELECT[waymo] = out
    return out


def select_host(t, lane_min_dist):
    from cm3d_amd import bevfit
    return bevfit.yaw_select_host(t["fit_rect"], t["fit_status"], t["medoid_pos"], t["class_id"], t["is_vehicle"], t["lane_dist"], t["lane_yaw"],
                                  lane_min_dist, t["pose_rt"], t["mask_frame"])
