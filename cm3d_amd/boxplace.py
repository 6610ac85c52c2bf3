"""Host side of the opt-in box placement (include/cm3d_hip.h: cm3d_box_place, cm3d_lift_pass_placed).

The box launch puts a vehicle's centre at the medoid of its in-mask points, pushed along the view ray by min(|w / 2 sin|, |l / 2 cos|)
(the reference's push_centroid, src/nuscenes/2d_to_3d.py:164-198): a guess at how far behind the seen surface the centre lies.  With the
yaw fit (bevfit.YawFit) the pass knows the bounding rectangle of the points at the fitted angle; its sensor-side corner is a corner of
the object and its sensor-side edges are faces.  Here the class's length and width are hung on them.  This module is the statement of
the rule, to the bit (box_place_host, circle NMS included), and the switches of the placed pass (BoxPlace).  The device result is held
against it, never the other way round.

What the placement does to label quality has not been measured, and the default of `thin` has not been tuned.
"""
from dataclasses import dataclass

import numpy as np

from ._lib import BOX_STRIDE, MAX_MASKS_PER_FRAME

NOT_PLACED, SRC_CORNER, SRC_ONE_AXIS, SRC_FACE_CENTRE = 0, 1, 2, 3      # place_src
MODES = ("push", "fit")                                                # --place


def _check(thin):
    if not (np.isfinite(thin) and thin >= 0.0):
        raise ValueError("thin: finite and >= 0")


@dataclass
class BoxPlace:
    """The opt-in placement of a LiftEngine (with yaw=YawFit(...) only): a vehicle box whose yaw was fitted is placed from the fitted
    rectangle.  Along an axis across which the rectangle is at least `thin` metres wide a second face was seen, and the box is anchored
    at the sensor-side corner; along the other it is centred on the seen face.  thin = 0 anchors both axes always.  Untuned."""
    thin: float = 0.5

    def __post_init__(self):
        _check(self.thin)
        self.thin = float(self.thin)

    @property
    def active(self):
        return True

    @staticmethod
    def from_args(mode="push", thin=None):
        """From an entry point's flags; None for --place push (the default: the path without the stage)."""
        if mode not in MODES:
            raise ValueError(f"place: one of {MODES}")
        if mode == "push":
            return None
        return BoxPlace(0.5 if thin is None else thin)


def add_arguments(ap):
    """The flags every nuScenes / Waymo lifting entry point carries; --place push (the default) is the path without the stage."""
    ap.add_argument("--place", choices=MODES, default="push",
                    help="push: a vehicle's centre is the medoid pushed along the view ray; fit (with --yaw fit): the box is hung on the "
                         "sensor-side corner and faces of the fitted rectangle.  Untuned, quality not measured")
    ap.add_argument("--place-thin", type=float, default=0.5, metavar="M",
                    help="with --place fit: a rectangle narrower than M metres across an axis shows one face, and the box is centred on it "
                         "along that axis (0: both axes are always anchored at the corner)")


def from_namespace(args, ap=None):
    """BoxPlace from an entry point's flags; None for --place push.  --place fit without --yaw fit is an error of the command line
    (ap.error when the parser is given, else ValueError)."""
    try:
        if args.place == "fit" and getattr(args, "yaw", "lane") != "fit":
            raise ValueError("--place fit needs --yaw fit")
        return BoxPlace.from_args(args.place, args.place_thin)
    except ValueError as e:
        if ap is None:
            raise
        ap.error(str(e))


def circle_nms_host(x, y, score, group, valid, nms_thr):
    """The greedy circle NMS of one frame as cm3d_box_nms states it (csrc/circle_nms.h): descending score, ties by descending index; a
    kept box suppresses every later box of its group within dist^2 <= nms_thr[group].  Only `valid` boxes take part.  Finite scores.
    Returns keep (n,) bool."""
    n = len(x)
    keep, sup = np.zeros(n, bool), np.zeros(n, bool)
    order = sorted(np.flatnonzero(valid).tolist(), key=lambda k: (-score[k], -k))
    for r, i in enumerate(order):
        if sup[i]:
            continue
        keep[i] = True
        for j in order[r + 1:]:
            if sup[j] or group[j] != group[i]:
                continue
            dx, dy = x[i] - x[j], y[i] - y[j]
            if (dx * dx) + (dy * dy) <= nms_thr[group[j]]:
                sup[j] = True
    return keep


def box_place_host(box, flags, mask_off, fit_rect, yaw_src, prior_wlh, nms_group, nms_thr, ego_xyz=None, thin=0.5,
                   max_masks_per_frame=MAX_MASKS_PER_FRAME):
    """What cm3d_box_place computes (include/cm3d_hip.h states the rule), to the bit.  ego_xyz (F, 3) on nuScenes, None on Waymo (the
    sensor is the origin of the vehicle frame).  Returns a dict: the new box and flags (copies), place_src (M,) int32, place_pushed (M, 2).
    numpy rounds every float64 product, sum and difference on its own: the expressions below are the rule's, bracket for bracket."""
    _check(thin)
    box = np.array(box, np.float64).reshape(-1, BOX_STRIDE)
    M = box.shape[0]
    flags = np.array(flags, np.int32).reshape(M)
    rect = np.asarray(fit_rect, np.float64).reshape(M, 6)
    yaw_src = np.asarray(yaw_src, np.int32).reshape(M)
    prior = np.asarray(prior_wlh, np.float64).reshape(-1, 3)
    nms_group, nms_thr = np.asarray(nms_group, np.int64).reshape(-1), np.asarray(nms_thr, np.float64).reshape(-1)
    off = np.clip(np.asarray(mask_off, np.int64).reshape(-1), 0, M)
    F = off.size - 1
    cap = min(int(max_masks_per_frame), MAX_MASKS_PER_FRAME)
    pushed = box[:, :2].copy()
    src = np.zeros(M, np.int32)
    with np.errstate(invalid="ignore"):
        b8 = box[:, 8]
        cls = np.where((b8 >= 0.0) & (b8 < float(prior.shape[0])), b8, 0.0).astype(np.int64)
    group = nms_group[cls]
    thin = np.float64(thin)
    for f in range(F):
        m0 = int(off[f])
        n_all = max(int(off[f + 1]), m0) - m0
        nm = min(n_all, cap)
        sl = slice(m0, m0 + nm)
        sx, sy = (np.float64(0.0), np.float64(0.0)) if ego_xyz is None else np.asarray(ego_xyz, np.float64).reshape(-1, 3)[f, :2]
        cx, cy, a, b, hc, hs = (rect[sl, q] for q in range(6))
        ln, wd = prior[cls[sl], 1], prior[cls[sl], 0]
        valid = (flags[sl] & 1) != 0
        take = valid & (yaw_src[sl] == 1) & np.isfinite(sx) & np.isfinite(sy) & np.isfinite(rect[sl]).all(1)
        with np.errstate(invalid="ignore", over="ignore"):
            ex, ey = sx - cx, sy - cy
            pu, pv = (ex * hc) + (ey * hs), (ey * hc) - (ex * hs)
            su, sv = np.where(pu >= 0.0, 1.0, -1.0), np.where(pv >= 0.0, 1.0, -1.0)
            au, av = b >= thin, a >= thin
            du = np.where(au, su * ((a - ln) * 0.5), 0.0)
            dv = np.where(av, sv * ((b - wd) * 0.5), 0.0)
            x = ((du * hc) - (dv * hs)) + cx
            y = ((du * hs) + (dv * hc)) + cy
        box[sl, 0] = np.where(take, x, box[sl, 0])
        box[sl, 1] = np.where(take, y, box[sl, 1])
        src[sl] = np.where(take, np.where(au & av, SRC_CORNER, np.where(au | av, SRC_ONE_AXIS, SRC_FACE_CENTRE)), NOT_PLACED)
        keep = circle_nms_host(box[sl, 0], box[sl, 1], box[sl, 7], group[sl], valid, nms_thr)
        flags[sl] = (flags[sl] & ~2) | (keep.astype(np.int32) << 1)
        flags[m0 + nm:m0 + n_all] &= ~2                    # beyond the launch's bound: not placed, not kept
        box[m0:m0 + n_all, 9] = flags[m0:m0 + n_all]
    return dict(box=box, flags=flags, place_src=src, place_pushed=pushed)
