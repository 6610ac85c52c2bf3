"""Host side of the rotated-box NMS (include/cm3d_hip.h: cm3d_rotated_nms, cm3d_box_rotated_nms; the last stage of cm3d_lift_pass_opt).

Every pseudo-label file passes through the reference's class-aware circle NMS (circle_nms, src/nuscenes/2d_to_3d.py:309-332): a box goes
when another box of its class has its centre within a per-class radius, wherever the two rectangles lie.  The reference also carries a
rotated-rectangle NMS it never calls (nms(rrects, scores, ...), src/kitti/2d_to_3d.py:359-599): sort by score, keep the best box, drop
every remaining box whose intersection with it, divided by the remaining box's own area, exceeds nms_threshold (strict >, :596;
default 0.4, :531-534) -- on polygons rasterised to an integer pixel grid, which is useless in metres.  What stands here in its place
is that greedy pass on the float64 rectangle clip the project already owns (csrc/bev_iou.h), with the reference's ratio ("cover") or
the IoU as the overlap.  This module is its statement to the bit (rotated_nms_host, records_from_boxes) and the switches of an engine
(RotatedNms).
"""
from dataclasses import dataclass
from typing import Mapping, Union

import numpy as np

from ._lib import MAX_MASKS_PER_FRAME

MEASURES = ("iou", "cover")                        # cm3d_rotated_nms's measure 0 / 1
DEFAULT_THR = 0.4                                  # the dead code's nms_threshold (src/kitti/2d_to_3d.py:531-534)


def measure_code(measure):
    if measure in MEASURES:
        return MEASURES.index(measure)
    if measure in (0, 1) and not isinstance(measure, bool):
        return int(measure)
    raise ValueError(f"measure: one of {MEASURES}")


@dataclass
class RotatedNms:
    """The opt-in NMS of a LiftEngine: behind the box launch of every pass the kept set is decided again, by the bird's-eye-view overlap
    of the boxes (class prior as the size, lane yaw as the heading) instead of their centre distance.  measure: "iou", or "cover" =
    the share of the lower-scored box that the kept one covers (the reference's ratio).  thr: a box goes when the measure exceeds it;
    one float, or a mapping from class name to float (classes it does not name: 0.4).  class_agnostic: boxes of different NMS groups
    suppress each other too."""
    measure: str = "iou"
    thr: Union[float, Mapping[str, float]] = DEFAULT_THR
    class_agnostic: bool = False

    def __post_init__(self):
        self.measure = MEASURES[measure_code(self.measure)]
        self.class_agnostic = bool(self.class_agnostic)
        if isinstance(self.thr, Mapping):
            self.thr = {str(k): float(v) for k, v in self.thr.items()}
            vals = list(self.thr.values())
        else:
            self.thr = float(self.thr)
            vals = [self.thr]
        if not all(v == v for v in vals):
            raise ValueError("thr: not NaN")

    @property
    def active(self):
        return True

    @property
    def measure_index(self):
        return MEASURES.index(self.measure)

    def thr_by_group(self, classes):
        """float64 threshold of every NMS group of a lifting.ClassTable (the kernel compares with thr[group of the lower box])."""
        out = np.full(len(classes.nms_thr), DEFAULT_THR if isinstance(self.thr, dict) else self.thr, np.float64)
        if isinstance(self.thr, dict):
            seen = {}
            for name, v in self.thr.items():
                g = int(classes.nms_group[classes.index(name)])
                if seen.setdefault(g, v) != v:
                    raise ValueError(f"thr: {name} shares its NMS group with a class of another threshold")
                out[g] = v
        return out


def add_arguments(ap):
    """The four flags of the nuScenes and Waymo entry points; --nms circle (the default) is the reference's NMS."""
    ap.add_argument("--nms", choices=("circle", "rotated"), default="circle",
                    help="circle: the reference's NMS on centre distances; rotated: greedy NMS on the bird's-eye-view overlap of the "
                         "boxes (class prior as the size, lane yaw as the heading)")
    ap.add_argument("--nms-overlap", choices=MEASURES, default="iou",
                    help="with --nms rotated: iou, or cover = the share of the lower-scored box that the kept box covers")
    ap.add_argument("--nms-thr", type=float, default=DEFAULT_THR, metavar="T",
                    help="with --nms rotated: a box goes when its overlap with a kept box exceeds T")
    ap.add_argument("--nms-class-agnostic", action="store_true", help="with --nms rotated: boxes of different classes suppress each other too")


def from_args(args):
    """RotatedNms from an entry point's flags; None for --nms circle."""
    return RotatedNms(args.nms_overlap, args.nms_thr, args.nms_class_agnostic) if args.nms == "rotated" else None


def records_from_boxes(box, prior_wlh, waymo):
    """(n, 6) float64 records cx, cy, length, width, c, s of box rows (n, BOX_STRIDE), as cm3d_box_rotated_nms builds them: centre and
    class from the row, size from the [w, l, h] table (length along the heading), and the heading's unit vector -- nuScenes: the axis of
    the rotation [qw, 0, 0, qz] = columns 3, 4, every product rounded on its own; Waymo: cos / sin of column 3."""
    box = np.atleast_2d(np.asarray(box, np.float64))
    prior = np.asarray(prior_wlh, np.float64).reshape(-1, 3)
    c8 = box[:, 8]
    with np.errstate(invalid="ignore"):
        cls = np.where((c8 >= 0.0) & (c8 < float(len(prior))), c8, 0.0).astype(np.int64)
    if waymo:
        c, s = np.cos(box[:, 3]), np.sin(box[:, 3])
    else:
        qw, qz = box[:, 3], box[:, 4]
        ww, zz = qw * qw, qz * qz
        c, s = ww - zz, (2.0 * qw) * qz
    return np.stack([box[:, 0], box[:, 1], prior[cls, 1], prior[cls, 0], c, s], 1)


def live(rec):
    """Boxes that take part in the overlap tests: positive float64 area, finite centre."""
    rec = np.asarray(rec, np.float64).reshape(-1, 6)
    with np.errstate(invalid="ignore", over="ignore"):
        return (rec[:, 2] * rec[:, 3] > 0.0) & np.isfinite(rec[:, 0]) & np.isfinite(rec[:, 1])


def measures(kept, later, measure):
    """measure(kept, later[j]) for record rows later (m, 6) against the kept record (6,) -- or row by row against kept (m, 6) --, all of
    them live: the device's values to the bit (waymo_eval._clip_area is bev_inter_area's host statement; the kept box is its first
    argument)."""
    from .waymo_eval import _clip_area
    later = np.asarray(later, np.float64).reshape(-1, 6)
    a = np.ascontiguousarray(np.broadcast_to(np.asarray(kept, np.float64).reshape(-1, 6), later.shape))
    inter = _clip_area(a, later)
    area_j = later[:, 2] * later[:, 3]
    with np.errstate(divide="ignore", invalid="ignore", over="ignore"):
        if measure_code(measure) == 0:
            uni = (a[:, 2] * a[:, 3] + area_j) - inter
            m = np.where(uni > 0.0, inter / uni, 0.0)
        else:
            m = inter / area_j
    return np.where(m > 1.0, 1.0, m)


def rotated_nms_host(rec, score, group, frame_off, thr, measure="iou", class_agnostic=False, take=None):
    """The statement cm3d_rotated_nms is held against: rec (n, 6), score (n,) finite, group (n,) int, frame_off (F + 1,), thr per group.
    Per frame: order = descending score, ties by descending index; the box of rank r, unless suppressed, is kept and suppresses every
    later-ranked, not yet suppressed box j with (class_agnostic or group[j] == group[i]) and measure(i, j) > thr[group[j]]; a box
    that is not `live` neither suppresses nor is suppressed; the boxes of a frame beyond its 1024th get keep 0.  take (n,) bool: the
    boxes that take part at all (cm3d_box_rotated_nms: flags & 1), the others get keep 0.  Returns keep (n,) int32.
    (The measures of all pairs the pass can come to compare are taken in one vectorised call per frame, the higher-ranked box first;
    pairs whose circumscribed circles are apart -- bev_inter_area's own first test: overlap 0 -- are left out of it.)"""
    rec = np.asarray(rec, np.float64).reshape(-1, 6)
    score, group = np.asarray(score, np.float64).reshape(-1), np.asarray(group, np.int64).reshape(-1)
    thr = np.asarray(thr, np.float64).reshape(-1)
    frame_off = np.asarray(frame_off, np.int64).reshape(-1)
    group = np.where((group >= 0) & (group < thr.size), group, 0)
    take = np.ones(len(rec), bool) if take is None else np.asarray(take, bool).reshape(-1)
    alive = live(rec)
    keep = np.zeros(len(rec), np.int32)
    for f in range(frame_off.size - 1):
        o, e = int(frame_off[f]), int(frame_off[f + 1])
        idx = np.arange(o, min(e, o + MAX_MASKS_PER_FRAME))
        idx = idx[take[idx]]
        order = idx[np.lexsort((-idx, -score[idx]))]
        keep[order[~alive[order]]] = 1                        # neither suppresses nor is suppressed
        order = order[alive[order]]
        m = order.size
        if m == 0:
            continue
        R, G = rec[order], group[order]
        T = thr[G]
        with np.errstate(invalid="ignore", over="ignore"):
            dx, dy = R[None, :, 0] - R[:, None, 0], R[None, :, 1] - R[:, None, 1]
            rad = np.sqrt(R[:, 2] * R[:, 2] + R[:, 3] * R[:, 3])
            r = 0.5 * (rad[:, None] + rad[None, :])
            apart = dx * dx + dy * dy > r * r
        pair = np.triu(np.ones((m, m), bool), 1) & ~(apart & (T[None, :] >= 0.0))        # (0 > thr only for a negative threshold)
        if not class_agnostic:
            pair &= G[:, None] == G[None, :]
        P, J = np.nonzero(pair)                               # row-major: the pairs of one kept box are consecutive
        hit = measures(R[P], R[J], measure) > T[J] if P.size else np.zeros(0, bool)
        start = np.searchsorted(P, np.arange(m + 1))
        sup = np.zeros(m, bool)
        for p in range(m):
            if not sup[p]:
                keep[order[p]] = 1
                s, t = start[p], start[p + 1]
                sup[J[s:t][hit[s:t]]] = True
    return keep
