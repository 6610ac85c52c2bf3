"""Host side of the box velocity stage (include/cm3d_hip.h: cm3d_box_velocity; the call behind cm3d_lift_pass_opt).

Every nuScenes box the reference writes carries "velocity": [0, 0] (src/nuscenes/2d_to_3d.py:808-817).  nuScenes boxes are in the global
frame and a GPU batch is a set of whole scenes, so the kept boxes of consecutive keyframes can be associated on the device -- a
maximum-weight one-to-one assignment of gated centre distances by the solver the fusion matcher and the Waymo metrics share
(csrc/assign.h) -- and a box's velocity is the difference of matched centres over the difference of the frames' times.  This module is
the rule's statement to the bit (track_velocity_host, with link_table, pair_weights and assign_host as its parts), the switches of an
engine (Velocity) and the flags of the entry points.  Nothing here is tuned: the speed table is a guess at plausible top speeds, and
neither label quality nor mAVE on real data has been measured.
"""
from dataclasses import dataclass
from typing import Mapping, Optional, Union

import numpy as np

from ._lib import MAX_MASKS_PER_FRAME

ASSIGN_KMAX = 1000000                              # csrc/assign.h
DEFAULT_MAX_DT = 1.5                               # the devkit's box_velocity max_time_diff (eval_detection.box_velocity)
# m/s per class; untuned
DEFAULT_MAX_SPEED = {"car": 40.0, "truck": 40.0, "bus": 40.0, "trailer": 40.0, "construction_vehicle": 40.0, "motorcycle": 40.0,
                     "bicycle": 15.0, "pedestrian": 5.0, "barrier": 1.0, "traffic_cone": 1.0}
FALLBACK_MAX_SPEED = 40.0                          # a class the table does not name
VEL_NONE, VEL_FORWARD, VEL_BACKWARD, VEL_CENTRAL = 0, 1, 2, 3


@dataclass
class Velocity:
    """The opt-in velocity stage of a LiftEngine: behind every pass, the kept boxes of consecutive frames (HostBatch.frame_next,
    frame_time) are associated and `vel`, `vel_src`, `next_match`, `prev_match` filled.  max_speed: m/s, one float or a mapping from
    class name to float (classes it does not name: DEFAULT_MAX_SPEED, untuned); the gate of a pair is max_speed * dt.  Boxes are
    associated within the groups of the class table's nms_group, so classes that share a group must share a speed.  max_dt: seconds,
    the longest step between two frames that is a link, and the longest span a velocity is taken over."""
    max_speed: Union[None, float, Mapping[str, float]] = None
    max_dt: float = DEFAULT_MAX_DT

    def __post_init__(self):
        if self.max_speed is None:
            self.max_speed = {}
        if isinstance(self.max_speed, Mapping):
            self.max_speed = {str(k): float(v) for k, v in self.max_speed.items()}
            vals = list(self.max_speed.values())
        else:
            self.max_speed = float(self.max_speed)
            vals = [self.max_speed]
        self.max_dt = float(self.max_dt)
        if not all(v > 0.0 for v in vals):
            raise ValueError("max_speed: positive, not NaN")
        if not self.max_dt > 0.0:
            raise ValueError("max_dt: positive, not NaN")

    @property
    def active(self):
        return True

    def speed_by_group(self, classes):
        """float64 max_speed of every NMS group of a lifting.ClassTable (groups no class belongs to: FALLBACK_MAX_SPEED)."""
        out = np.full(len(classes.nms_thr), FALLBACK_MAX_SPEED, np.float64)
        seen = {}
        for ci, name in enumerate(classes.names):
            if isinstance(self.max_speed, dict):
                v = self.max_speed.get(name, DEFAULT_MAX_SPEED.get(name, FALLBACK_MAX_SPEED))
            else:
                v = self.max_speed
            g = int(classes.nms_group[ci])
            if seen.setdefault(g, v) != v:
                raise ValueError(f"max_speed: {name} shares its group with a class of another speed")
            out[g] = v
        return out


def add_arguments(ap):
    """The three flags of the nuScenes entry points; --velocity none (the default) writes the reference's [0, 0]."""
    ap.add_argument("--velocity", choices=("none", "track"), default="none",
                    help="none: \"velocity\": [0, 0] as the reference writes it; track: associate the kept boxes of consecutive keyframes "
                         "of a scene and write the difference of matched centres over the difference of the timestamps")
    ap.add_argument("--velocity-max-speed", default="", metavar="NAME=V[,NAME=V...]",
                    help="with --velocity track: m/s a box of class NAME may move between two keyframes (default table: untuned)")
    ap.add_argument("--velocity-max-dt", type=float, default=DEFAULT_MAX_DT, metavar="S",
                    help="with --velocity track: seconds; no association across a longer step, no velocity over a longer span")


def parse_max_speed(text):
    out = {}
    for item in filter(None, (s.strip() for s in (text or "").split(","))):
        name, sep, v = item.partition("=")
        if not sep:
            raise ValueError(f"--velocity-max-speed: NAME=V expected, got {item!r}")
        out[name.strip()] = float(v)
    return out


def from_args(args):
    """Velocity from an entry point's flags; None for --velocity none."""
    return Velocity(parse_max_speed(args.velocity_max_speed), args.velocity_max_dt) if args.velocity == "track" else None


def frame_times(timestamps_us):
    """frame_time of a batch: the int64 microsecond timestamps minus the batch's smallest (an exact integer difference -- absolute
    counts of about 1.5e15 are never subtracted in float64), then times 1e-6."""
    ts = np.asarray(timestamps_us, np.int64).reshape(-1)
    return ((ts - ts.min()) if ts.size else ts).astype(np.float64) * 1e-6


def frame_next_of(tokens, next_tokens):
    """frame_next of a batch from its frames' sample tokens and their `next` tokens: the batch index of the follower, -1 for '' or
    a follower outside the batch."""
    at = {t: i for i, t in enumerate(tokens)}
    return np.array([at.get(n, -1) if n else -1 for n in next_tokens], np.int32)


def frame_next_of_rows(rows, next_rows):
    """frame_next_of for frames named by their rows in sample.json (reader.Tables.sample_links): no Python statement per frame."""
    rows, nxt = np.asarray(rows, np.int64).reshape(-1), np.asarray(next_rows, np.int64).reshape(-1)
    if rows.size == 0:
        return np.zeros(0, np.int32)
    order = np.argsort(rows, kind="stable")
    pos = np.clip(np.searchsorted(rows[order], nxt), 0, rows.size - 1)
    return np.where((nxt >= 0) & (rows[order][pos] == nxt), order[pos], -1).astype(np.int32)


def _frame_masks(mask_off, f, n_masks):
    a, b = int(mask_off[f]), int(mask_off[f + 1])
    m0 = min(max(a, 0), n_masks)
    return m0, min(max(b, m0), n_masks) - m0


def link_table(mask_off, frame_next, frame_time, max_dt, n_masks=None):
    """The links of a batch: (link (F,) bool, dt (F,) float64, pair_off (F + 1,) int64 -- the prefix sums of M_f * M_n over the link
    slots, what cm3d_box_velocity takes --, status).  Slot f is a link iff n = frame_next[f] lies in [0, F) and
    0 < dt = frame_time[n] - frame_time[f] <= max_dt; a frame_next outside [-1, F) sets status bit 0, a frame of more than 1024 masks in a
    link status bit 1, and either slot holds no pair."""
    mask_off = np.asarray(mask_off, np.int64).reshape(-1)
    frame_next = np.asarray(frame_next, np.int64).reshape(-1)
    frame_time = np.asarray(frame_time, np.float64).reshape(-1)
    F = mask_off.size - 1
    n_masks = int(mask_off[-1]) if n_masks is None else int(n_masks)
    link, dt, sizes, status = np.zeros(F, bool), np.zeros(F, np.float64), np.zeros(F, np.int64), 0
    for f in range(F):
        n = int(frame_next[f])
        if n < -1 or n >= F:
            status |= 1
            continue
        if n < 0:
            continue
        d = frame_time[n] - frame_time[f]
        if not (d > 0.0 and d <= max_dt):
            continue
        Mf, Mn = _frame_masks(mask_off, f, n_masks)[1], _frame_masks(mask_off, n, n_masks)[1]
        if Mf > MAX_MASKS_PER_FRAME or Mn > MAX_MASKS_PER_FRAME:
            status |= 2
            continue
        link[f], dt[f], sizes[f] = True, d, Mf * Mn
    return link, dt, np.concatenate([[0], np.cumsum(sizes)]).astype(np.int64), status


def pair_weights(bf, kf, gf, bn, kn, gn, max_speed, dt):
    """int64 weights (len(bf), len(bn)) of a link: bf / bn box rows (centre in columns 0, 1), kf / kn kept, gf / gn group (-1: none),
    every operation rounded on its own as the header states."""
    bf, bn = np.asarray(bf, np.float64), np.asarray(bn, np.float64)
    max_speed = np.asarray(max_speed, np.float64).reshape(-1)
    gf, gn = np.asarray(gf, np.int64), np.asarray(gn, np.int64)
    ok = (np.asarray(kf, bool)[:, None] & np.asarray(kn, bool)[None, :] & (gf[:, None] == gn[None, :])
          & (gf[:, None] >= 0) & (gf[:, None] < max_speed.size))
    with np.errstate(invalid="ignore", over="ignore", divide="ignore"):
        dx, dy = bn[None, :, 0] - bf[:, None, 0], bn[None, :, 1] - bf[:, None, 1]
        d2 = (dx * dx) + (dy * dy)
        gate = (max_speed[np.clip(gf, 0, max_speed.size - 1)] * dt)[:, None]
        inside = ok & (gate > 0.0) & (d2 <= gate * gate)
        r = np.sqrt(d2) / gate
        inside &= r <= 1.0
        w = 1 + ((1.0 - np.where(inside, r, 1.0)) * float(ASSIGN_KMAX - 1)).astype(np.int64)
    return np.where(inside, w, 0)


def assign_host(W):
    """AssignSolver's steps (csrc/assign.h), one after the other: W (n, m) integer weights with n <= m; returns row_of (m,), the row
    assigned to every column or -1.  Every row gets a column; cost = ASSIGN_KMAX - weight; one row is added per phase; in a step the
    column of the least reduced cost joins the tree, ties going to an unassigned column first, then to the lowest column."""
    W = np.asarray(W, np.int64)
    n, m = W.shape
    assert n <= m
    INF = 1 << 30
    u, v = np.zeros(n + 1, np.int64), np.zeros(m + 1, np.int64)
    p, way = np.zeros(m + 1, np.int64), np.zeros(m + 1, np.int64)
    cols = np.arange(1, m + 1)
    C = ASSIGN_KMAX - W
    for i in range(1, n + 1):
        minv = np.full(m + 1, INF, np.int64)
        used = np.zeros(m + 1, bool)
        used[0] = True
        rows = []
        j0 = 0
        while True:
            used[j0] = True
            i0 = i if j0 == 0 else int(p[j0])
            rows.append(i0)
            free = ~used[1:]
            cur = C[i0 - 1] - u[i0] - v[1:]
            upd = free & (cur < minv[1:])
            minv[1:][upd] = cur[upd]
            way[1:][upd] = j0
            key = np.where(free, minv[1:] * 4096 + np.where(p[1:] != 0, 2048, 0) + cols, np.int64(INF) << 12)
            j1 = int(np.argmin(key)) + 1
            delta = int(key[j1 - 1] >> 12)
            u[rows] += delta
            v[1:][used[1:]] -= delta
            minv[1:][free] -= delta
            j0 = j1
            if p[j0] == 0:
                break
        while j0:
            j1 = int(way[j0])
            p[j0] = i if j1 == 0 else p[j1]
            j0 = j1
    return p[1:] - 1


def track_velocity_host(box, flags, mask_off, class_id, frame_next, frame_time, track_group, max_speed, max_dt=DEFAULT_MAX_DT,
                        want_weights=False):
    """What cm3d_box_velocity computes (include/cm3d_hip.h states the rule), to the bit.  Returns a dict: next_match, prev_match (M,)
    int32, vel (M, 2) float64, vel_src (M,) int32, status int, pair_off (F + 1,) int64; want_weights adds `weights`: slot -> (M_f, M_n)
    int64 matrix of every link."""
    box = np.asarray(box, np.float64)
    M = box.shape[0]
    flags = np.asarray(flags, np.int32).reshape(-1)
    mask_off = np.asarray(mask_off, np.int64).reshape(-1)
    class_id = np.asarray(class_id, np.int64).reshape(-1)
    frame_next = np.asarray(frame_next, np.int64).reshape(-1)
    frame_time = np.asarray(frame_time, np.float64).reshape(-1)
    track_group = np.asarray(track_group, np.int64).reshape(-1)
    max_speed = np.asarray(max_speed, np.float64).reshape(-1)
    F = mask_off.size - 1
    link, dt, pair_off, status = link_table(mask_off, frame_next, frame_time, max_dt, M)
    kept = (flags & 3) == 3
    cls_ok = (class_id >= 0) & (class_id < track_group.size)
    group = np.where(cls_ok, track_group[np.where(cls_ok, class_id, 0)], -1)
    next_match, prev_match = np.full(M, -1, np.int32), np.full(M, -1, np.int32)
    weights = {}
    for f in np.flatnonzero(link):
        n = int(frame_next[f])
        (f0, Mf), (n0, Mn) = _frame_masks(mask_off, f, M), _frame_masks(mask_off, n, M)
        if Mf == 0 or Mn == 0:
            continue
        rf, rn = slice(f0, f0 + Mf), slice(n0, n0 + Mn)
        W = pair_weights(box[rf], kept[rf], group[rf], box[rn], kept[rn], group[rn], max_speed, dt[f])
        if want_weights:
            weights[int(f)] = W
        tr = Mf > Mn                              # rows = the smaller side
        A = W.T if tr else W
        row_of = assign_host(A)
        for col, row in enumerate(row_of):
            if row >= 0 and A[row, col] > 0:
                pi, gi = (col, row) if tr else (row, col)
                next_match[f0 + pi] = n0 + gi
                prev_match[n0 + gi] = f0 + pi
    mask_frame = np.zeros(M, np.int64)
    for f in range(F):
        m0, k = _frame_masks(mask_off, f, M)
        mask_frame[m0:m0 + k] = f
    vel, vel_src = np.zeros((M, 2), np.float64), np.zeros(M, np.int32)
    for i in np.flatnonzero(kept):
        nm, pm = int(next_match[i]), int(prev_match[i])
        t = frame_time[mask_frame[i]]
        tp = frame_time[mask_frame[nm]] if nm >= 0 else t
        tm = frame_time[mask_frame[pm]] if pm >= 0 else t
        with np.errstate(invalid="ignore", over="ignore", divide="ignore"):
            if nm >= 0 and pm >= 0 and tp - tm <= max_dt:
                vel[i], vel_src[i] = (box[nm, :2] - box[pm, :2]) / (tp - tm), VEL_CENTRAL
            elif nm >= 0 and tp - t <= max_dt:
                vel[i], vel_src[i] = (box[nm, :2] - box[i, :2]) / (tp - t), VEL_FORWARD
            elif pm >= 0 and t - tm <= max_dt:
                vel[i], vel_src[i] = (box[i, :2] - box[pm, :2]) / (t - tm), VEL_BACKWARD
    out = dict(next_match=next_match, prev_match=prev_match, vel=vel, vel_src=vel_src, status=status, pair_off=pair_off)
    if want_weights:
        out["weights"] = weights
    return out
