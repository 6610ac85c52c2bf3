"""Host side of the opt-in ground stage (include/cm3d_hip.h: cm3d_box_ground; the call behind the pass and the vertical stage's).

The bottom face of a box is a guess: column 2 is the medoid's z, a point somewhere on the surface the LiDAR saw, and even the vertical
stage sees tops, not bottoms.  Objects stand on the ground, and the ground around an object is what the sweep measures best.  Here every
mask looks at the points of its frame's own sweep inside a circle around its centre and a window around its height -- the first stage
that looks at a point outside a mask -- bins their z, and takes a low quantile of the bins as the ground under the box.  The box then
spans ground to the top the vertical stage saw, or is the class's prior height stood on the ground, or stays what it was.
This module is the rule's statement to the bit (box_ground_host), the switches of the stage (BoxGround) and the flags of the entry
points.  The device result is held against it, never the other way round.

The seven defaults (radius = 3.0 m, quantile = 0.1, min_points = 20, down, up = 5.0, 0.5 m, lo, hi = 0.7, 1.3) are untuned, and what the
stage does to label quality has not been measured: it cannot be on synthetic scenes.
"""
from dataclasses import dataclass

import numpy as np

from ._lib import BOX_STRIDE, GROUND_BINS

SRC_NONE, SRC_GROUND_TOP, SRC_PRIOR = 0, 1, 2               # ground_src
ST_OK, ST_FEW, ST_EMPTY, ST_NOT_FINITE = 0, 1, 2, 4          # ground_status
MODES = ("medoid", "fit")                                   # --ground
DEFAULT_RADIUS, DEFAULT_QUANTILE, DEFAULT_MIN_POINTS = 3.0, 0.1, 20                  # untuned
DEFAULT_DOWN, DEFAULT_UP, DEFAULT_LO, DEFAULT_HI = 5.0, 0.5, 0.7, 1.3                 # untuned
RESULTS = ("ground_z", "ground_n", "ground_h", "ground_src", "ground_status", "ground_zref")


def _check(radius, quantile, min_points, down, up, lo, hi):
    if not (np.isfinite(radius) and radius > 0.0):
        raise ValueError("radius finite and > 0")
    if not (0.0 <= quantile <= 1.0):
        raise ValueError("0 <= quantile <= 1")
    if int(min_points) < 1:
        raise ValueError("min_points >= 1")
    if not (np.isfinite(down) and np.isfinite(up) and down > 0.0 and up >= 0.0):
        raise ValueError("down finite and > 0, up finite and >= 0")
    if not (0.0 < lo <= hi and np.isfinite(hi)):
        raise ValueError("0 < lo <= hi, both finite")


@dataclass
class BoxGround:
    """The opt-in ground stage of a LiftEngine (nuScenes and Waymo batches; needs no other option): z of a box from the ground of its
    frame's own sweep.  radius: the circle around the centre; down, up: the window below and above the box's reference height, cut into
    128 bins; quantile: of the members' bins, the ground; min_points: fewer members leave the box alone; lo, hi: the top the vertical
    stage saw over the ground, against the prior's height, inside [lo, hi] means the box spans ground to top.  All untuned."""
    radius: float = DEFAULT_RADIUS
    quantile: float = DEFAULT_QUANTILE
    min_points: int = DEFAULT_MIN_POINTS
    down: float = DEFAULT_DOWN
    up: float = DEFAULT_UP
    lo: float = DEFAULT_LO
    hi: float = DEFAULT_HI

    def __post_init__(self):
        self.radius, self.quantile, self.min_points = float(self.radius), float(self.quantile), int(self.min_points)
        self.down, self.up, self.lo, self.hi = float(self.down), float(self.up), float(self.lo), float(self.hi)
        _check(self.radius, self.quantile, self.min_points, self.down, self.up, self.lo, self.hi)

    @property
    def active(self):
        return True

    def params(self):
        return dict(radius=self.radius, quantile=self.quantile, min_points=self.min_points, down=self.down, up=self.up, lo=self.lo,
                    hi=self.hi)


def add_arguments(ap):
    """The flags of the nuScenes and Waymo entry points; --ground medoid (the default) is the path without the stage."""
    ap.add_argument("--ground", choices=MODES, default="medoid",
                    help="medoid: a box's z is the medoid's (or the vertical stage's); fit: the box stands on the ground of the frame's own "
                         "sweep around it.  Untuned, quality not measured")
    ap.add_argument("--ground-radius", type=float, default=None, metavar="R",
                    help=f"with --ground fit: the radius in metres of the circle around a box's centre (default {DEFAULT_RADIUS}; untuned)")
    ap.add_argument("--ground-quantile", type=float, default=None, metavar="Q",
                    help=f"with --ground fit: the quantile of the members' height bins that is the ground (default {DEFAULT_QUANTILE}; untuned)")
    ap.add_argument("--ground-min-points", type=int, default=None, metavar="N",
                    help=f"with --ground fit: fewer than N points around a box leave it alone (default {DEFAULT_MIN_POINTS}; untuned)")
    ap.add_argument("--ground-window", default=None, metavar="DOWN,UP",
                    help=f"with --ground fit: the window in metres below and above the box's height in which ground is looked for (default "
                         f"{DEFAULT_DOWN},{DEFAULT_UP}; untuned)")
    ap.add_argument("--ground-ratio", default=None, metavar="LO,HI",
                    help=f"with --ground fit and --vertical fit: a top inside [LO, HI] prior heights over the ground makes the box span both "
                         f"(default {DEFAULT_LO},{DEFAULT_HI}; untuned)")


def _pair(text, flag, names):
    parts = text.split(",")
    if len(parts) != 2:
        raise ValueError(f"{flag}: {names} expected, got {text!r}")
    return float(parts[0]), float(parts[1])


def from_args(args, ap=None):
    """BoxGround from an entry point's flags; None for --ground medoid.  A --ground-* flag without --ground fit is an error of the
    command line (ap.error when the parser is given, else ValueError)."""
    try:
        given = [flag for flag, v in (("--ground-radius", args.ground_radius), ("--ground-quantile", args.ground_quantile),
                                      ("--ground-min-points", args.ground_min_points), ("--ground-window", args.ground_window),
                                      ("--ground-ratio", args.ground_ratio)) if v is not None]
        if args.ground != "fit":
            if given:
                raise ValueError(f"{given[0]} needs --ground fit")
            return None
        down, up = DEFAULT_DOWN, DEFAULT_UP
        if args.ground_window is not None:
            down, up = _pair(args.ground_window, "--ground-window", "DOWN,UP")
        lo, hi = DEFAULT_LO, DEFAULT_HI
        if args.ground_ratio is not None:
            lo, hi = _pair(args.ground_ratio, "--ground-ratio", "LO,HI")
        return BoxGround(DEFAULT_RADIUS if args.ground_radius is None else args.ground_radius,
                         DEFAULT_QUANTILE if args.ground_quantile is None else args.ground_quantile,
                         DEFAULT_MIN_POINTS if args.ground_min_points is None else args.ground_min_points, down, up, lo, hi)
    except ValueError as e:
        if ap is None:
            raise
        ap.error(str(e))


def box_ground_host(points, pt_off, mask_off, box, flags, prior_wlh, zref=None, vert=None, radius=DEFAULT_RADIUS, quantile=DEFAULT_QUANTILE,
                    min_points=DEFAULT_MIN_POINTS, down=DEFAULT_DOWN, up=DEFAULT_UP, lo=DEFAULT_LO, hi=DEFAULT_HI):
    """What cm3d_box_ground computes (include/cm3d_hip.h states the rule), to the bit.  points: (N, >= 3) float32, the frames' clouds
    back to back -- the very float32 the sweep preparation gives; a row with a non-finite coordinate is no point (so the rows the
    preparation drops may be left out or left in as NaN) --, pt_off (F + 1,) their first rows, mask_off (F + 1,), box (M, BOX_STRIDE),
    flags (M,), prior_wlh (C, 3).  zref (M,): the reference heights, None: column 2 of box.  vert: None, or the vertical stage's outputs
    (a mapping with vert_status, vert_z, vert_h).  Returns a dict: the new box (a copy) and the six RESULTS.  numpy rounds every float64
    operation on its own: the expressions below are the rule's, bracket for bracket."""
    _check(radius, quantile, min_points, down, up, lo, hi)
    box = np.array(box, np.float64).reshape(-1, BOX_STRIDE)
    M = box.shape[0]
    flags = np.asarray(flags, np.int32).reshape(M)
    prior = np.asarray(prior_wlh, np.float64).reshape(-1, 3)
    pt_off, mask_off = np.asarray(pt_off, np.int64).reshape(-1), np.asarray(mask_off, np.int64).reshape(-1)
    pts = np.asarray(points, np.float32)
    pts = pts.reshape(-1, pts.shape[-1] if pts.ndim > 1 else 4)
    if pt_off.size != mask_off.size or pt_off.size < 1 or (M > 0 and prior.shape[0] == 0):
        raise ValueError("one pt_off and one mask_off entry per frame and one more, n_classes > 0")
    zr = box[:, 2].copy() if zref is None else np.array(zref, np.float64).reshape(M)
    R, Q, DOWN, UP = np.float64(radius), float(quantile), np.float64(down), np.float64(up)
    rr = R * R
    dz = (DOWN + UP) / np.float64(GROUND_BINS)
    cx, cy = box[:, 0], box[:, 1]
    with np.errstate(invalid="ignore"):
        z0 = zr - DOWN
    finite = np.isfinite(cx) & np.isfinite(cy) & np.isfinite(zr)
    status = np.where(finite, ST_EMPTY, ST_NOT_FINITE).astype(np.int32)
    n_mem, gz = np.zeros(M, np.int32), np.zeros(M, np.float64)
    for f in range(pt_off.size - 1):
        m0 = min(max(int(mask_off[f]), 0), M)
        m1 = min(max(int(mask_off[f + 1]), m0), M)
        p0 = min(max(int(pt_off[f]), 0), len(pts))
        p1 = min(max(int(pt_off[f + 1]), p0), len(pts))
        p = pts[p0:p1, :3]
        p = p[np.isfinite(p).all(1)].astype(np.float64)
        for m in range(m0, m1):
            if not finite[m]:
                continue
            dx, dy = p[:, 0] - cx[m], p[:, 1] - cy[m]
            t = (p[:, 2] - z0[m]) / dz
            member = ((dx * dx) + (dy * dy) <= rr) & (t >= 0.0) & (t < float(GROUND_BINS))
            n = int(member.sum())
            n_mem[m] = n
            if n == 0:
                continue
            if n < int(min_points):
                status[m] = ST_FEW
                continue
            status[m] = ST_OK
            cum = np.cumsum(np.bincount(t[member].astype(np.int64), minlength=GROUND_BINS))
            k = int(Q * float(n - 1))
            b = int(np.searchsorted(cum, k, side="right"))             # the smallest bin whose cumulative count exceeds k
            gz[m] = z0[m] + ((np.float64(b) + 0.5) * dz)
    with np.errstate(invalid="ignore"):
        b8 = box[:, 8]
        cls = np.where((b8 >= 0.0) & (b8 < float(max(prior.shape[0], 1))), b8, 0.0).astype(np.int64)
    h0 = prior[cls, 2] if M else np.zeros(0)
    lo, hi = np.float64(lo), np.float64(hi)
    with np.errstate(invalid="ignore", over="ignore", divide="ignore"):
        judged = ((flags & 1) != 0) & (status == ST_OK) & np.isfinite(h0) & (h0 > 0.0)
        hs = np.where(judged, h0, 1.0)
        if vert is not None:
            top = np.asarray(vert["vert_z"], np.float64).reshape(M, 2)[:, 1]
            ext = top - gz
            r = ext / hs
            s1 = judged & (np.asarray(vert["vert_status"]).reshape(M) == 0) & (lo <= r) & (r <= hi)
            h_was = np.array(vert["vert_h"], np.float64).reshape(M)
        else:
            ext, s1, h_was = np.zeros(M), np.zeros(M, bool), h0
        s2 = judged & ~s1 & (zr - gz <= h0 + UP)
        z1, z2 = gz + (ext * 0.5), gz + (h0 * 0.5)
    src = np.where(s1, SRC_GROUND_TOP, np.where(s2, SRC_PRIOR, SRC_NONE)).astype(np.int32)
    box[:, 2] = np.where(s1, z1, np.where(s2, z2, box[:, 2]))
    return dict(box=box, ground_z=gz, ground_n=n_mem, ground_h=np.where(s1, ext, np.where(s2, h0, h_was)), ground_src=src,
                ground_status=status, ground_zref=zr)
