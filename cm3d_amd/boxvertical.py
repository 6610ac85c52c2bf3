"""Host side of the opt-in vertical stage (include/cm3d_hip.h: cm3d_box_vertical; the call behind the pass).

Column 2 of a box is the medoid's z -- a point somewhere on the surface the LiDAR saw -- and its height is the class's prior.  Height
is the dimension a LiDAR sees most directly: one face shows its whole vertical extent.  Here two order statistics of every in-mask
list's z say where the seen surface begins and ends; where their distance is about the prior's height both ends were seen and the box
takes height and z from them, where it is much less the lower part was hidden and the prior's height is hung on the top seen, and
where it is much more the list holds ground or a wall and the box stays what it was.  Per frame, every class, no track and no yaw fit.
This module is the rule's statement to the bit (box_vertical_host), the switches of the stage (BoxVertical) and the flags of the entry
points.  The device result is held against it, never the other way round.

The five defaults (q_bot = 0.02, q_top = 0.98, min_points = 5, lo = 0.7, hi = 1.3) are untuned, and what the stage does to label
quality has not been measured: it cannot be on synthetic scenes.
"""
from dataclasses import dataclass

import numpy as np

from ._lib import BOX_STRIDE

SRC_NONE, SRC_BOTH_ENDS, SRC_TOP = 0, 1, 2                  # vert_src
ST_OK, ST_FEW, ST_EMPTY, ST_NOT_FINITE = 0, 1, 2, 4          # vert_status
MODES = ("medoid", "fit")                                   # --vertical
DEFAULT_Q_BOT, DEFAULT_Q_TOP, DEFAULT_MIN_POINTS, DEFAULT_LO, DEFAULT_HI = 0.02, 0.98, 5, 0.7, 1.3      # untuned
RESULTS = ("vert_z", "vert_h", "vert_src", "vert_status", "vert_entry_z")


def _check(q_bot, q_top, min_points, lo, hi):
    if not (0.0 <= q_bot <= q_top <= 1.0):
        raise ValueError("0 <= q_bot <= q_top <= 1")
    if int(min_points) < 1:
        raise ValueError("min_points >= 1")
    if not (0.0 < lo <= hi and np.isfinite(hi)):
        raise ValueError("0 < lo <= hi, both finite")


@dataclass
class BoxVertical:
    """The opt-in vertical stage of a LiftEngine (nuScenes and Waymo batches; needs no other option): height and z of a box from the
    order statistics q_bot and q_top (no interpolation) of its in-mask list's z.  min_points: a shorter list leaves the box alone;
    lo, hi: the seen extent over the prior's height inside [lo, hi] means both ends were seen, below lo only the top.  All untuned."""
    q_bot: float = DEFAULT_Q_BOT
    q_top: float = DEFAULT_Q_TOP
    min_points: int = DEFAULT_MIN_POINTS
    lo: float = DEFAULT_LO
    hi: float = DEFAULT_HI

    def __post_init__(self):
        self.q_bot, self.q_top, self.min_points = float(self.q_bot), float(self.q_top), int(self.min_points)
        self.lo, self.hi = float(self.lo), float(self.hi)
        _check(self.q_bot, self.q_top, self.min_points, self.lo, self.hi)

    @property
    def active(self):
        return True


def add_arguments(ap):
    """The flags of the nuScenes and Waymo entry points; --vertical medoid (the default) is the path without the stage."""
    ap.add_argument("--vertical", choices=MODES, default="medoid",
                    help="medoid: a box's z is the medoid's and its height the class's; fit: both from the vertical quantiles of the "
                         "in-mask points.  Untuned, quality not measured")
    ap.add_argument("--vertical-quantiles", default=None, metavar="QB,QT",
                    help=f"with --vertical fit: the two order statistics of a list's z (default {DEFAULT_Q_BOT},{DEFAULT_Q_TOP}; untuned)")
    ap.add_argument("--vertical-min-points", type=int, default=None, metavar="N",
                    help=f"with --vertical fit: a list of fewer than N points leaves its box alone (default {DEFAULT_MIN_POINTS}; untuned)")
    ap.add_argument("--vertical-ratio", default=None, metavar="LO,HI",
                    help=f"with --vertical fit: a seen extent inside [LO, HI] times the prior's height is the object's height, one below "
                         f"LO hangs the prior on the top seen (default {DEFAULT_LO},{DEFAULT_HI}; untuned)")


def _pair(text, flag, names):
    parts = text.split(",")
    if len(parts) != 2:
        raise ValueError(f"{flag}: {names} expected, got {text!r}")
    return float(parts[0]), float(parts[1])


def from_args(args, ap=None):
    """BoxVertical from an entry point's flags; None for --vertical medoid.  A --vertical-* flag without --vertical fit is an error of the
    command line (ap.error when the parser is given, else ValueError)."""
    try:
        given = [flag for flag, v in (("--vertical-quantiles", args.vertical_quantiles), ("--vertical-min-points", args.vertical_min_points),
                                      ("--vertical-ratio", args.vertical_ratio)) if v is not None]
        if args.vertical != "fit":
            if given:
                raise ValueError(f"{given[0]} needs --vertical fit")
            return None
        qb, qt = DEFAULT_Q_BOT, DEFAULT_Q_TOP
        if args.vertical_quantiles is not None:
            qb, qt = _pair(args.vertical_quantiles, "--vertical-quantiles", "QB,QT")
        lo, hi = DEFAULT_LO, DEFAULT_HI
        if args.vertical_ratio is not None:
            lo, hi = _pair(args.vertical_ratio, "--vertical-ratio", "LO,HI")
        return BoxVertical(qb, qt, DEFAULT_MIN_POINTS if args.vertical_min_points is None else args.vertical_min_points, lo, hi)
    except ValueError as e:
        if ap is None:
            raise
        ap.error(str(e))


def z_keys(z):
    """The unsigned keys whose order is the rule's order of the float32 values z: a total order on the bit patterns, -0.0 before +0.0."""
    bits = np.ascontiguousarray(z, np.float32).view(np.uint32)
    return bits ^ np.where(bits >> np.uint32(31), np.uint32(0xFFFFFFFF), np.uint32(0x80000000))


def box_vertical_host(xyz, off, idx_cap, box, flags, prior_wlh, q_bot=DEFAULT_Q_BOT, q_top=DEFAULT_Q_TOP, min_points=DEFAULT_MIN_POINTS,
                      lo=DEFAULT_LO, hi=DEFAULT_HI):
    """What cm3d_box_vertical computes (include/cm3d_hip.h states the rule), to the bit.  xyz: at least idx_cap rows of 4 float32 (rows
    from idx_cap on are never looked at), off (M + 1,), box (M, BOX_STRIDE), flags (M,), prior_wlh (C, 3).  Returns a dict: the new box
    (a copy), vert_z (M, 2), vert_h (M,), vert_src (M,) int32, vert_status (M,) int32, vert_entry_z (M,).  numpy rounds every float64
    operation on its own: the expressions below are the rule's, bracket for bracket."""
    _check(q_bot, q_top, min_points, lo, hi)
    idx_cap = int(idx_cap)
    box = np.array(box, np.float64).reshape(-1, BOX_STRIDE)
    M = box.shape[0]
    flags = np.asarray(flags, np.int32).reshape(M)
    prior = np.asarray(prior_wlh, np.float64).reshape(-1, 3)
    off = np.asarray(off, np.int64).reshape(-1)
    if idx_cap < 0 or off.size != M + 1 or (M > 0 and prior.shape[0] == 0):
        raise ValueError("idx_cap >= 0, one offset more than masks, n_classes > 0")
    zcol = np.ascontiguousarray(np.asarray(xyz, np.float32).reshape(-1, 4)[:idx_cap, 2]) if idx_cap else np.zeros(0, np.float32)
    if zcol.size < idx_cap:
        raise ValueError("xyz: fewer than idx_cap rows")
    q_bot, q_top = float(q_bot), float(q_top)
    status, vz = np.zeros(M, np.int32), np.zeros((M, 2), np.float64)
    for m in range(M):
        a = min(max(int(off[m]), 0), idx_cap)
        b = min(max(int(off[m + 1]), a), idx_cap)
        n = b - a
        if n == 0:
            status[m] = ST_EMPTY
        elif n < int(min_points):
            status[m] = ST_FEW
        else:
            z = zcol[a:b]
            if not np.isfinite(z).all():
                status[m] = ST_NOT_FINITE
                continue
            keys = z_keys(z)
            order = np.argsort(keys, kind="stable")             # (equal keys are equal bits: which of them is taken does not matter)
            kb, kt = int(q_bot * float(n - 1)), int(q_top * float(n - 1))
            vz[m] = float(z[order[kb]]), float(z[order[kt]])
    entry = box[:, 2].copy()
    with np.errstate(invalid="ignore"):
        b8 = box[:, 8]
        cls = np.where((b8 >= 0.0) & (b8 < float(max(prior.shape[0], 1))), b8, 0.0).astype(np.int64)
    h0 = prior[cls, 2] if M else np.zeros(0)
    lo, hi = np.float64(lo), np.float64(hi)
    zb, zt = vz[:, 0], vz[:, 1]
    with np.errstate(invalid="ignore", over="ignore", divide="ignore"):
        judged = ((flags & 1) != 0) & (status == 0) & np.isfinite(h0) & (h0 > 0.0)
        ext = zt - zb
        r = ext / np.where(judged, h0, 1.0)
        top = judged & (r < lo)
        both = judged & ~top & (r <= hi)
        z_both, z_top = zb + (ext * 0.5), zt - (h0 * 0.5)
    src = np.where(both, SRC_BOTH_ENDS, np.where(top, SRC_TOP, SRC_NONE)).astype(np.int32)
    box[:, 2] = np.where(both, z_both, np.where(top, z_top, box[:, 2]))
    return dict(box=box, vert_z=vz, vert_h=np.where(both, ext, h0), vert_src=src, vert_status=status, vert_entry_z=entry)
