"""Host side of the opt-in ground strip (include/cm3d_hip.h: cm3d_ground_grid, cm3d_ground_strip; the stage in front of the depth
clustering in cm3d_lift_pass_stripped).

A mask drawn around a vehicle or a pedestrian almost always covers a strip of road at its foot.  The erosion does not remove it and
the depth clustering cannot: the road beside the wheels lies at the object's own range.  So the medoid is pulled down and towards the
sensor, the L-shape fit sees a fan of road points, and the vertical and size stages reject what is often just road in the list.  Here
every frame's own sweep gives a grid of ground heights around the frame's origin (ground_grid_host: a low quantile of the heights in
every cell), and every in-mask list loses the points below its cell's ground plus a margin (ground_strip_host) before anything else
reads it.  The reference has nothing of the kind.  This module is the rule's statement to the bit, the switches of the stage
(GroundStrip) and the flags of the entry points.  The device result is held against it, never the other way round.

The seven defaults (cell = 2.0 m, down, up = 4.0, 4.0 m, quantile = 0.1, min_points = 8, margin = 0.3 m, min_keep = 5) are untuned, and
what the stage does to label quality has not been measured: it cannot be on synthetic scenes.
"""
from dataclasses import dataclass

import numpy as np

from ._lib import GROUND_GRID_BINS, GROUND_GRID_CELLS, MEDOID_TILE

ST_STRIPPED, ST_KEPT_WHOLE, ST_EMPTY = 0, 1, 2               # gs_status
MODES = ("off", "grid")                                      # --ground-strip
DEFAULT_CELL, DEFAULT_DOWN, DEFAULT_UP, DEFAULT_QUANTILE = 2.0, 4.0, 4.0, 0.1          # untuned
DEFAULT_MIN_POINTS, DEFAULT_MARGIN, DEFAULT_MIN_KEEP = 8, 0.3, 5                        # untuned
HALF = GROUND_GRID_CELLS // 2
N_CELLS = GROUND_GRID_CELLS * GROUND_GRID_CELLS


def _check(cell, down, up, quantile, min_points, margin, min_keep):
    if not (np.isfinite(cell) and cell > 0.0):
        raise ValueError("cell finite and > 0")
    if not (np.isfinite(down) and np.isfinite(up) and down > 0.0 and up > 0.0):
        raise ValueError("down and up finite and > 0")
    if not (0.0 <= quantile <= 1.0):
        raise ValueError("0 <= quantile <= 1")
    if int(min_points) != min_points or int(min_points) < 1:
        raise ValueError("min_points: an integer >= 1")
    if not np.isfinite(margin):
        raise ValueError("margin finite")
    if int(min_keep) != min_keep or int(min_keep) < 1:
        raise ValueError("min_keep: an integer >= 1")


@dataclass
class GroundStrip:
    """The opt-in ground strip of a LiftEngine (nuScenes and Waymo batches; needs no other option): ground points leave every in-mask
    list before the clustering, the medoid and every fit see it.  cell: the side of a grid cell; down, up: the window below and above
    the frame's origin, cut into 64 bins; quantile: of a cell's members' bins, its ground; min_points: a cell of fewer members has no
    estimate; margin: a list point below its cell's ground plus this is ground; min_keep: a list that would keep fewer points is kept
    whole.  All untuned."""
    cell: float = DEFAULT_CELL
    down: float = DEFAULT_DOWN
    up: float = DEFAULT_UP
    quantile: float = DEFAULT_QUANTILE
    min_points: int = DEFAULT_MIN_POINTS
    margin: float = DEFAULT_MARGIN
    min_keep: int = DEFAULT_MIN_KEEP

    def __post_init__(self):
        self.cell, self.down, self.up = float(self.cell), float(self.down), float(self.up)
        self.quantile, self.margin = float(self.quantile), float(self.margin)
        _check(self.cell, self.down, self.up, self.quantile, self.min_points, self.margin, self.min_keep)
        self.min_points, self.min_keep = int(self.min_points), int(self.min_keep)

    @property
    def active(self):
        return True

    def params(self):
        return dict(cell=self.cell, down=self.down, up=self.up, quantile=self.quantile, min_points=self.min_points, margin=self.margin,
                    min_keep=self.min_keep)


def add_arguments(ap):
    """The flags of the nuScenes and Waymo entry points; --ground-strip off (the default) is the path without the stage."""
    ap.add_argument("--ground-strip", choices=MODES, default="off",
                    help="off: the in-mask lists are what the masks left; grid: points below the ground of the frame's own sweep (a grid "
                         "of heights around the sensor rig) leave every list before anything reads it.  Untuned, quality not measured")
    ap.add_argument("--ground-strip-cell", type=float, default=None, metavar="C",
                    help=f"with --ground-strip grid: the side of a grid cell in metres (default {DEFAULT_CELL}; untuned)")
    ap.add_argument("--ground-strip-window", default=None, metavar="DOWN,UP",
                    help=f"with --ground-strip grid: the window in metres below and above the rig's height in which ground is looked for "
                         f"(default {DEFAULT_DOWN},{DEFAULT_UP}; untuned)")
    ap.add_argument("--ground-strip-quantile", type=float, default=None, metavar="Q",
                    help=f"with --ground-strip grid: the quantile of a cell's height bins that is its ground (default {DEFAULT_QUANTILE}; untuned)")
    ap.add_argument("--ground-strip-min-points", type=int, default=None, metavar="N",
                    help=f"with --ground-strip grid: a cell of fewer than N points has no ground (default {DEFAULT_MIN_POINTS}; untuned)")
    ap.add_argument("--ground-strip-margin", type=float, default=None, metavar="M",
                    help=f"with --ground-strip grid: a point less than M metres above its cell's ground is ground (default {DEFAULT_MARGIN}; untuned)")
    ap.add_argument("--ground-strip-min-keep", type=int, default=None, metavar="K",
                    help=f"with --ground-strip grid: a list that would keep fewer than K points is kept whole (default {DEFAULT_MIN_KEEP}; untuned)")


def from_namespace(args, ap=None):
    """GroundStrip from an entry point's flags; None for --ground-strip off.  A --ground-strip-* flag without --ground-strip grid is an
    error of the command line (ap.error when the parser is given, else ValueError)."""
    try:
        given = [flag for flag, v in (("--ground-strip-cell", args.ground_strip_cell), ("--ground-strip-window", args.ground_strip_window),
                                      ("--ground-strip-quantile", args.ground_strip_quantile),
                                      ("--ground-strip-min-points", args.ground_strip_min_points),
                                      ("--ground-strip-margin", args.ground_strip_margin),
                                      ("--ground-strip-min-keep", args.ground_strip_min_keep)) if v is not None]
        if args.ground_strip != "grid":
            if given:
                raise ValueError(f"{given[0]} needs --ground-strip grid")
            return None
        down, up = DEFAULT_DOWN, DEFAULT_UP
        if args.ground_strip_window is not None:
            parts = args.ground_strip_window.split(",")
            if len(parts) != 2:
                raise ValueError(f"--ground-strip-window: DOWN,UP expected, got {args.ground_strip_window!r}")
            down, up = float(parts[0]), float(parts[1])
        pick = lambda v, dflt: dflt if v is None else v
        return GroundStrip(pick(args.ground_strip_cell, DEFAULT_CELL), down, up, pick(args.ground_strip_quantile, DEFAULT_QUANTILE),
                           pick(args.ground_strip_min_points, DEFAULT_MIN_POINTS), pick(args.ground_strip_margin, DEFAULT_MARGIN),
                           pick(args.ground_strip_min_keep, DEFAULT_MIN_KEEP))
    except ValueError as e:
        if ap is None:
            raise
        ap.error(str(e))


def cells(x, y, origin, cell):
    """The rule's cell of float32 coordinates: (inside (n,) bool, index (n,) int64, valid where inside).  iu = floor(((double)x - ox) / C),
    iv alike; inside iff -32 <= iu < 32 and -32 <= iv < 32; index (iv + 32) * 64 + (iu + 32)."""
    C = np.float64(cell)
    with np.errstate(invalid="ignore", over="ignore"):
        iu = np.floor((np.asarray(x, np.float32).astype(np.float64) - np.float64(origin[0])) / C)
        iv = np.floor((np.asarray(y, np.float32).astype(np.float64) - np.float64(origin[1])) / C)
        inside = (iu >= -HALF) & (iu < HALF) & (iv >= -HALF) & (iv < HALF)              # (a NaN fails)
    idx = np.where(inside, (iv + HALF) * GROUND_GRID_CELLS + (iu + HALF), 0.0).astype(np.int64)
    return inside, idx


def ground_grid_host(points, pt_off, origin, cell=DEFAULT_CELL, down=DEFAULT_DOWN, up=DEFAULT_UP, quantile=DEFAULT_QUANTILE,
                     min_points=DEFAULT_MIN_POINTS):
    """What cm3d_ground_grid computes (include/cm3d_hip.h states the rule), to the bit.  points: (N, >= 3) float32, the frames' clouds back
    to back -- the very float32 the sweep preparation gives; a row with a non-finite coordinate is no point (so the rows the preparation
    drops may be left out or left in as NaN) --, pt_off (F + 1,) their first rows, origin (F, 3) float64.  Returns (grid_z (F, 4096)
    float64, NaN where a cell has no estimate, grid_n (F, 4096) int32).  numpy rounds every float64 operation on its own: the expressions
    below are the rule's, bracket for bracket."""
    _check(cell, down, up, quantile, min_points, 0.0, 1)
    pts = np.asarray(points, np.float32)
    pts = pts.reshape(-1, pts.shape[-1] if pts.ndim > 1 else 4)
    pt_off = np.asarray(pt_off, np.int64).reshape(-1)
    org = np.asarray(origin, np.float64).reshape(-1, 3)
    F = pt_off.size - 1
    if F < 0 or org.shape[0] != F:
        raise ValueError("one pt_off entry per frame and one more, one origin per frame")
    Q, DOWN, UP = float(quantile), np.float64(down), np.float64(up)
    dz = (DOWN + UP) / np.float64(GROUND_GRID_BINS)
    grid_z, grid_n = np.full((F, N_CELLS), np.nan), np.zeros((F, N_CELLS), np.int32)
    for f in range(F):
        if not np.isfinite(org[f]).all():
            continue
        p0 = min(max(int(pt_off[f]), 0), len(pts))
        p1 = min(max(int(pt_off[f + 1]), p0), len(pts))
        p = pts[p0:p1, :3]
        p = p[np.isfinite(p).all(1)]
        inside, idx = cells(p[:, 0], p[:, 1], org[f], cell)
        z0 = org[f, 2] - DOWN
        t = (p[:, 2].astype(np.float64) - z0) / dz
        member = inside & (t >= 0.0) & (t < float(GROUND_GRID_BINS))
        hist = np.bincount(idx[member] * GROUND_GRID_BINS + t[member].astype(np.int64), minlength=N_CELLS * GROUND_GRID_BINS)
        hist = hist.reshape(N_CELLS, GROUND_GRID_BINS)
        n = hist.sum(1)
        k = (Q * (n - 1).astype(np.float64)).astype(np.int64)                  # (int) of a value >= 0 where it is used
        b = (np.cumsum(hist, 1) > k[:, None]).argmax(1)                        # the smallest bin whose cumulative count exceeds k
        grid_n[f] = n
        grid_z[f] = np.where(n >= int(min_points), z0 + ((b.astype(np.float64) + 0.5) * dz), np.nan)
    return grid_z, grid_n


def ground_strip_host(xyz, origin, grid_z, cell=DEFAULT_CELL, margin=DEFAULT_MARGIN, min_keep=DEFAULT_MIN_KEEP):
    """What cm3d_ground_strip decides for one list: xyz (n, 3) float32 in list order, origin (3,) float64 and grid_z (4096,) of the
    list's frame (grid_z None: a frame without estimates).  Returns (keep (n,) bool, status, dropped)."""
    _check(cell, 1.0, 1.0, 0.0, 1, margin, min_keep)
    p = np.asarray(xyz, np.float32).reshape(-1, 3)
    n = p.shape[0]
    if n == 0:
        return np.zeros(0, bool), ST_EMPTY, 0
    ground = np.zeros(n, bool)
    if grid_z is not None:
        inside, idx = cells(p[:, 0], p[:, 1], origin, cell)
        z = p[:, 2].astype(np.float64)
        with np.errstate(invalid="ignore"):
            ground = inside & np.isfinite(z) & (z < np.asarray(grid_z, np.float64).reshape(N_CELLS)[idx] + np.float64(margin))
    kept = int(n - ground.sum())
    if kept < int(min_keep):
        return np.ones(n, bool), ST_KEPT_WHOLE, 0
    return ~ground, ST_STRIPPED, n - kept


def strip_lists(hit_off, hit_xyz, mask_frame, origins, grid_z, cell=DEFAULT_CELL, margin=DEFAULT_MARGIN, min_keep=DEFAULT_MIN_KEEP):
    """ground_strip_host over the lists of a batch: (gs_off, gs_tile_off, keep over all positions, gs_status, gs_dropped).  origins
    (F, 3), grid_z (F, 4096); a mask_frame outside [0, F) is a frame without estimates."""
    hit_off = np.asarray(hit_off, np.int64)
    M = hit_off.size - 1
    org, gz = np.asarray(origins, np.float64).reshape(-1, 3), np.asarray(grid_z, np.float64).reshape(-1, N_CELLS)
    xyz = np.asarray(hit_xyz)
    keep = np.zeros(int(hit_off[-1]) if M >= 0 else 0, bool)
    status, dropped = np.zeros(M, np.int32), np.zeros(M, np.int32)
    for m in range(M):
        o, e = int(hit_off[m]), int(hit_off[m + 1])
        f = int(mask_frame[m])
        ok = 0 <= f < org.shape[0]
        keep[o:e], status[m], dropped[m] = ground_strip_host(xyz[o:e, :3], org[f] if ok else np.zeros(3), gz[f] if ok else None, cell, margin,
                                                             min_keep)
    cnt = np.array([int(keep[hit_off[m]:hit_off[m + 1]].sum()) for m in range(M)], np.int64)
    gs_off = np.concatenate([[0], np.cumsum(cnt)]).astype(np.int32)
    gs_tile_off = np.concatenate([[0], np.cumsum((cnt + MEDOID_TILE - 1) // MEDOID_TILE)]).astype(np.int32)
    return gs_off, gs_tile_off, keep, status, dropped
