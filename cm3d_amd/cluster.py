"""Host side of the depth clustering of the in-mask lists (include/cm3d_hip.h: cm3d_depth_cluster; a stage of cm3d_lift_pass_opt).

The reference carries a clustering step it never calls: clusters_hdbscan (src/kitti/2d_to_3d.py:159-174, src/waymo/2d_to_3d.py:102-117,
min_cluster_size=20, cluster_selection_epsilon=1; its only call site is commented out at src/kitti/2d_to_3d.py:1192).  What stands
here in its place is a 1-D gap clustering on the range from the sensor rig -- the depth along the mask's frustum.  A 1-D key makes the
result independent of the order in which points are processed, which 3-D DBSCAN is not, and it can be stated to the bit, which HDBSCAN
cannot: this module is that statement (depth_cluster_host), and the switches of the clustered pass (DepthCluster).
"""
from dataclasses import dataclass

import numpy as np

PICKS = ("largest", "nearest")                     # cm3d_depth_cluster's pick 0 / 1
KEPT, KEPT_WHOLE, EMPTY = 0, 1, 2                  # cl_status: a cluster chosen; none qualifies, list kept whole; empty list


def pick_code(pick):
    if pick in PICKS:
        return PICKS.index(pick)
    if pick in (0, 1) and not isinstance(pick, bool):
        return int(pick)
    raise ValueError(f"pick: one of {PICKS}")


@dataclass
class DepthCluster:
    """The opt-in depth clustering of a LiftEngine: every mask's in-mask points are clustered by their range from the frame's origin
    (gaps of more than `eps` metres separate clusters), and the medoid and the box fit see only the chosen cluster -- the largest one of
    at least `min_points` points (the nearer on a tie), or with pick="nearest" the first such one; a list without such a cluster is
    kept whole.  The reference's commented-out values are eps 1 and min_points 20."""
    eps: float
    min_points: int = 20
    pick: str = "largest"

    def __post_init__(self):
        self.eps = float(self.eps)
        if not self.eps > 0.0:                     # (NaN fails the comparison)
            raise ValueError("eps > 0 (inf: one cluster)")
        if int(self.min_points) != self.min_points or int(self.min_points) < 1:
            raise ValueError("min_points: an integer >= 1")
        self.min_points = int(self.min_points)
        self.pick = PICKS[pick_code(self.pick)]

    @property
    def active(self):
        return True

    @property
    def pick_index(self):
        return PICKS.index(self.pick)

    @staticmethod
    def from_args(eps=None, min_points=20, pick="largest"):
        """From an entry point's flags (eps None = --depth-cluster not given); None when the flag is absent."""
        return None if eps is None else DepthCluster(eps, 20 if min_points is None else min_points, pick or "largest")


def add_arguments(ap):
    """The three flags every lifting entry point carries; absent --depth-cluster means off."""
    ap.add_argument("--depth-cluster", type=float, default=None, metavar="EPS",
                    help="cluster every mask's points by their range from the sensor rig (gaps above EPS metres separate clusters) and lift "
                         "only the chosen cluster; the reference's commented-out clustering used 1")
    ap.add_argument("--depth-cluster-min-points", type=int, default=20, metavar="N",
                    help="points a cluster needs to be chosen; a mask without such a cluster keeps all its points")
    ap.add_argument("--depth-cluster-pick", choices=PICKS, default="largest",
                    help="largest: the cluster of most points, the nearer on a tie; nearest: the first one of at least N points")


def from_namespace(args):
    return DepthCluster.from_args(args.depth_cluster, args.depth_cluster_min_points, args.depth_cluster_pick)


def ranges(xyz, origin):
    """The key: float64 range of float32 points from `origin` (3,), r = sqrt((dx*dx + dy*dy) + dz*dz)."""
    p = np.asarray(xyz, np.float32).reshape(-1, 3).astype(np.float64)
    o = np.asarray(origin, np.float64).reshape(3)
    dx, dy, dz = p[:, 0] - o[0], p[:, 1] - o[1], p[:, 2] - o[2]
    return np.sqrt((dx * dx + dy * dy) + dz * dz)


def depth_cluster_host(xyz, origin, eps, min_points=20, pick="largest"):
    """The statement cm3d_depth_cluster is held against, for one list: xyz (n, 3) float32 in list order, origin (3,) float64.
    Returns (keep (n,) bool, status)."""
    eps, min_points, pick = float(eps), int(min_points), pick_code(pick)
    if not eps > 0.0 or min_points < 1:
        raise ValueError("eps > 0, min_points >= 1")
    r = ranges(xyz, origin)
    n = r.size
    if n == 0:
        return np.zeros(0, bool), EMPTY
    order = np.argsort(r, kind="stable")           # by (r, position)
    rs = r[order]
    with np.errstate(invalid="ignore"):
        starts = np.concatenate([[0], np.flatnonzero(rs[1:] - rs[:-1] > eps) + 1])
    sizes = np.diff(np.concatenate([starts, [n]]))
    ok = np.flatnonzero(sizes >= min_points)
    keep = np.ones(n, bool)
    if ok.size == 0:
        return keep, KEPT_WHOLE
    c = int(ok[0]) if pick == 1 else int(ok[np.argmax(sizes[ok])])       # (argmax: the first of the largest = the nearest of them)
    keep[:] = False
    keep[order[starts[c]:starts[c] + sizes[c]]] = True
    return keep, KEPT


def cluster_lists(hit_off, hit_xyz, mask_frame, origins, eps, min_points=20, pick="largest"):
    """depth_cluster_host over the lists of a batch: (cl_off, cl_tile_off, keep over all positions, cl_status)."""
    from ._lib import MEDOID_TILE
    hit_off = np.asarray(hit_off, np.int64)
    M = hit_off.size - 1
    keep = np.zeros(int(hit_off[-1]), bool)
    status = np.zeros(M, np.int32)
    for m in range(M):
        o, e = int(hit_off[m]), int(hit_off[m + 1])
        keep[o:e], status[m] = depth_cluster_host(np.asarray(hit_xyz)[o:e, :3], np.asarray(origins, np.float64).reshape(-1, 3)[int(mask_frame[m])],
                                                  eps, min_points, pick)
    cnt = np.array([int(keep[hit_off[m]:hit_off[m + 1]].sum()) for m in range(M)], np.int64)
    cl_off = np.concatenate([[0], np.cumsum(cnt)]).astype(np.int32)
    cl_tile_off = np.concatenate([[0], np.cumsum((cnt + MEDOID_TILE - 1) // MEDOID_TILE)]).astype(np.int32)
    return cl_off, cl_tile_off, keep, status
