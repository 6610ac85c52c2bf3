"""Host side of the opt-in point ownership (include/cm3d_hip.h: cm3d_point_owner; the stage in front of the ground strip in
cm3d_lift_pass_owned).

Every stage behind the compaction assumes that an in-mask list holds the points of its own object.  Nothing makes that true where masks
overlap, and they do: the 2D NMS is per class, a pedestrian's mask lies inside the mask of the bus behind them, adjacent cameras see one
object twice.  A point under two masks sits in both lists.  Here every contested point of a frame gets one owner -- the claimant that
beats all the others under a strict total order of the frame's masks -- and every list keeps the positions it owns (point_owner_host).
The table of owners is also a third product beside boxes and virtual points: one instance, class and score per LiDAR point
(label_rows).  The reference has nothing of the kind.  This module is the rule's statement to the bit, the switches of the stage
(PointOwner) and the flags of the entry points.  The device result is held against it, never the other way round.

Both defaults (rule = "score", min_keep = 5) are untuned, and what the stage does to label quality has not been measured: it cannot be on
synthetic scenes.
"""
from dataclasses import dataclass

import numpy as np

from ._lib import MEDOID_TILE

ST_OWNED, ST_KEPT_WHOLE, ST_EMPTY = 0, 1, 2                  # ow_status
RULES = ("score", "smallest")                                # rule 0, rule 1
MODES = ("off",) + RULES                                     # --point-owner
DEFAULT_RULE, DEFAULT_MIN_KEEP = "score", 5                  # untuned


def _check(rule, min_keep):
    if rule not in RULES:
        raise ValueError(f"rule: one of {RULES}")
    if int(min_keep) != min_keep or int(min_keep) < 1:
        raise ValueError("min_keep: an integer >= 1")


def rule_code(rule):
    """0 for "score", 1 for "smallest" (an integer 0 or 1 passes through)."""
    if rule in (0, 1) and not isinstance(rule, str):
        return int(rule)
    _check(rule, 1)
    return RULES.index(rule)


@dataclass
class PointOwner:
    """The opt-in point ownership of a LiftEngine (nuScenes and Waymo batches; needs no other option): a point that several masks of
    a frame list stays in the list of one of them before the strip, the clustering, the medoid and every fit see the lists.  rule:
    "score" (the higher score owns; then the shorter list; then the lower index) or "smallest" (the shorter list owns; then the higher
    score; then the lower index); min_keep: a list that would keep fewer points is kept whole.  Both untuned."""
    rule: str = DEFAULT_RULE
    min_keep: int = DEFAULT_MIN_KEEP

    def __post_init__(self):
        _check(self.rule, self.min_keep)
        self.min_keep = int(self.min_keep)

    @property
    def active(self):
        return True

    @property
    def code(self):
        return RULES.index(self.rule)

    def params(self):
        return dict(rule=self.rule, min_keep=self.min_keep)


def add_arguments(ap):
    """The flags of the nuScenes and Waymo entry points; --point-owner off (the default) is the path without the stage."""
    ap.add_argument("--point-owner", choices=MODES, default="off",
                    help="off: a point under several masks sits in all their lists; score / smallest: it stays in the list of the mask "
                         "with the highest score / the shortest list, before anything reads the lists.  Untuned, quality not measured")
    ap.add_argument("--point-owner-min-keep", type=int, default=None, metavar="K",
                    help=f"with --point-owner: a list that would keep fewer than K points is kept whole (default {DEFAULT_MIN_KEEP}; untuned)")
    ap.add_argument("--point-labels", default=None, metavar="DIR",
                    help="with --point-owner: write one .npz per frame with the owner (mask, camera, class, score) of every listed point")


def from_namespace(args, ap=None):
    """PointOwner from an entry point's flags; None for --point-owner off.  --point-owner-min-keep or --point-labels without
    --point-owner is an error of the command line (ap.error when the parser is given, else ValueError)."""
    try:
        if args.point_owner == "off":
            if args.point_owner_min_keep is not None:
                raise ValueError("--point-owner-min-keep needs --point-owner")
            if getattr(args, "point_labels", None) is not None:
                raise ValueError("--point-labels needs --point-owner")
            return None
        return PointOwner(args.point_owner, DEFAULT_MIN_KEEP if args.point_owner_min_keep is None else args.point_owner_min_keep)
    except ValueError as e:
        if ap is None:
            raise
        ap.error(str(e))


def clamped_lists(hit_off, idx_cap):
    """(lo (M,), hi (M,)) int64: every list's positions, the offsets clamped into [0, idx_cap] as cm3d_depth_cluster clamps them."""
    off = np.asarray(hit_off, np.int64).reshape(-1)
    lo = np.clip(off[:-1], 0, int(idx_cap))
    hi = np.minimum(np.maximum(off[1:], lo), int(idx_cap))
    return lo, hi


def priority_key(score, n, m, rule):
    """The key of mask m under the rule: a beats b iff key(a) > key(b).  A NaN score is lower than every number, two NaNs are equal."""
    s = float(score)
    nan = s != s
    sk = (0, 0.0) if nan else (1, s)
    return (sk, -int(n), -int(m)) if rule_code(rule) == 0 else (-int(n), sk, -int(m))


def frame_ranks(score, n, m0, m1, rule):
    """rank (m1 - m0,) int64 of the masks m0 .. m1 - 1 of one frame: the number of the frame's masks a mask beats."""
    order = sorted(range(m0, m1), key=lambda m: priority_key(score[m], n[m], m, rule))
    rank = np.zeros(m1 - m0, np.int64)
    rank[np.asarray(order, np.int64) - m0] = np.arange(m1 - m0)
    return rank


def point_owner_host(hit_idx, hit_off, mask_off, score, max_pts_per_frame, rule=DEFAULT_RULE, min_keep=DEFAULT_MIN_KEEP, idx_cap=None):
    """What cm3d_point_owner computes (include/cm3d_hip.h states the rule), to the bit.  hit_idx (n,) int32, hit_off (M + 1,), mask_off
    (F + 1,) ascending from 0 to M, score (M,) float64; idx_cap: the capacity the call is told (default: n).  Returns a dict: ow_owner
    (end,) int32 with end = the clamped end of the last list, keep (end,) bool -- the positions the ow_* lists keep --, ow_off,
    ow_tile_off (M + 1,) int32, ow_status, ow_lost (M,) int32."""
    _check(RULES[rule_code(rule)], min_keep)
    idx = np.asarray(hit_idx, np.int64).reshape(-1)
    cap = idx.size if idx_cap is None else int(idx_cap)
    lo, hi = clamped_lists(hit_off, cap)
    M = lo.size
    mo = np.clip(np.asarray(mask_off, np.int64).reshape(-1), 0, M)
    sc = np.asarray(score, np.float64).reshape(-1)
    P = int(max_pts_per_frame)
    n = hi - lo
    end = int(hi[-1]) if M else 0
    owner = np.zeros(end, np.int32)
    framed = np.zeros(M, bool)
    for f in range(mo.size - 1):
        m0, m1 = int(mo[f]), int(max(mo[f + 1], mo[f]))
        if m1 == m0:
            continue
        framed[m0:m1] = True
        rank = frame_ranks(sc, n, m0, m1, rule)
        table = np.zeros(max(P, 1), np.int64)
        by_rank = np.argsort(rank) + m0
        for m in by_rank:                                   # from the lowest priority to the highest: the last store stands
            p = idx[lo[m]:hi[m]]
            table[p[(p >= 0) & (p < P)]] = rank[m - m0] + 1
        for m in range(m0, m1):
            p = idx[lo[m]:hi[m]]
            ok = (p >= 0) & (p < P)
            owner[lo[m]:hi[m]] = np.where(ok, by_rank[table[np.where(ok, p, 0)] - 1], m)
    for m in np.flatnonzero(~framed):                       # (a mask of no frame contests nothing)
        owner[lo[m]:hi[m]] = m
    keep = np.zeros(end, bool)
    status, lost = np.zeros(M, np.int32), np.zeros(M, np.int32)
    for m in range(M):
        if n[m] == 0:
            status[m] = ST_EMPTY
            continue
        mine = owner[lo[m]:hi[m]] == m
        kept = int(mine.sum())
        if kept < int(min_keep):
            keep[lo[m]:hi[m]], status[m] = True, ST_KEPT_WHOLE
        else:
            keep[lo[m]:hi[m]], status[m], lost[m] = mine, ST_OWNED, int(n[m]) - kept
    cnt = np.array([int(keep[lo[m]:hi[m]].sum()) for m in range(M)], np.int64)
    ow_off = np.concatenate([[0], np.cumsum(cnt)]).astype(np.int32)
    ow_tile_off = np.concatenate([[0], np.cumsum((cnt + MEDOID_TILE - 1) // MEDOID_TILE)]).astype(np.int32)
    return dict(ow_owner=owner, keep=keep, ow_off=ow_off, ow_tile_off=ow_tile_off, ow_status=status, ow_lost=lost)


def owned_lists(hit_idx, hit_xyz, hit_off, res, idx_cap=None):
    """(ow_idx, ow_xyz): the lists point_owner_host's result `res` keeps, every list in its own order."""
    idx, xyz = np.asarray(hit_idx), np.asarray(hit_xyz)
    lo, hi = clamped_lists(hit_off, idx.size if idx_cap is None else idx_cap)
    sel = np.concatenate([np.arange(a, b)[res["keep"][a:b]] for a, b in zip(lo, hi)] + [np.zeros(0, np.int64)]).astype(np.int64)
    return idx[sel], xyz[sel]


def write_frame(out_dir, name, rows):
    """DIR/<name>.npz of one frame's rows (label_rows); returns the path."""
    import os
    os.makedirs(out_dir, exist_ok=True)
    path = os.path.join(out_dir, f"{name}.npz")
    np.savez(path, **{k: rows[k] for k in LABEL_FIELDS})
    return path


def write_batch(files, frames, ordinals):
    """frames: lifting.point_label_frames of one finished batch; ordinals: its frames' ordinals in the job; files: the
    virtualpoints.FrameFiles that names the job's frames (the virtual points' own naming) with --point-labels' DIR.  Returns the rows
    written."""
    n = 0
    for rows, k in zip(frames, ordinals):
        if rows is not None:
            write_frame(files.out_dir, files.names[int(k)], rows)
            n += len(rows["idx"])
    return n


LABEL_FIELDS = ("idx", "xyz", "mask", "cam", "class_id", "score", "kept", "claims")


def label_rows(f, hit_idx, hit_xyz, hit_off, mask_off, ow_owner, mask_cam, class_id, score, flags, max_pts_per_frame):
    """The painted cloud of frame f: one row per listed point of the frame, ascending by idx, as a dict of the arrays LABEL_FIELDS names
    (idx int32, xyz float32 (n, 3), mask int32 -- the owner's index in the frame's mask list --, cam, class_id int32, score float32,
    kept uint8: 1 iff the owner's (flags & 3) == 3, claims uint8: how many masks listed the point, saturating at 255).  From ow_owner
    and the raw lists: every point appears once, in its owner's list."""
    idx, xyz = np.asarray(hit_idx, np.int64), np.asarray(hit_xyz, np.float32)
    lo, hi = clamped_lists(hit_off, idx.size)
    m0, m1 = int(mask_off[f]), int(mask_off[f + 1])
    P = int(max_pts_per_frame)
    pos, listed = [], []
    for m in range(m0, m1):
        i = np.arange(lo[m], hi[m])
        i = i[(idx[i] >= 0) & (idx[i] < P)]
        listed.append(np.unique(idx[i]))
        pos.append(i[np.asarray(ow_owner)[i] == m])
    pos = np.concatenate(pos + [np.zeros(0, np.int64)]).astype(np.int64)
    pts, first = np.unique(idx[pos], return_index=True)     # (a list that names a point twice owns it once)
    pos = pos[first]
    allp, cnt = np.unique(np.concatenate(listed + [np.zeros(0, np.int64)]), return_counts=True)
    own = np.asarray(ow_owner, np.int64)[pos]
    return dict(idx=pts.astype(np.int32), xyz=np.ascontiguousarray(xyz[pos, :3], np.float32), mask=(own - m0).astype(np.int32),
                cam=np.asarray(mask_cam, np.int32)[own], class_id=np.asarray(class_id, np.int32)[own],
                score=np.asarray(score, np.float64)[own].astype(np.float32), kept=((np.asarray(flags)[own] & 3) == 3).astype(np.uint8),
                claims=np.minimum(cnt[np.searchsorted(allp, pts)], 255).astype(np.uint8))
