"""Host side of the opt-in virtual-point stage (include/cm3d_hip.h: cm3d_hit_project, cm3d_virtual_points; behind everything that
writes `flags`).

Every other stage behind the compaction refines the one box a mask gets.  This one yields the other product of a 2D -> 3D lifter:
for every instance mask, pixels sampled inside the eroded mask take the depth of the nearest LiDAR return that projects into the same
mask and are unprojected to 3D, so that a downstream detector can train on the sweep plus these points, carrying class and score.
It writes no box, flag or record.  This module is the rule's statement to the bit (virtual_points_host; steps 2 to 5 -- numpy has no
fmaf chain of its own, so step 1, the re-projection, is an input here and is held against the oracle's project_points), the switches
of the stage (VirtualPoints), the flags of the entry points and the writer of their per-frame files.  The device result is held
against it, never the other way round.

The defaults (50 points per mask, seed 0, no pixel limit, kept masks only) are untuned, and what the points do to a detector has not
been measured: it cannot be on synthetic scenes.
"""
import os
from dataclasses import dataclass

import numpy as np

from ._lib import BBOX_STRIDE, CAM_STRIDE, VP_MAX_K, VP_MAX_ROWS

ST_OK, ST_NOT_KEPT, ST_EMPTY, ST_CAMERA = 0, 1, 2, 4        # vp_status
DEFAULT_PER_MASK, DEFAULT_SEED, DEFAULT_MAX_PX = 50, 0, 0.0  # untuned
RESULTS = ("vp_count", "vp_status", "vp_xyz", "vp_pix", "vp_src", "vp_depth", "vp_d2")
FILE_FIELDS = (("xyz", np.float32), ("pixel", np.int32), ("cam", np.int32), ("mask", np.int32), ("class_id", np.int32),
               ("src_idx", np.int32), ("score", np.float32), ("depth", np.float32))      # what an entry point writes per frame
_U32 = 0xFFFFFFFF


def _check(per_mask, seed, max_px):
    if not (1 <= int(per_mask) <= VP_MAX_K):
        raise ValueError(f"1 <= per_mask <= {VP_MAX_K}")
    if not (0 <= int(seed) <= _U32):
        raise ValueError("seed: a uint32")
    if not (float(max_px) >= 0.0 and np.isfinite(max_px)):
        raise ValueError("max_px >= 0, finite (0: no limit)")


@dataclass
class VirtualPoints:
    """The opt-in virtual-point stage of a LiftEngine (any batch, with any other option or none): per_mask points sampled inside every
    eroded mask, each with the depth of the nearest return of the mask's list in the image.  seed: of the sampling; max_px: a sample
    farther than that many pixels from every return is dropped (0: no limit); kept_only: only masks with (flags & 3) == 3 get points.
    All untuned."""
    per_mask: int = DEFAULT_PER_MASK
    seed: int = DEFAULT_SEED
    max_px: float = DEFAULT_MAX_PX
    kept_only: bool = True

    def __post_init__(self):
        _check(self.per_mask, self.seed, self.max_px)
        self.per_mask, self.seed, self.max_px, self.kept_only = int(self.per_mask), int(self.seed), float(self.max_px), bool(self.kept_only)

    @property
    def active(self):
        return True


def add_arguments(ap):
    """The flags of the nuScenes and Waymo entry points; without --virtual-points the stage is off."""
    ap.add_argument("--virtual-points", default=None, metavar="DIR",
                    help="also write virtual points: pixels sampled inside every kept mask, lifted to 3D with the depth of the nearest "
                         "in-mask return; one DIR/<frame>.npz per frame with at least one point.  Untuned, effect on a detector not measured")
    ap.add_argument("--virtual-points-per-mask", type=int, default=None, metavar="K",
                    help=f"with --virtual-points: points per mask, 1..{VP_MAX_K} (default {DEFAULT_PER_MASK}; untuned)")
    ap.add_argument("--virtual-points-seed", type=int, default=None, metavar="S",
                    help=f"with --virtual-points: seed of the sampling, a uint32 (default {DEFAULT_SEED})")
    ap.add_argument("--virtual-points-max-px", type=float, default=None, metavar="R",
                    help="with --virtual-points: drop a sample farther than R pixels from every in-mask return (default 0: no limit; untuned)")
    ap.add_argument("--virtual-points-all-masks", action="store_true",
                    help="with --virtual-points: points for every mask, not only for those whose box is kept")


def from_args(args, ap=None):
    """VirtualPoints from an entry point's flags; None without --virtual-points.  A --virtual-points-* flag without --virtual-points is
    an error of the command line (ap.error when the parser is given, else ValueError)."""
    try:
        given = [flag for flag, v in (("--virtual-points-per-mask", args.virtual_points_per_mask is not None),
                                      ("--virtual-points-seed", args.virtual_points_seed is not None),
                                      ("--virtual-points-max-px", args.virtual_points_max_px is not None),
                                      ("--virtual-points-all-masks", bool(args.virtual_points_all_masks))) if v]
        if args.virtual_points is None:
            if given:
                raise ValueError(f"{given[0]} needs --virtual-points DIR")
            return None
        return VirtualPoints(DEFAULT_PER_MASK if args.virtual_points_per_mask is None else args.virtual_points_per_mask,
                             DEFAULT_SEED if args.virtual_points_seed is None else args.virtual_points_seed,
                             DEFAULT_MAX_PX if args.virtual_points_max_px is None else args.virtual_points_max_px,
                             not args.virtual_points_all_masks)
    except ValueError as e:
        if ap is None:
            raise
        ap.error(str(e))


# ---- the rule, step by step -------------------------------------------------------------------------------------------------------------
def mix(x):
    """The rule's uint32 mixer."""
    x &= _U32
    x ^= x >> 16
    x = (x * 0x7FEB352D) & _U32
    x ^= x >> 15
    x = (x * 0x846CA68B) & _U32
    x ^= x >> 16
    return x


def sample_ranks(A, per_mask, seed, frame_seed, kk):
    """Step 2: the k = min(per_mask, A) ranks r_j, ascending, one in each stratum [j*A/k, (j+1)*A/k).  Python integers: the products
    are exact, as the device's uint64 products are."""
    A, K = int(A), int(per_mask)
    k = min(K, A)
    h0 = (int(seed) ^ ((int(frame_seed) * 0x9E3779B1) & _U32) ^ ((int(kk) * 0x85EBCA77) & _U32)) & _U32
    out = np.zeros(k, np.int64)
    for j in range(k):
        lo, hi = j * A // k, (j + 1) * A // k
        out[j] = lo + mix(h0 ^ ((j * 0xC2B2AE3D) & _U32)) % (hi - lo)
    return out


def mask_pixels(slot, bb, W, H):
    """The set pixels of one eroded mask in the rule's rank order (ascending y, then x), as (px, py) int64 arrays; None where the bounds
    bb[0..3] or the stored rectangle bb[4..7] do not lie inside the image and the mask's slot (an empty mask has x0 > x1).  slot: the
    mask's H * Wp words of `packed`; only words of the eroded bounds are looked at, bits outside the bounds are cleared."""
    x0, y0, x1, y1, xw0, ys, wc, rows = (int(v) for v in bb[:BBOX_STRIDE])
    Wp = (W + 31) // 32
    ok = (0 <= x0 <= x1 < W and 0 <= y0 <= y1 < H and xw0 >= 0 and wc >= 1 and xw0 + wc <= Wp and ys >= 0 and rows >= 1 and ys + rows <= H
          and (x0 >> 5) >= xw0 and (x1 >> 5) < xw0 + wc and y0 >= ys and y1 < ys + rows)
    if not ok:
        return None
    w0, nw = x0 >> 5, (x1 >> 5) - (x0 >> 5) + 1
    words = np.asarray(slot).view(np.uint32).reshape(-1)
    r = np.arange(y0 - ys, y1 - ys + 1)[:, None] * wc + (w0 - xw0) + np.arange(nw)[None, :]
    tile = words[r].copy()                                             # (rows of the bounds, nw)
    tile[:, 0] &= np.uint32((_U32 << (x0 & 31)) & _U32)
    tile[:, nw - 1] &= np.uint32(_U32 >> (31 - (x1 & 31)))
    bits = np.unpackbits(tile.view(np.uint8).reshape(tile.shape[0], nw * 4), axis=1, bitorder="little")
    py, px = np.nonzero(bits)                                          # row-major: ascending y, then ascending x
    return px.astype(np.int64) + 32 * w0, py.astype(np.int64) + y0


def fmaf32(a, b, c):
    """float32 fmaf(a, b, c) of float32 arrays, one rounding: the product of two float32 is exact in float64; the float64 sum with c is
    rounded once too often, which matters only where it lands exactly between two float32 -- there the sum's own error (two-sum)
    says on which side the true value lies."""
    a, b, c = (np.asarray(v, np.float32).astype(np.float64) for v in (a, b, c))
    with np.errstate(over="ignore", invalid="ignore"):
        p = a * b
        s = p + c
        bb = s - p
        err = (p - (s - bb)) + (c - bb)                                # s + err == p + c exactly
        r = s.astype(np.float32)
        d = s - r.astype(np.float64)                                   # exact
        toward = np.where(d > 0, np.float32(np.inf), np.float32(-np.inf)).astype(np.float32)
        r2 = np.nextafter(r, toward)
        half = (r2.astype(np.float64) - r.astype(np.float64)) * 0.5
        tie = np.isfinite(r) & np.isfinite(r2) & (d != 0) & (d == half)
        beyond = tie & (np.sign(err) == np.sign(d))                    # the true value lies past the midpoint: the other neighbour
    return np.where(beyond, r2, r).astype(np.float32)


def nearest(uv, cx, cy):
    """Step 3 for one sample: (winner, d2) over the list's (n, 2) float32 `uv`, winner -1 where no position wins."""
    if uv.shape[0] == 0:
        return -1, np.float32(0)
    with np.errstate(over="ignore", invalid="ignore"):
        du, dv = (uv[:, 0] - np.float32(cx)).astype(np.float32), (uv[:, 1] - np.float32(cy)).astype(np.float32)
        d2 = fmaf32(dv, dv, (du * du).astype(np.float32))
    cand = np.flatnonzero(~np.isnan(d2))
    if cand.size == 0:
        return -1, np.float32(0)
    w = int(cand[np.argmin(d2[cand])])                                 # np.argmin: the first minimum
    return w, d2[w]


def camera_ok(cam):
    """Step 4's test of a camera record (float32[CAM_STRIDE])."""
    K = np.asarray(cam, np.float32)[45:54]
    ns = int(cam[54])
    return bool(0 <= ns <= 3 and K[3] == 0 and K[6] == 0 and K[7] == 0 and K[8] == 1 and np.isfinite(K[0]) and K[0] != 0
                and np.isfinite(K[4]) and K[4] != 0)


def unproject(cam, cx, cy, depth):
    """Step 4: the float64 point of pixel centre (cx, cy) -- float32 values -- at float32 `depth` through camera record `cam`.  numpy
    rounds every float64 operation on its own: the expressions are the rule's, bracket for bracket."""
    cam = np.asarray(cam, np.float32).astype(np.float64)
    K = cam[45:54]
    ns, fl = int(cam[54]), int(cam[55])
    cx, cy, d = np.float64(np.float32(cx)), np.float64(np.float32(cy)), np.float64(np.float32(depth))
    with np.errstate(over="ignore", invalid="ignore"):
        y = ((cy - K[5]) * d) / K[4]
        x = (((cx - K[2]) * d) - K[1] * y) / K[0]
        z = d
        for s in range(ns - 1, -1, -1):
            st = cam[15 * s:15 * s + 15]
            if fl & (2 << (2 * s)):
                x, y, z = x - st[12], y - st[13], z - st[14]
            R = st[3:12]
            x, y, z = ((R[0] * x + R[3] * y) + R[6] * z, (R[1] * x + R[4] * y) + R[7] * z, (R[2] * x + R[5] * y) + R[8] * z)
            if fl & (1 << (2 * s)):
                x, y, z = x - st[0], y - st[1], z - st[2]
    return np.array([x, y, z], np.float64)


def virtual_points_host(packed, bbox, W, H, cams, mask_off, mask_frame, mask_cam, flags, hit_uvd, off, idx_cap, per_mask=DEFAULT_PER_MASK,
                        seed=DEFAULT_SEED, max_px=DEFAULT_MAX_PX, kept_only=True, frame_seed=None):
    """What cm3d_virtual_points computes (include/cm3d_hip.h states the rule), to the bit.  packed: M slots of H * Wp words; bbox
    (M, BBOX_STRIDE); cams (F, n_cams, CAM_STRIDE) float32; mask_off (F + 1,), mask_frame, mask_cam, flags (M,); hit_uvd: at least
    idx_cap rows of 4 float32, step 1's result (rows from idx_cap on are never looked at); off (M + 1,); frame_seed (F,) uint32, None:
    arange(F).  Returns a dict of the seven RESULTS; rows behind a mask's count are zeros here (the device never writes them)."""
    _check(per_mask, seed, max_px)
    K, W, H, idx_cap = int(per_mask), int(W), int(H), int(idx_cap)
    bbox = np.asarray(bbox, np.int32).reshape(-1, BBOX_STRIDE)
    M = bbox.shape[0]
    cams = np.asarray(cams, np.float32)
    F, n_cams = (cams.shape[0], cams.shape[1]) if cams.ndim == 3 else (0, 0)
    if W < 1 or H < 1 or H > VP_MAX_ROWS or idx_cap < 0:
        raise ValueError(f"W, H >= 1, H <= {VP_MAX_ROWS}, idx_cap >= 0")
    Wp = (W + 31) // 32
    packed = np.asarray(packed).view(np.uint32).reshape(M, H * Wp) if M else np.zeros((0, H * Wp), np.uint32)
    mask_off, off = np.asarray(mask_off, np.int64).reshape(-1), np.asarray(off, np.int64).reshape(-1)
    mask_frame, mask_cam = np.asarray(mask_frame, np.int64).reshape(-1), np.asarray(mask_cam, np.int64).reshape(-1)
    if off.size != M + 1 or mask_frame.size != M or mask_cam.size != M or mask_off.size != F + 1:
        raise ValueError("one offset more than masks, one frame and one camera per mask, one mask offset more than frames")
    flags = None if flags is None else np.asarray(flags, np.int32).reshape(M)
    if kept_only and flags is None:
        raise ValueError("kept_only needs flags")
    frame_seed = np.arange(F, dtype=np.uint32) if frame_seed is None else np.asarray(frame_seed).astype(np.uint32).reshape(F)
    uvd = np.asarray(hit_uvd, np.float32).reshape(-1, 4)[:idx_cap]
    if uvd.shape[0] < idx_cap:
        raise ValueError("hit_uvd: fewer than idx_cap rows")
    max2 = np.float64(max_px) * np.float64(max_px)
    out = dict(vp_count=np.zeros(M, np.int32), vp_status=np.zeros(M, np.int32), vp_xyz=np.zeros((M * K, 3), np.float64),
               vp_pix=np.zeros((M * K, 2), np.int32), vp_src=np.zeros(M * K, np.int32), vp_depth=np.zeros(M * K, np.float32),
               vp_d2=np.zeros(M * K, np.float32))
    for m in range(M):
        f, c = int(mask_frame[m]), int(mask_cam[m])
        a = min(max(int(off[m]), 0), idx_cap)
        b = min(max(int(off[m + 1]), a), idx_cap)
        if kept_only and (int(flags[m]) & 3) != 3:
            out["vp_status"][m] = ST_NOT_KEPT
            continue
        if not (0 <= f < F and 0 <= c < n_cams and camera_ok(cams[f, c])):
            out["vp_status"][m] = ST_CAMERA
            continue
        pix = mask_pixels(packed[m], bbox[m], W, H) if b > a else None
        if pix is None or pix[0].size == 0:
            out["vp_status"][m] = ST_EMPTY
            continue
        px, py = pix
        ranks = sample_ranks(px.size, K, seed, frame_seed[f], m - int(mask_off[f]))
        lst = uvd[a:b]
        row = m * K
        for r in ranks:
            x, y = int(px[r]), int(py[r])
            cx, cy = np.float32(x) + np.float32(0.5), np.float32(y) + np.float32(0.5)
            w, d2 = nearest(lst[:, :2], cx, cy)
            if w < 0 or (max_px > 0 and np.float64(d2) > max2):
                continue
            out["vp_xyz"][row] = unproject(cams[f, c], cx, cy, lst[w, 2])
            out["vp_pix"][row] = x, y
            out["vp_src"][row], out["vp_depth"][row], out["vp_d2"][row] = w, lst[w, 2], d2
            row += 1
        out["vp_count"][m] = row - m * K
    return out


# ---- what an entry point writes ---------------------------------------------------------------------------------------------------------
@dataclass
class FrameFiles:
    """What an entry point's loop needs for --virtual-points: the stage, DIR, and the file stem of every frame of the whole job by the
    frame's ordinal in it (the ordinal is also the frame's seed word, so that a frame's points do not depend on how the job was cut
    into batches or ranks)."""
    stage: VirtualPoints
    out_dir: str
    names: list

    def write_batch(self, frames, ordinals):
        """frames: lifting.virtual_point_frames of one finished batch; ordinals: its frames' ordinals in the job.  Returns the points written."""
        n = 0
        for rec, k in zip(frames, ordinals):
            if rec is not None:
                write_frame(self.out_dir, self.names[int(k)], rec)
                n += len(rec["depth"])
        return n


def frame_records(res, f, per_mask, mask_off, mask_cam, class_id, score, list_off, list_idx):
    """The virtual points of frame f as the dict an entry point stores: `res` holds the seven RESULTS (numpy), list_off / list_idx the
    offsets and cloud indices of the lists the stage read (`src_idx` is the winner's index in the frame's cloud).  None for a frame
    without a point."""
    K = int(per_mask)
    m0, m1 = int(mask_off[f]), int(mask_off[f + 1])
    cnt = np.asarray(res["vp_count"][m0:m1], np.int64)
    if cnt.sum() == 0:
        return None
    masks = np.repeat(np.arange(m0, m1), cnt)
    rows = masks * K + (np.arange(masks.size) - np.repeat(np.cumsum(cnt) - cnt, cnt))
    src = np.asarray(res["vp_src"])[rows].astype(np.int64)
    vals = dict(xyz=np.asarray(res["vp_xyz"])[rows], pixel=np.asarray(res["vp_pix"])[rows], cam=np.asarray(mask_cam)[masks], mask=masks - m0,
                class_id=np.asarray(class_id)[masks], src_idx=np.asarray(list_idx)[np.asarray(list_off, np.int64)[masks] + src],
                score=np.asarray(score)[masks], depth=np.asarray(res["vp_depth"])[rows])
    return {name: np.ascontiguousarray(vals[name], dtype) for name, dtype in FILE_FIELDS}


def write_frame(out_dir, name, rec):
    """DIR/<name>.npz of one frame's records (frame_records); returns the path."""
    os.makedirs(out_dir, exist_ok=True)
    path = os.path.join(out_dir, f"{name}.npz")
    np.savez(path, **{k: np.ascontiguousarray(rec[k], dtype) for k, dtype in FILE_FIELDS})
    return path
