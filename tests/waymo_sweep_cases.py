"""Shared inputs of the alpha-sweep tests (tests/test_waymo_sweep_host.py, tests/test_gpu_waymo_sweep.py): the G11 fusion
fixture's parsed inputs, a crafted set with matched pairs and the edge cases of the candidate formulation, and the per-alpha
reference path (fuse, encode, decode, pack)."""
import functools
import math

import numpy as np

from cm3d_amd import fusion, ops, waymo as wm, waymo_eval as we
from tests.waymo_metrics_cases import blob, fixtures, generator

VEH, PED = (4.5, 2.0, 1.6), (0.9, 0.8, 1.8)
# 0: no pair takes its SAM3D box; 2: the exact-equality pair, the clip and the score tie; 1000: every pair takes it
CRAFTED_ALPHAS = [0.0, 0.5, 1.0, 2.0, 3.0, 1000.0]


def oracle_match_samples(pb, sb, iou=0.2):
    """fusion.match_samples with the CPU oracle's bev_match in the place of the GPU call (as the G11 generator does it)."""
    from oracle import oracle as orc
    pm, sm = {}, {}
    for k in pb:
        pm[k], sm[k] = [], []
        if k not in sb or not len(pb[k]) or not len(sb[k]):
            continue
        m, _, _, _ = orc.bev_match(ops.match_records(np.array(pb[k], dtype=float)), ops.match_records(np.array(sb[k], dtype=float)), iou)
        ids = np.flatnonzero(m >= 0)
        pm[k], sm[k] = [int(i) for i in ids], [int(i) for i in m[ids]]
    return pm, sm


class Inputs:
    """Parsed predictions and SAM3D boxes, their match lists and the decoded ground truth of one set."""

    def __init__(self, pred_blob, sam_blob, gt_blob, match=oracle_match_samples, matches=None):
        self.pred_objs, self.sam_objs = wm.decode_objects(pred_blob), wm.decode_objects(sam_blob)
        self.gt = we.decode_objects(gt_blob)
        self.sb, self.ss, self.s_max, self.s_min = fusion.waymo_parse(self.sam_objs, zero_min_quirk=True)
        self.pb, self.ps, self.p_max, self.p_min = fusion.waymo_parse(self.pred_objs)
        self.pm, self.sm = matches if matches is not None else match(self.pb, self.sb)

    def sides(self):
        return self.pb, self.ps, self.sb, self.ss, self.pm, self.sm

    def candidates(self):
        return fusion.waymo_candidates(*self.sides())

    def packed_candidates(self):
        return we.pack_candidates(*self.candidates(), self.gt)

    def packed_at(self, alpha):
        """What the per-alpha loop packs: the fused file encoded, decoded and grouped against the ground truth."""
        return we.pack(we.decode_objects(wm.encode_objects(fusion.fuse_waymo(*self.sides(), alpha))), self.gt)


@functools.lru_cache(None)
def g11_inputs(match=oracle_match_samples):
    f = fixtures()["fusion"]
    return Inputs(blob(f["pred"]), blob(f["sam3d"]), blob(f["gt"]), match)


def g11_alphas(inp):
    return fusion.waymo_alpha_grid(inp.p_min, inp.p_max, inp.s_min, inp.s_max)


def _pred(c, size, heading, t, score, ctx, ts):
    return wm.encode_object(c, size[0], size[1], size[2], heading, t, float(score), ctx, ts)


def _gt(c, size, heading, t, ctx, ts, pts=100):
    return we.encode_gt_object(c, size[0], size[1], size[2], heading, t, ctx, ts, pts)


def crafted_blobs():
    """24 random frames (the G11 generator's random_set) with SAM3D boxes as jittered copies of about 60 % of the predictions
    plus a few of its own, and frames that hold one edge case each (see SPECIAL)."""
    rng = np.random.default_rng(77)
    P, G = generator().random_set(rng, 24, gt_rate=6, fp_rate=2)
    S = []
    for o in wm.decode_objects(wm.encode_objects(P)):
        if rng.uniform() < 0.6:
            c = [o["center"][0] + float(rng.normal(0, 0.1)), o["center"][1] + float(rng.normal(0, 0.1)), o["center"][2] + float(rng.normal(0, 0.05))]
            S.append(wm.encode_object(c, o["length"] * float(rng.uniform(0.95, 1.05)), o["width"], o["height"],
                                      o["heading"] + float(rng.normal(0, 0.1)), o["type"], float(rng.uniform(0.25, 1)),
                                      o["context_name"], o["timestamp_micros"]))
    for f in range(0, 24, 3):              # SAM3D boxes of its own
        S.append(_pred([float(rng.uniform(-60, 60)), float(rng.uniform(-60, 60)), 0.5], VEH, float(rng.uniform(-3, 3)), 1,
                       float(rng.uniform(0.25, 1)), f"segment-{f % 13:02d}", 1_500_000_000_000_000 + 100_000 * f))
    c = "special"
    # ts 1: a pair on both sides of 30 m and one on both sides of 50 m (range shards 1 | 2 and 2 | 3)
    G += [_gt([30.0, 0.0, 0.5], VEH, 0.0, 1, c, 1), _gt([0.0, 50.0, 0.0], VEH, 0.0, 1, c, 1)]
    P += [_pred([29.9, 0.0, 0.5], VEH, 0.0, 1, 0.625, c, 1), _pred([0.0, 49.9, 0.0], VEH, 0.0, 1, 0.375, c, 1)]
    S += [_pred([30.1, 0.0, 0.5], VEH, 0.02, 1, 0.5, c, 1), _pred([0.0, 50.1, 0.0], VEH, 0.02, 1, 0.5, c, 1)]
    # ts 2: s * alpha == p exactly at alpha 2 (keeps the prediction); s * alpha > 1 at alpha 2 (clips to 1)
    G += [_gt([10.0, 0.0, 0.0], VEH, 0.0, 1, c, 2), _gt([10.0, 10.0, 0.0], VEH, 0.0, 1, c, 2)]
    P += [_pred([10.1, 0.0, 0.0], VEH, 0.0, 1, 0.5, c, 2), _pred([10.1, 10.0, 0.0], VEH, 0.0, 1, 0.875, c, 2)]
    S += [_pred([9.9, 0.0, 0.0], VEH, 0.3, 1, 0.25, c, 2), _pred([9.95, 10.0, 0.0], VEH, 0.3, 1, 0.75, c, 2)]
    # ts 3: a SAM3D score of 0 (unmatched); an unmatched SAM3D box whose score at alpha 2 equals an unmatched prediction's, both
    # on one ground-truth box with the same weight (each covers 9/16 of it, they overlap each other below the match IoU)
    G += [_gt([10.0, 0.0, 0.0], (2.0, 2.0, 1.5), 0.0, 2, c, 3), _gt([20.0, 0.0, 0.0], PED, 0.0, 2, c, 3)]
    P += [_pred([9.5625, 0.0, 0.0], (1.125, 2.0, 1.5), 0.0, 2, 0.5, c, 3)]
    S += [_pred([10.4375, 0.0, 0.0], (1.125, 2.0, 1.5), 0.0, 2, 0.25, c, 3), _pred([20.0, 0.1, 0.0], PED, 0.0, 2, 0.0, c, 3)]
    # ts 4: a pair whose SAM3D type differs from the prediction's
    G += [_gt([15.0, 5.0, 0.0], PED, 0.0, 2, c, 4)]
    P += [_pred([15.0, 5.05, 0.0], PED, 0.1, 2, 0.4375, c, 4)]
    S += [_pred([15.05, 5.0, 0.0], PED, 0.0, 4, 0.6875, c, 4)]
    # a frame only SAM3D has, a frame only the ground truth has
    S += [_pred([12.0, -8.0, 0.0], VEH, 0.5, 1, 0.5, "only-sam3d", 5)]
    G += [_gt([12.0, -8.0, 0.0], VEH, 0.5, 1, "only-sam3d", 5), _gt([12.0, 8.0, 0.0], VEH, 0.5, 1, "only-gt", 6)]
    return wm.encode_objects(P), wm.encode_objects(S), wm.encode_objects(G)


SPECIAL = {"range": ("special", 1), "scores": ("special", 2), "tie": ("special", 3), "type": ("special", 4),
           "only_sam3d": ("only-sam3d", 5), "only_gt": ("only-gt", 6)}


@functools.lru_cache(None)
def crafted_inputs(match=oracle_match_samples):
    return Inputs(*crafted_blobs(), match)


def long_alphas(n):
    """n alphas that hold CRAFTED_ALPHAS' interesting values and a fine grid around them."""
    return (CRAFTED_ALPHAS + [float(a) for a in np.arange(0.2, 0.2 + 0.013 * n, 0.013)])[:n]


SOLVER_SIZES = (64, 65, 128, 129, 256, 257)        # the sizes at which the solver changes instance, and one past them


def solver_inputs():
    """Two frames per solver size n, one type per frame, match lists given explicitly.  Every ground-truth vehicle has one
    active row on it at every alpha -- an unmatched prediction, an unmatched SAM3D box or a pair -- so that the type's shard 0
    has the same number of rows at every alpha while their order, scores and boxes change.  In the first frame of a size the
    active rows number n (n + n // 2 candidates), in the second the candidates number n (n - n // 3 rows).  Centres and
    headings are jittered.  Returns (Inputs, {frame timestamp: (rows, candidates)})."""
    rng = np.random.default_rng(404)
    P, S, G = [], [], []
    matches = ({}, {})
    sizes = {}
    plans = [(n, n // 2) for n in SOLVER_SIZES] + [(n - n // 3, n // 3) for n in SOLVER_SIZES]
    for ts, (rows, n_pairs) in enumerate(plans, start=1):
        k = ("solver", ts)
        sizes[ts] = (rows, rows + n_pairs)
        matches[0][k], matches[1][k] = [], []
        c = rng.uniform(-45, 45, (rows, 2))
        what = np.array([2] * n_pairs + [0] * ((rows - n_pairs) // 2) + [1] * (rows - n_pairs - (rows - n_pairs) // 2))
        rng.shuffle(what)
        n_p = n_s = 0
        for i in range(rows):
            h = float(rng.uniform(-math.pi, math.pi))
            G.append(_gt([c[i, 0], c[i, 1], 0.0], VEH, h, 1, k[0], ts))

            def near():
                return [c[i, 0] + float(rng.normal(0, 0.2)), c[i, 1] + float(rng.normal(0, 0.2)), float(rng.normal(0, 0.05))]
            if what[i] != 1:
                P.append(_pred(near(), VEH, h + float(rng.normal(0, 0.2)), 1, float(rng.uniform(0.05, 1)), k[0], ts))
            if what[i] != 0:
                S.append(_pred(near(), VEH, h + float(rng.normal(0, 0.2)), 1, float(rng.uniform(0.2, 1)), k[0], ts))
            if what[i] == 2:
                matches[0][k].append(n_p)
                matches[1][k].append(n_s)
            n_p += what[i] != 1
            n_s += what[i] != 0
    return Inputs(wm.encode_objects(P), wm.encode_objects(S), wm.encode_objects(G), matches=matches), sizes


SOLVER_ALPHAS = [0.3, 0.7, 1.0, 1.6, 3.0]
