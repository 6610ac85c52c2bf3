"""Seeded case sets for the nuScenes matching rule (cm3d_nusc_match, cm3d_amd.nusc_eval.match_host); no GPU.

A case is (candidates, ground truth, class names or None, alphas): candidates as fusion.nusc_candidates returns them, the ground
truth as an EvalBoxes, so that the same case can be packed for the matcher and walked by a transcription of the evaluator's
own loop.  In the crafted sets every coordinate and score is a multiple of 2^-6 and every alpha of 2^-5: products, sums, squares
and comparisons are exact, so the squared-distance rule and the evaluator's norm must decide alike.
"""
import json
import os
from collections import namedtuple

import numpy as np

from cm3d_amd import _lib, eval_detection as ev, nusc_eval

Case = namedtuple("Case", "name cands gt class_names alphas")
Q = 1.0 / 64
TH = (0.5, 1.0, 2.0, 4.0)
ALPHAS97 = [k / 32.0 for k in range(1, 98)]            # 1/32 .. 97/32: 2.0 and its neighbours are in it
CLASSES = list(ev.CVPR_2019["class_range"])


class Builder:
    def __init__(self):
        self.boxes, self.kind, self.p, self.s = [], [], [], []
        self.gt = ev.EvalBoxes()
        self.n = 0

    def sample(self):
        self.n += 1
        tok = f"s{self.n:04d}"
        self.gt.add_boxes(tok, [])
        return tok

    def cand(self, tok, x, y, kind=0, p=0.0, s=0.0, name="car"):
        self.boxes.append(dict(sample_token=tok, translation=[float(x), float(y), 0.0], size=[2.0, 4.0, 1.5], rotation=[1.0, 0.0, 0.0, 0.0],
                               velocity=[0, 0], detection_name=name, detection_score=p if kind in (0, 2) else None, attribute_name=""))
        self.kind.append(kind); self.p.append(p); self.s.append(s)

    def pair(self, tok, xy_pred, xy_sam, p, s, name="car"):
        self.cand(tok, xy_pred[0], xy_pred[1], 2, p, s, name)
        self.cand(tok, xy_sam[0], xy_sam[1], 3, p, s, name)

    def truth(self, tok, x, y, name="car"):
        self.gt.boxes[tok].append(ev._box(tok, (x, y, 0.0), (2.0, 4.0, 1.5), (1.0, 0.0, 0.0, 0.0), (0.0, 0.0), 5, name, -1.0, ""))

    def case(self, name, class_names, alphas):
        return Case(name, (self.boxes, np.array(self.kind, np.int32), np.array(self.p, np.float64), np.array(self.s, np.float64)), self.gt,
                    class_names, list(alphas))


def _grid(rng, n, span=40):
    return rng.integers(-span * 64, span * 64, (n, 2)) * Q


def _fill(b, rng, tok, n_cand, n_gt, mixed, origin=(0.0, 0.0)):
    """n_gt boxes on the dyadic grid, n_cand candidates: about half near a box (within 3 m), the others anywhere; scores
    k/64 (many ties).  mixed: kinds 0..3, else all kind 0 (such a group's walk does not depend on alpha)."""
    g = _grid(rng, n_gt) + origin
    for x, y in g:
        b.truth(tok, x, y)
    left = n_cand
    while left > 0:
        near = n_gt > 0 and rng.random() < 0.5
        xy = (g[rng.integers(n_gt)] + rng.integers(-192, 193, 2) * Q) if near else _grid(rng, 1)[0] + origin
        p, s = rng.integers(1, 65) * Q, rng.integers(1, 65) * Q
        kind = int(rng.integers(0, 3)) if mixed else 0
        if kind == 2 and left >= 2:
            b.pair(tok, xy, xy + rng.integers(-64, 65, 2) * Q, p, s)
            left -= 2
        else:
            b.cand(tok, xy[0], xy[1], min(kind, 1), p, s)
            left -= 1


# (candidates, ground truth, mixed kinds): the 500-candidate group walks several 64-rank chunks with some candidates inactive
SEAM_SHAPES = [(1, 0, True), (0, 1, True), (64, 63, True), (65, 64, True), (500, 65, True), (65, 128, True), (1, 129, True),
               (_lib.NUSC_MAX_CAND, _lib.NUSC_MAX_GT, False), (0, 0, True), (64, 1, True)]


def seams(origin=(0.0, 0.0), name="seams"):
    """(candidates, ground truth) per sample at the lane, slot and chunk boundaries of the kernel; class-agnostic groups."""
    rng = np.random.default_rng(41)
    b = Builder()
    for n_cand, n_gt, mixed in SEAM_SHAPES:
        _fill(b, rng, b.sample(), n_cand, n_gt, mixed, origin)
    return b.case(name, None, ALPHAS97)


def ties(origin=(0.0, 0.0), name="ties"):
    ox, oy = origin
    b = Builder()
    rng = np.random.default_rng(42)
    t = b.sample()                                  # all scores equal: the walk is by descending position alone
    for x, y in _grid(rng, 6, 6):
        b.truth(t, ox + x, oy + y)
    for x, y in _grid(rng, 10, 6):
        b.cand(t, ox + x, oy + y, 0, 0.5)
    t = b.sample()                                  # scores that alpha clips to exactly 1.0, beside a prediction at 1.0
    for i, s in enumerate((0.5, 0.75, 1.0, 0.25)):
        b.truth(t, ox + 8.0 * i, oy)
        b.cand(t, ox + 8.0 * i + 0.25, oy, 1, 0.0, s)
    b.cand(t, ox + 0.125, oy, 0, 1.0)
    b.pair(t, (ox + 8.0, oy + 0.125), (ox + 16.0, oy + 0.125), 0.75, 0.5)
    t = b.sample()                                  # two boxes on one spot, two candidates on one spot
    b.truth(t, ox + 1.0, oy + 1.0); b.truth(t, ox + 1.0, oy + 1.0); b.truth(t, ox + 3.0, oy + 1.0)
    b.cand(t, ox + 1.25, oy + 1.0, 0, 0.5); b.cand(t, ox + 1.25, oy + 1.0, 0, 0.5); b.cand(t, ox + 1.25, oy + 1.0, 0, 0.75)
    b.cand(t, ox + 2.0, oy + 1.0, 1, 0.0, 0.5)      # the same distance to two boxes: the lower index
    for th in TH:                                   # exactly at the threshold (no match) and 2^-6 below it
        for d in (th, th - Q):
            t = b.sample()
            b.truth(t, ox + d, oy)
            b.cand(t, ox, oy, 0, 0.5)
            t = b.sample()                          # the same along y, the candidate below the box
            b.truth(t, ox, oy)
            b.cand(t, ox, oy - d, 0, 0.5)
    return b.case(name, None, ALPHAS97)


def switch(origin=(0.0, 0.0), name="switch"):
    """Pairs whose s * alpha equals p exactly at alpha = 2 (the prediction stays), with 2 -+ 1/32 in the grid; the two boxes of
    a pair lie on either side of a threshold, so the switch shows in the bits."""
    ox, oy = origin
    b = Builder()
    for i, (p, s) in enumerate(((0.5, 0.25), (0.75, 0.375), (1.0, 0.5), (0.25, 0.125), (0.5, 1.0), (0.5, 0.5))):
        t = b.sample()
        b.truth(t, ox, oy + i)
        b.truth(t, ox + 6.0, oy + i)
        b.pair(t, (ox + 0.25, oy + i), (ox + 1.5, oy + i), p, s)
        b.cand(t, ox + 5.5, oy + i, 0, 0.5)
        b.cand(t, ox + 0.375, oy + i, 1, 0.0, 0.25)
    return b.case(name, None, ALPHAS97)


def steal(origin=(0.0, 0.0), name="steal"):
    """Chains in which a higher-scored candidate takes the box a lower one is nearer to, differently at every threshold."""
    ox, oy = origin
    b = Builder()
    t = b.sample()
    b.truth(t, ox, oy); b.truth(t, ox + 3.0, oy)
    b.cand(t, ox + 1.375, oy, 0, 0.875)             # 0.5: FP; 2: takes box 0; 4: takes box 0
    b.cand(t, ox - 0.3125, oy, 0, 0.75)             # 0.5: takes box 0; 2: FP (box 1 is 3.3125 away); 4: takes box 1
    rng = np.random.default_rng(43)
    for _ in range(12):                             # a row of boxes 1.5 m apart, candidates between them, scores descending along it
        t = b.sample()
        n = int(rng.integers(3, 9))
        for j in range(n):
            b.truth(t, ox + 1.5 * j, oy + 10.0)
        for j in range(n + 2):
            b.cand(t, ox + 1.5 * j - rng.integers(20, 90) * Q, oy + 10.0, int(rng.integers(0, 2)), (64 - j) * Q, (64 - j) * Q / 2)
    return b.case(name, None, ALPHAS97)


def crafted():
    far = (2000.0, -1984.0)
    return [seams(), ties(), switch(), steal(), ties(far, "global-ties"), switch(far, "global-switch"), steal(far, "global-steal"),
            seams(far, "global-seams")]


def random_case(seed=7, n_samples=300):
    """300 samples, 10 classes, up to 40 candidates and 25 boxes per sample, scores rounded to 0.01, 60 % of the SAM3D boxes
    jittered copies of predictions (the pairs), prediction-only and ground-truth-only samples; class-aware groups."""
    rng = np.random.default_rng(seed)
    b = Builder()
    for i in range(n_samples):
        t = b.sample()
        n_gt = 0 if i % 17 == 3 else int(rng.integers(1, 26))
        n_pred = 0 if i % 19 == 5 else int(rng.integers(1, 24))
        centre = rng.uniform(-1, 1, 2) * (700.0, 1500.0)
        g = centre + rng.uniform(-45, 45, (n_gt, 2))
        g_names = [CLASSES[int(k)] for k in rng.integers(0, 10, n_gt)]
        for (x, y), nm in zip(g, g_names):
            b.truth(t, x, y, nm)
        preds = []
        for _ in range(n_pred):
            if n_gt and rng.random() < 0.7:
                k = int(rng.integers(n_gt))
                preds.append((g[k] + rng.normal(0, 0.8, 2), g_names[k] if rng.random() < 0.85 else CLASSES[int(rng.integers(10))]))
            else:
                preds.append((centre + rng.uniform(-45, 45, 2), CLASSES[int(rng.integers(10))]))
        n_sam = int(rng.integers(0, 17)) if n_pred else 0       # no prediction: no SAM3D box either, only the ground truth names the sample
        copied = set()
        sam = []
        for _ in range(n_sam):
            if preds and rng.random() < 0.6 and len(copied) < len(preds):
                k = int(rng.choice([j for j in range(len(preds)) if j not in copied]))
                copied.add(k)
                sam.append((k, preds[k][0] + rng.normal(0, 0.3, 2)))
            else:
                sam.append((None, centre + rng.uniform(-45, 45, 2)))
        score = lambda: round(float(rng.uniform(0.05, 1.0)), 2)  # noqa: E731
        p_score = [score() for _ in preds]
        for k, (xy, nm) in enumerate(preds):
            if k not in copied:
                b.cand(t, xy[0], xy[1], 0, p_score[k], 0.0, nm)
        for k, xy in sam:
            if k is None:
                b.cand(t, xy[0], xy[1], 1, 0.0, score(), CLASSES[int(rng.integers(10))])
        for k, xy in sam:
            if k is not None:
                b.pair(t, preds[k][0], xy, p_score[k], score(), preds[k][1])
    return b.case("random", CLASSES, [0.1 + 0.04 * k for k in range(97)])


def packed_of(case):
    return nusc_eval.pack(case.cands, case.gt, case.class_names, TH)


def over_capacity_case(n_cand=_lib.NUSC_MAX_CAND + 1, n_gt=3):
    """One group over the kernel's capacity between two ordinary ones."""
    rng = np.random.default_rng(44)
    b = Builder()
    _fill(b, rng, b.sample(), 30, 20, True)
    _fill(b, rng, b.sample(), n_cand, n_gt, False)
    _fill(b, rng, b.sample(), 30, 20, True)
    return b.case("over", None, ALPHAS97[:3])


# ------------------------------------------------------------------ a table set with files to fuse
def fusion_files(root, n_pairs_extra=0, seed=5, narrow=False):
    """nusc_io.write_synthetic_dataset tables + a prediction file (perturbed ground truth and clutter) + a SAM3D file (jittered
    copies of predictions and boxes of its own).  n_pairs_extra: that many more prediction / SAM3D twins in the first sample
    (a group over the kernel's candidate capacity).  narrow: scores in [0.5, 0.625], a grid of about ten alphas instead of about
    ninety.  -> (tables, pred_objects, sam3d_objects)"""
    from cm3d_amd import nusc_io, synthetic as syn
    dataroot, _, _ = nusc_io.write_synthetic_dataset(str(root), syn.config("tiny"), n_scenes=2, frames_per_scene=4)
    tables = nusc_io.NuscTables("v1.0-synth", dataroot)
    gt = ev.add_center_dist(tables, ev.load_gt(tables))
    rng = np.random.default_rng(seed)
    pred, sam = {}, {}
    p_score = lambda lo=0.1, hi=0.9: round(float(rng.uniform(0.5, 0.6) if narrow else rng.uniform(lo, hi)), 3 if narrow else 2)  # noqa: E731
    s_score = lambda: round(float(rng.uniform(0.5, 0.625) if narrow else rng.uniform(0.25, 1.0)), 3 if narrow else 2)  # noqa: E731

    def obj(tok, b, dxy, score, name=None):
        return dict(sample_token=tok, translation=[b["translation"][0] + float(dxy[0]), b["translation"][1] + float(dxy[1]), b["translation"][2]],
                    size=list(b["size"]), rotation=list(b["rotation"]), velocity=[0, 0], detection_name=name or b["detection_name"],
                    detection_score=score, attribute_name="")
    for si, tok in enumerate(gt.sample_tokens):
        pred[tok], sam[tok] = [], []
        for b in gt[tok]:
            if rng.random() < 0.8:
                pred[tok].append(obj(tok, b, rng.normal(0, 0.4, 2), p_score()))
                if rng.random() < 0.7:
                    sam[tok].append(obj(tok, pred[tok][-1], rng.normal(0, 0.15, 2), s_score()))
            if rng.random() < 0.3:
                pred[tok].append(obj(tok, b, rng.uniform(-15, 15, 2), p_score(0.1, 0.6)))
            if rng.random() < 0.3:
                sam[tok].append(obj(tok, b, rng.normal(0, 0.5, 2), s_score()))
        if si == 0 and n_pairs_extra:
            b = min((g for g in gt[tok] if ev.CVPR_2019["class_range"][g["detection_name"]] == 50), key=ev.ego_dist)
            for k in range(n_pairs_extra):
                d = (1.0 * (k % 24) - 12.0, 1.0 * (k // 24) - 11.0)
                pred[tok].append(obj(tok, b, d, p_score()))
                sam[tok].append(obj(tok, pred[tok][-1], (0.1, 0.05), s_score()))
    return tables, {"meta": {}, "results": pred}, {"meta": {}, "results": sam}


def write_json(path, obj):
    os.makedirs(os.path.dirname(os.path.abspath(str(path))), exist_ok=True)
    with open(path, "w") as f:
        json.dump(obj, f)
    return str(path)
