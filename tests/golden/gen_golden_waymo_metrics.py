#!/usr/bin/env python3
"""G11: the Waymo detection metrics (cm3d_amd/waymo_eval.py) pinned against the output of the reference checkout's own
evaluator binary, src/waymo/compute_detection_metrics_main (waymo-open-dataset's tool as mmdetection3d builds it; an
x86-64 ELF that runs on the CPU build machine through the dynamic loader, never on the GPU box).

For each case this writes synthetic pred / ground-truth `metrics_pb2.Objects` files, runs the binary on them and keeps
the 32 breakdown lines it prints.  A last case runs fusion.waymo_grid_search with the binary as its evaluator (the box
matching of the fusion step through the CPU oracle) and keeps every alpha's Overall/L2 mAP, the best alpha and the
best file's hash.

Writes tests/golden/g11_waymo_metrics.json.gz (inputs base64, printed lines) and its log, g11_waymo_metrics_report.json
(source of the numbers, the fixture's sha256, case sizes).  The shared gen_report.json of the older goldens stays as it is.
Usage: python tests/golden/gen_golden_waymo_metrics.py [--bin PATH]   (from the repo root)
"""
import argparse
import base64
import gzip
import hashlib
import json
import math
import os
import subprocess
import sys
import tempfile

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)
REF_BIN = "/root/reference/src/waymo/compute_detection_metrics_main"
LOADER = "/lib64/ld-linux-x86-64.so.2"
OUT = os.path.join(HERE, "g11_waymo_metrics.json.gz")
REPORT = os.path.join(HERE, "g11_waymo_metrics_report.json")

from cm3d_amd import waymo as wm, waymo_eval as we  # noqa: E402

SIZES = {1: (4.5, 2.0, 1.6), 2: (0.9, 0.8, 1.8), 3: (0.6, 0.2, 0.9), 4: (1.8, 0.7, 1.7)}      # length, width, height per type


def pred(c, size, heading, t, score, ctx="ctx", ts=1):
    return wm.encode_object(c, size[0], size[1], size[2], heading, t, float(score), ctx, ts)


def gt(c, size, heading, t, ctx="ctx", ts=1, pts=100, diff=None):
    return we.encode_gt_object(c, size[0], size[1], size[2], heading, t, ctx, ts, pts, diff)


def offset_for_iou(L, target):
    """Shift along the length that gives two equal boxes this IoU: (L - d) / (L + d)."""
    return L * (1.0 - target) / (1.0 + target)


def case_iou_thresholds():
    P, G = [], []
    ts = 1
    for t, thr in ((1, 0.7), (2, 0.5), (4, 0.5), (3, 0.5)):
        L, W, H = SIZES[t]
        for k, step in enumerate((-2e-3, -2e-4, 2e-4, 2e-3)):
            y = 6.0 * k - 9.0
            x = 12.0 + 8.0 * t
            s = 0.3 + 0.15 * k
            G.append(gt([x, y, 0.5], (L, W, H), 0.0, t, ts=ts))                      # shift along the length
            P.append(pred([x + offset_for_iou(L, thr + step), y, 0.5], (L, W, H), 0.0, t, s, ts=ts))
            G.append(gt([x, y + 3.0, 0.5], (L, W, H), 0.0, t, ts=ts + 1))             # z offset only
            P.append(pred([x, y + 3.0, 0.5 + offset_for_iou(H, thr + step)], (L, W, H), 0.0, t, s, ts=ts + 1))
            # rotated pair, both boxes turned: the binary's polygon IoU of rotated boxes departs from the exact one by up
            # to ~2e-4 near the threshold (one vehicle pair at 0.7 - 2e-4 matched there), so these pairs keep 5e-3 away
            hd = 0.4 * k + 0.1
            c, sn = math.cos(hd), math.sin(hd)
            d = offset_for_iou(L, thr + math.copysign(5e-3, step))
            G.append(gt([x, y - 3.0, 0.5], (L, W, H), hd, t, ts=ts + 2))
            P.append(pred([x + d * c, y - 3.0 + d * sn, 0.5], (L, W, H), hd, t, s, ts=ts + 2))
        ts += 3
    # a rotated prediction on an axis-aligned ground truth, vehicle and pedestrian
    for t, ang in ((1, 0.05), (1, 0.12), (1, 0.3), (2, 0.4), (2, 1.0), (4, 0.2)):
        L, W, H = SIZES[t]
        G.append(gt([20.0, 20.0 + 5 * ang, 0.0], (L, W, H), 0.0, t, ts=ts))
        P.append(pred([20.0, 20.0 + 5 * ang, 0.0], (L, W, H), ang, t, 0.77, ts=ts))
    return P, G


def case_headings():
    P, G = [], []
    sq = (2.0, 2.0, 1.5)
    for k, (g_h, p_h) in enumerate(((0.0, 0.0), (0.0, math.pi / 2), (0.0, math.pi), (0.0, -math.pi), (3.1, -3.1), (-3.1, 3.1),
                                    (math.pi, -math.pi), (0.3, 0.3 + 2 * math.pi), (1.0, -2.0), (0.0, math.pi - 1e-7))):
        G.append(gt([10.0 + 3 * k, 0.0, 0.0], sq, g_h, 1, ts=1 + k % 3))
        P.append(pred([10.0 + 3 * k, 0.0, 0.0], sq, p_h, 1, 0.2 + 0.07 * k, ts=1 + k % 3))
    for k, p_h in enumerate((0.0, math.pi / 2, math.pi, 2.5)):
        G.append(gt([10.0 + 3 * k, 8.0, 0.0], (0.8, 0.8, 1.8), 0.0, 2, ts=5))
        P.append(pred([10.0 + 3 * k, 8.0, 0.0], (0.8, 0.8, 1.8), p_h, 2, 0.9 - 0.1 * k, ts=5))
    return P, G


def case_difficulty():
    P, G = [], []
    L = SIZES[1]
    specs = ((0, None, True), (1, None, True), (5, None, True), (6, None, True), (200, None, True), (200, 2, True), (3, 1, True),
             (0, None, False), (1, None, False), (5, None, False), (6, None, False), (200, None, False), (200, 2, False), (3, 1, False),
             (4, 2, False), (50, 1, False))
    for k, (pts, diff, with_pred) in enumerate(specs):
        x = 10.0 + 6.0 * (k % 7)
        y = -10.0 + 7.0 * (k // 7)
        G.append(gt([x, y, 0.0], L, 0.0, 1, ts=1 + k % 2, pts=pts, diff=diff))
        if with_pred:
            P.append(pred([x + 0.1, y, 0.0], L, 0.0, 1, 0.95 - 0.05 * k, ts=1 + k % 2))
    # one prediction between a LEVEL_2 ground truth (closer) and a LEVEL_1 one
    G.append(gt([10.0, 30.0, 0.0], L, 0.0, 1, ts=3, pts=2))
    G.append(gt([10.3, 30.0, 0.0], L, 0.0, 1, ts=3, pts=100))
    P.append(pred([10.05, 30.0, 0.0], L, 0.0, 1, 0.6, ts=3))
    for k in range(6):                 # cyclists with few points
        G.append(gt([8.0 + 3 * k, -5.0, 0.0], SIZES[4], 0.0, 4, ts=4, pts=(3, 7)[k % 2]))
        if k % 3:
            P.append(pred([8.0 + 3 * k, -5.0, 0.0], SIZES[4], 0.1, 4, 0.3 + 0.1 * k, ts=4))
    return P, G


def case_ranges():
    P, G = [], []
    for k, r in enumerate((29.9, 30.0, 49.9, 50.0, 29.95)):
        for t in (1, 2):
            ang = 0.3 + 0.7 * k + 0.2 * t
            c = [r * math.cos(ang), r * math.sin(ang), 0.0]
            if k == 4:
                c = [29.95 * math.cos(ang), 29.95 * math.sin(ang), 3.0]            # BEV inside 30 m, 3D distance beyond
            G.append(gt(c, SIZES[t], ang, t, ts=1))
            P.append(pred(c, SIZES[t], ang, t, 0.4 + 0.1 * k, ts=1))
    # prediction and ground truth overlapping across the 30 m boundary
    G.append(gt([30.02, 0.0, 0.0], SIZES[1], 0.0, 1, ts=2))
    P.append(pred([29.97, 0.0, 0.0], SIZES[1], 0.0, 1, 0.8, ts=2))
    G.append(gt([0.0, 49.98, 0.0], SIZES[1], 0.0, 1, ts=2))
    P.append(pred([0.0, 50.01, 0.0], SIZES[1], 0.0, 1, 0.7, ts=2))
    return P, G


def case_scores():
    P, G = [], []
    L = SIZES[1]
    scores = (0.5, 0.51, 0.0, 1.0, 0.6, 0.6, 0.6, 0.05, 0.99, 0.5, 0.25)
    for k, s in enumerate(scores):
        x = 8.0 + 6.0 * k
        G.append(gt([x, 0.0, 0.0], L, 0.0, 1, ts=1))
        if k % 4 != 3 or s == 1.0:
            P.append(pred([x + 0.15 * (k % 3), 0.0, 0.0], L, 0.0, 1, s, ts=1))
        P.append(pred([x, 20.0, 0.0], L, 0.0, 1, scores[-1 - k], ts=1))            # false positives with the same scores
    return P, G


def case_frames():
    P, G = [], []
    L = SIZES[1]
    P.append(pred([10.0, 0.0, 0.0], L, 0.0, 1, 0.9, "a", 1))                      # frame with predictions only
    P.append(pred([15.0, 0.0, 0.0], L, 0.0, 1, 0.4, "a", 1))
    G.append(gt([10.0, 0.0, 0.0], L, 0.0, 1, "a", 2))                            # ground truth only
    G.append(gt([10.0, 0.0, 0.0], L, 0.0, 1, "b", 1))                            # a normal frame
    P.append(pred([10.1, 0.0, 0.0], L, 0.0, 1, 0.7, "b", 1))
    G.append(gt([10.0, 0.0, 0.0], L, 0.0, 1, "b", 2, pts=0))                     # its only object has no points: an empty frame
    P.append(pred([12.0, 4.0, 0.0], SIZES[2], 0.0, 2, 0.6, "c", 7))               # pred file only
    G.append(gt([12.0, 4.0, 0.0], SIZES[2], 0.0, 2, "d", 7))                     # gt file only
    G.append(gt([14.0, 4.0, 0.0], SIZES[2], 0.0, 2, "b", 1))
    P.append(pred([14.0, 4.1, 0.0], SIZES[2], 0.0, 2, 0.55, "b", 1))
    return P, G


def case_duplicates(rng):
    P, G = [], []
    L = SIZES[1]
    for k in range(4):                 # several predictions on one ground truth, distinct IoUs and headings
        x = 10.0 + 8.0 * k
        G.append(gt([x, 0.0, 0.0], L, 0.0, 1, ts=1))
        for j in range(4):
            P.append(pred([x + 0.05 + 0.11 * j, 0.02 * j, 0.0], L, 0.1 * j, 1, 0.9 - 0.13 * j - 0.01 * k, ts=1))
    for ts, n in ((2, 120), (3, 300)):  # crowded frames
        c = rng.uniform(-60, 60, (n, 2))
        t = rng.choice([1, 2, 4], n, p=[0.5, 0.35, 0.15])
        for i in range(n):
            sz = SIZES[int(t[i])]
            h = float(rng.uniform(-math.pi, math.pi))
            G.append(gt([c[i, 0], c[i, 1], 0.0], sz, h, int(t[i]), ts=ts, pts=int(rng.choice([3, 20, 300]))))
            for _ in range(int(rng.integers(0, 3))):
                P.append(pred([c[i, 0] + rng.normal(0, 0.15), c[i, 1] + rng.normal(0, 0.15), rng.normal(0, 0.1)], sz,
                              h + rng.normal(0, 0.3), int(t[i]), float(rng.uniform(0, 1)), ts=ts))
    return P, G


def random_set(rng, n_frames, gt_rate=8, fp_rate=3, min_score=0.0):
    """A Waymo-shaped synthetic set: per frame a few contexts / timestamps, ground truth of all types with point counts and
    difficulty levels, predictions around most of it (noise, flipped headings) and false positives."""
    P, G = [], []
    for f in range(n_frames):
        ctx, ts = f"segment-{f % 13:02d}", 1_500_000_000_000_000 + 100_000 * f
        for _ in range(int(rng.poisson(gt_rate))):
            t = int(rng.choice([1, 2, 4, 3], p=[0.6, 0.25, 0.1, 0.05]))
            sz = tuple(float(s) * float(rng.uniform(0.85, 1.15)) for s in SIZES[t])
            c = [float(rng.uniform(-75, 75)), float(rng.uniform(-75, 75)), float(rng.uniform(-0.5, 2.5))]
            h = float(rng.uniform(-math.pi, math.pi))
            diff = int(rng.choice([0, 1, 2], p=[0.7, 0.15, 0.15]))
            G.append(gt(c, sz, h, t, ctx, ts, pts=int(rng.choice([0, 1, 4, 5, 6, 30, 400])), diff=diff or None))
            for _ in range(int(rng.choice([0, 1, 1, 1, 2]))):
                cc = [c[0] + float(rng.normal(0, 0.25)), c[1] + float(rng.normal(0, 0.25)), c[2] + float(rng.normal(0, 0.1))]
                ss = tuple(s * float(rng.uniform(0.9, 1.1)) for s in sz)
                hh = h + float(rng.normal(0, 0.3)) + float(rng.choice([0.0, math.pi], p=[0.85, 0.15]))
                P.append(pred(cc, ss, hh, t, float(rng.uniform(min_score, 1)), ctx, ts))
        for _ in range(int(rng.poisson(fp_rate))):
            t = int(rng.choice([1, 2, 4]))
            P.append(pred([float(rng.uniform(-75, 75)), float(rng.uniform(-75, 75)), 0.5], SIZES[t], float(rng.uniform(-3, 3)), t,
                          float(rng.uniform(min_score, 1)), ctx, ts))
    return P, G


def run_bin(binary, pred_blob, gt_blob):
    with tempfile.TemporaryDirectory() as d:
        pp, gp = os.path.join(d, "pred.bin"), os.path.join(d, "gt.bin")
        open(pp, "wb").write(pred_blob)
        open(gp, "wb").write(gt_blob)
        out = subprocess.run([LOADER, binary, pp, gp], capture_output=True, text=True, check=True).stdout
    lines = [l.rstrip() for l in out.splitlines() if l.startswith(("OBJECT_TYPE_TYPE_", "RANGE_TYPE_"))]
    assert len(lines) == 32, out[-2000:]
    return "\n".join(lines) + "\n"


def fusion_case(binary, rng):
    """waymo_grid_search with the binary as evaluate(); the per-frame matching through the CPU oracle."""
    from cm3d_amd import fusion, ops
    from oracle import oracle as orc

    def cpu_match(pred_boxes, gt_boxes, iou=0.2):
        out = []
        for p, g in zip(pred_boxes, gt_boxes):
            pm, gm, io, _ = orc.bev_match(ops.match_records(p), ops.match_records(g), iou)
            ids = np.flatnonzero(pm >= 0)
            out.append((ids.astype(np.int64), pm[ids].astype(np.int64), io[ids]))
        return out
    ops.bev_match = cpu_match
    Pp, G = random_set(rng, 24, gt_rate=6, fp_rate=2)
    Ps, _ = random_set(np.random.default_rng(99), 24, gt_rate=6, fp_rate=2, min_score=0.25)      # a grid of ~100 alphas
    pred_blob, sam_blob, gt_blob = wm.encode_objects(Pp), wm.encode_objects(Ps), wm.encode_objects(G)
    scores = []
    with tempfile.TemporaryDirectory() as d:
        gp = os.path.join(d, "gt.bin")
        open(gp, "wb").write(gt_blob)

        def evaluate(path):
            text = subprocess.run([LOADER, binary, path, gp], capture_output=True, text=True, check=True).stdout
            s = fusion.parse_waymo_metrics(text)[1]
            scores.append(s)
            return s
        best = os.path.join(d, "best.bin")
        alpha, score = fusion.waymo_grid_search(wm.decode_objects(pred_blob), wm.decode_objects(sam_blob), evaluate,
                                                os.path.join(d, "cur.bin"), best, verbose=False)
        best_hash = hashlib.sha256(open(best, "rb").read()).hexdigest()
    return dict(pred=base64.b64encode(pred_blob).decode(), sam3d=base64.b64encode(sam_blob).decode(),
                gt=base64.b64encode(gt_blob).decode(), scores=scores, best_alpha=float(alpha), best_score=float(score),
                best_sha256=best_hash)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--bin", default=REF_BIN)
    a = ap.parse_args()
    rng = np.random.default_rng(11)
    cases = {"iou_thresholds": case_iou_thresholds(), "headings": case_headings(), "difficulty": case_difficulty(),
             "ranges": case_ranges(), "scores": case_scores(), "frames": case_frames(), "duplicates": case_duplicates(rng),
             "random": random_set(rng, 200, gt_rate=5, fp_rate=2)}
    out = {"cases": {}}
    for name, (P, G) in cases.items():
        pb, gb = wm.encode_objects(P), wm.encode_objects(G)
        out["cases"][name] = dict(pred=base64.b64encode(pb).decode(), gt=base64.b64encode(gb).decode(), text=run_bin(a.bin, pb, gb))
        print(name, len(P), "predictions", len(G), "ground truth")
    out["fusion"] = fusion_case(a.bin, rng)
    raw = json.dumps(out, sort_keys=True).encode()
    with open(OUT, "wb") as f:
        f.write(gzip.compress(raw, 9, mtime=0))
    report = {
        "G11 waymo metrics": ("printed output of the reference's src/waymo/compute_detection_metrics_main (waymo-open-dataset "
                              "evaluator, mmdetection3d build) on synthetic Objects files; fusion case scored by the same binary"),
        "G11 g11_waymo_metrics.json.gz sha256": hashlib.sha256(open(OUT, "rb").read()).hexdigest(),
        "G11 cases: name / predictions / ground truth": [[n, len(P), len(G)] for n, (P, G) in cases.items()],
        "G11 fusion: alphas / best alpha / best Overall L2 mAP": [len(out["fusion"]["scores"]), out["fusion"]["best_alpha"],
                                                                  out["fusion"]["best_score"]],
    }
    with open(REPORT, "w") as f:
        json.dump(report, f, indent=1)
        f.write("\n")
    print(OUT, os.path.getsize(OUT), "bytes")


if __name__ == "__main__":
    main()
