#!/usr/bin/env python3
"""What the native Waymo detection metrics cost (cm3d_amd/waymo_eval.py, cm3d_waymo_metrics) on a Waymo-val-shaped synthetic
set: --frames frames (default 40 000) with ~--gt ground-truth boxes (60) and ~--pred predictions (80) a frame, types in
Waymo proportions, predictions around most of the ground truth plus false positives.  The set is built as arrays
(waymo_eval.pack_arrays); the protobuf decoding of a file of this size is pure Python and measured separately, on
--decode-frames frames.
Reports (median of --reps): the GPU call alone (ops.waymo_metrics, counts downloaded) and evaluate_packed (GPU call + AP /
APH + text on the host); pack_arrays once; decode + pack + evaluate of an encoded file of --decode-frames frames.
--gpu-only: just --reps GPU calls (for a rocprofv3 --kernel-trace --stats run of its own).
The reference binary cannot run on the GPU machine: its time is taken on the CPU build machine with --binary PATH, which
times the binary on an encoded file of --decode-frames frames and skips everything that needs a GPU.
usage: tools/waymo_metrics_rate.py [--frames 40000] [--gt 60] [--pred 80] [--reps 5] [--out FILE.json] [--gpu-only]"""
import argparse
import json
import os
import subprocess
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np  # noqa: E402

from cm3d_amd import waymo as wm, waymo_eval as we  # noqa: E402

SIZES = np.array([[0, 0, 0], [4.5, 2.0, 1.6], [0.9, 0.8, 1.8], [0.6, 0.2, 0.9], [1.8, 0.7, 1.7]])


def synth(rng, frames, n_gt, n_pred):
    g_cnt = rng.poisson(n_gt, frames)
    G = int(g_cnt.sum())
    g_frame = np.repeat(np.arange(frames), g_cnt)
    g_type = rng.choice([1, 2, 4, 3], G, p=[0.62, 0.3, 0.05, 0.03])
    g_size = SIZES[g_type] * rng.uniform(0.85, 1.15, (G, 3))
    g_c = np.stack([rng.uniform(-75, 75, G), rng.uniform(-75, 75, G), rng.uniform(-0.5, 2.5, G)], 1)
    g_h = rng.uniform(-np.pi, np.pi, G)
    pts = rng.choice([1, 4, 8, 30, 400], G)
    # predictions: ~70 % of the ground truth found (noisy), the rest false positives, ~n_pred a frame
    hit = rng.uniform(size=G) < 0.7
    src = np.flatnonzero(hit)
    n_fp = max(int(frames * n_pred) - src.size, 0)
    p_frame = np.concatenate([g_frame[src], rng.integers(0, frames, n_fp)])
    p_type = np.concatenate([g_type[src], rng.choice([1, 2, 4], n_fp, p=[0.6, 0.3, 0.1])])
    p_c = np.concatenate([g_c[src] + rng.normal(0, 0.25, (src.size, 3)),
                          np.stack([rng.uniform(-75, 75, n_fp), rng.uniform(-75, 75, n_fp), np.full(n_fp, 0.5)], 1)])
    p_size = np.concatenate([g_size[src] * rng.uniform(0.9, 1.1, (src.size, 3)), SIZES[p_type[src.size:]]])
    p_h = np.concatenate([g_h[src] + rng.normal(0, 0.3, src.size), rng.uniform(-np.pi, np.pi, n_fp)])
    p_score = rng.uniform(0, 1, p_frame.size).astype(np.float32)

    def rec(c, size, h):
        r = np.zeros((c.shape[0], we.BOX_STRIDE))
        r[:, 0], r[:, 1], r[:, 2], r[:, 3] = c[:, 0], c[:, 1], size[:, 0], size[:, 1]
        r[:, 4], r[:, 5], r[:, 6], r[:, 7] = np.cos(h), np.sin(h), c[:, 2], size[:, 2]
        return r
    pred = dict(box=rec(p_c, p_size, p_h), head=p_h.astype(np.float32), type=p_type.astype(np.int32), dist=np.linalg.norm(p_c, axis=1),
                score=p_score, frame=p_frame)
    gt = dict(box=rec(g_c, g_size, g_h), head=g_h.astype(np.float32), type=g_type.astype(np.int32), dist=np.linalg.norm(g_c, axis=1),
              level=np.where(pts <= 5, 2, 1).astype(np.int32), frame=g_frame)
    raw = dict(p=(p_frame, p_type, p_c, p_size, p_h, p_score), g=(g_frame, g_type, g_c, g_size, g_h, pts))
    return pred, gt, raw


def encode(raw, frames):
    """The first `frames` frames of the synthetic set as pred / gt Objects files (bytes)."""
    p_frame, p_type, p_c, p_size, p_h, p_score = raw["p"]
    g_frame, g_type, g_c, g_size, g_h, pts = raw["g"]
    P = [wm.encode_object(p_c[i], p_size[i, 0], p_size[i, 1], p_size[i, 2], p_h[i], int(p_type[i]), float(p_score[i]), "val", int(p_frame[i]))
         for i in np.flatnonzero(p_frame < frames)]
    G = [we.encode_gt_object(g_c[i], g_size[i, 0], g_size[i, 1], g_size[i, 2], g_h[i], int(g_type[i]), "val", int(g_frame[i]), int(pts[i]))
         for i in np.flatnonzero(g_frame < frames)]
    return wm.encode_objects(P), wm.encode_objects(G)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=40000)
    ap.add_argument("--gt", type=float, default=60)
    ap.add_argument("--pred", type=float, default=80)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--decode-frames", type=int, default=2000)
    ap.add_argument("--gpu-only", action="store_true")
    ap.add_argument("--binary", default=None, help="time this evaluator binary on the encoded --decode-frames set (CPU only)")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    rng = np.random.default_rng(7)
    t0 = time.perf_counter()
    pred, gt, raw = synth(rng, a.frames, a.gt, a.pred)
    res = dict(frames=a.frames, gt_boxes=int(gt["frame"].size), pred_boxes=int(pred["frame"].size), gen_s=time.perf_counter() - t0)
    if a.binary:
        pb, gb = encode(raw, a.decode_frames)
        with tempfile.TemporaryDirectory() as d:
            open(os.path.join(d, "p.bin"), "wb").write(pb)
            open(os.path.join(d, "g.bin"), "wb").write(gb)
            t0 = time.perf_counter()
            subprocess.run(["/lib64/ld-linux-x86-64.so.2", a.binary, os.path.join(d, "p.bin"), os.path.join(d, "g.bin")],
                           check=True, capture_output=True)
            res.update(binary_frames=a.decode_frames, binary_s=time.perf_counter() - t0, where="CPU build machine, single-threaded binary")
        print(json.dumps(res, indent=1))
        if a.out:
            json.dump(res, open(a.out, "w"), indent=1)
        return
    import torch
    from cm3d_amd import ops
    t0 = time.perf_counter()
    packed = we.pack_arrays(pred, gt, a.frames)
    res["pack_arrays_s"] = time.perf_counter() - t0
    res["groups"] = int(packed["group_bd"].size)
    po, go = packed["pred_off"], packed["gt_off"]
    res["pairs"] = int(np.sum(np.diff(po) * np.diff(go)))
    res["largest_group_side"] = int(np.max(np.maximum(np.diff(po), np.diff(go))))
    ops.waymo_metrics(packed)                                   # warm-up (module load, allocator)
    torch.cuda.synchronize()
    gpu = []
    for _ in range(a.reps):
        t0 = time.perf_counter()
        ops.waymo_metrics(packed)
        gpu.append(time.perf_counter() - t0)
    res["gpu_call_s_median"] = float(np.median(gpu))
    if a.gpu_only:
        print(json.dumps(res, indent=1))
        return
    ev = []
    for _ in range(a.reps):
        t0 = time.perf_counter()
        ap_dict, text = we.evaluate_packed(packed)
        ev.append(time.perf_counter() - t0)
    res["evaluate_packed_s_median"] = float(np.median(ev))
    res["frames_per_s_evaluate_packed"] = a.frames / res["evaluate_packed_s_median"]
    res["overall_l2_map"] = ap_dict["Overall/L2 mAP"]
    pb, gb = encode(raw, a.decode_frames)
    t0 = time.perf_counter()
    objs = we.decode_objects(pb), we.decode_objects(gb)
    t1 = time.perf_counter()
    we.evaluate(*objs)
    t2 = time.perf_counter()
    res.update(file_frames=a.decode_frames, file_bytes=len(pb) + len(gb), decode_s=t1 - t0, evaluate_from_objects_s=t2 - t1)
    print(json.dumps(res, indent=1))
    print(text.splitlines()[0])
    if a.out:
        json.dump(res, open(a.out, "w"), indent=1)


if __name__ == "__main__":
    main()
