#!/usr/bin/env python3
"""Runs ON THE GPU BOX: what the opt-in depth clustering of the in-mask lists costs (cm3d_depth_cluster: three launches between the
compaction and the medoid), on the C2-shaped batch bench.py times and on the KITTI-shaped one of tools/kitti_obb_rate.py.  Per shape,
with HIP events and the median of --reps:
  * one pass over the resident batch without and with the clustering (eps 1 m, 20 points, the largest cluster);
  * the clustering's three launches alone, on the resident raw lists, and the medoid stage alone on the same raw lists;
  * inside the clustered pass: the span of the clustering's launches and the medoid stage on the clustered lists (stage events);
  * how many lists lose points, are kept whole, are empty, and how many points remain.
usage: tools/depth_cluster_rate.py [--frames 256] [--kitti-frames 64] [--reps 20] [--eps 1] [--min-points 20] [--out FILE.json]"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np  # noqa: E402
import torch  # noqa: E402

import bench  # noqa: E402  (make_batches_frames: the frames of a batch in forked processes)
from cm3d_amd import lifting, synthetic as syn  # noqa: E402
from tools.kitti_obb_rate import kitti_config, pass_ms  # noqa: E402


def _kitti_frames(job):
    cfg, first, n = job
    return [syn.make_kitti_frame(cfg, first + i)[0] for i in range(n)]


def staged_ms(eng, reps):
    """Median over `reps` clustered passes of (the clustering's launches, the medoid stage on the clustered lists) in ms."""
    runs = []
    for _ in range(reps):
        ev = []
        eng.run(masks="rle", stage_events=ev)
        runs.append(ev)
    torch.cuda.synchronize()
    cl = [ev[-2].elapsed_time(ev[-1]) for ev in runs]
    md = [ev[1].elapsed_time(ev[2]) - c for ev, c in zip(runs, cl)]
    return float(np.median(cl)), float(np.median(md))


def measure(hb, classes, cluster, reps):
    out = dict(frames=int(hb.n_frames), masks=int(hb.n_masks))
    res = {}
    for key, c in (("plain", None), ("clustered", cluster)):
        eng = lifting.LiftEngine("cuda:0", classes=classes, cluster=c)
        eng.upload(hb)
        for _ in range(3):
            eng.run(masks="rle")
        torch.cuda.synchronize()
        out[f"pass_ms_{key}"] = pass_ms(eng, reps)
        if c is None:
            out["medoid_stage_ms_raw_lists"] = pass_ms(eng, reps, eng.stage_medoid)
        else:
            out["cluster_stage_ms"] = pass_ms(eng, reps, eng.stage_cluster)
            out["cluster_span_in_pass_ms"], out["medoid_stage_ms_clustered_lists"] = staged_ms(eng, reps)
        res[key] = eng.download(full=True)
        del eng
        torch.cuda.empty_cache()
    a, b = res["plain"], res["clustered"]
    for key in ("hit_off", "hit_idx"):
        assert np.array_equal(a[key], b[key]), key
    n, kept, st = np.diff(a["hit_off"]), np.diff(b["cl_off"]), b["cl_status"]
    out["lists"] = dict(lose_points=int(((st == 0) & (kept < n)).sum()), chosen_whole=int(((st == 0) & (kept == n)).sum()),
                        kept_whole=int((st == 1).sum()), empty=int((st == 2).sum()), longest=int(n.max()),
                        longer_than_lds=int((n > lifting._lib.DEPTH_CLUSTER_LDS_POINTS).sum()))
    out["in_mask_points"] = dict(raw=int(n.sum()), clustered=int(kept.sum()))
    out["pass_ratio"] = out["pass_ms_clustered"] / out["pass_ms_plain"]
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=256)
    ap.add_argument("--kitti-frames", type=int, default=64)
    ap.add_argument("--kitti-points", type=int, default=120000)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--eps", type=float, default=1.0)
    ap.add_argument("--min-points", type=int, default=20)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    # the frames first: their generation forks, which a process that holds the GPU must not do
    t0 = time.time()
    c2 = bench.make_batches_frames(syn.config("c2"), [0], args.frames, 16)[0]
    kcfg = kitti_config(args.kitti_points)
    import multiprocessing
    jobs = [(kcfg, i, min(8, args.kitti_frames - i)) for i in range(0, args.kitti_frames, 8)]
    with multiprocessing.get_context("fork").Pool(min(16, len(jobs))) as pool:
        kf = [f for chunk in pool.map(_kitti_frames, jobs) for f in chunk]
    gen_s = round(time.time() - t0, 1)
    cluster = lifting.DepthCluster(args.eps, args.min_points)
    out = dict(eps=cluster.eps, min_points=cluster.min_points, pick=cluster.pick, reps=args.reps, gen_s=gen_s,
               lds_points=lifting._lib.DEPTH_CLUSTER_LDS_POINTS)
    lanes = [syn.make_lane_table([600.0, 1600.0], 50000, seed=7, extent=260.0)]
    out["c2"] = measure(lifting.pack_frames(c2, lanes, [0] * len(c2)), None, cluster, args.reps)
    del c2
    classes = lifting.ClassTable.nuscenes()
    out["kitti"] = measure(lifting.pack_frames(kf, [[[0.0, 0.0, 0.0]]], [0] * len(kf), classes), classes, cluster, args.reps)
    print(json.dumps(out), flush=True)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as fh:
            fh.write(json.dumps(out, indent=1) + "\n")


if __name__ == "__main__":
    main()
