#!/usr/bin/env python3
"""Runs ON THE GPU BOX: what the opt-in vertical stage costs (cm3d_box_vertical: one launch behind the pass), with HIP events and the
median of --reps, on the C2-shaped batch bench.py times (256 frames x 20 masks) and on the Waymo-shaped batch of C4 frames that
tools/bev_fit_rate.py uses.  Per batch, in one run:

  * cm3d_box_vertical alone, cm3d_bev_fit alone and the depth clustering alone on the resident lists -- the two yardsticks walk the
    same lists, and the clustering sorts them -- and the two ratios;
  * one pass over the resident batch without the option and with it, and the span of the stage's two events inside the pass;
  * how many masks take each vert_src and each vert_status, the longest list, and how many lists go each route of the kernel.

Every timed configuration is first held against the host statement.  The synthetic lists are frustum points, not objects: the counts
say how much work the launch had, nothing about real scenes.  Run it as one step under a time limit of its own, like the other rate
tools: timeout -k 10 900 python tools/box_vertical_rate.py --out profiles/box_vertical_rate.json
usage: tools/box_vertical_rate.py [--frames 256] [--waymo-frames 32] [--reps 20] [--out FILE.json]"""
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
from cm3d_amd import bevfit, boxvertical, cluster, lifting, synthetic as syn  # noqa: E402
from tools.bev_fit_rate import _waymo_frames, span_ms  # noqa: E402
from tools.kitti_obb_rate import pass_ms  # noqa: E402


def measure(hb, classes, reps):
    out = dict(frames=int(hb.n_frames), masks=int(hb.n_masks))
    v = boxvertical.BoxVertical()
    res = {}
    for key, kw in (("plain", {}), ("vertical", dict(vertical=v)), ("yaw", dict(yaw=bevfit.YawFit())), ("cluster", dict(cluster=cluster.DepthCluster(1.0)))):
        eng = lifting.LiftEngine("cuda:0", classes=classes, **kw)
        eng.upload(hb)
        for _ in range(3):
            eng.run(masks="rle")
        torch.cuda.synchronize()
        if key in ("plain", "vertical"):
            out[f"pass_ms_{key}"] = pass_ms(eng, reps)
        if key == "vertical":
            out["box_vertical_alone_ms"] = pass_ms(eng, reps, eng.stage_vertical)
            out["vertical_span_in_pass_ms"] = span_ms(eng, reps)
            eng.run(masks="rle")                      # (the stage alone left its own z as the entry values: one whole pass again)
            torch.cuda.synchronize()
            res[key] = eng.download(full=True)
        elif key == "yaw":
            out["bev_fit_alone_ms"] = pass_ms(eng, reps, eng.stage_bev_fit)
        elif key == "cluster":
            out["depth_cluster_alone_ms"] = pass_ms(eng, reps, eng.stage_cluster)
        else:
            res[key] = eng.download(full=False)
        del eng
        torch.cuda.empty_cache()
    a, b = res["plain"], res["vertical"]
    xyz = np.zeros((len(b["hit_xyz"]), 4), np.float32)
    xyz[:, :b["hit_xyz"].shape[1]] = b["hit_xyz"]
    prior = (classes or lifting.ClassTable.nuscenes()).prior_wlh
    host = boxvertical.box_vertical_host(xyz, b["hit_off"], len(xyz), a["box"], a["flags"], prior, v.q_bot, v.q_top, v.min_points, v.lo, v.hi)
    assert all(np.array_equal(b[k], host[k]) for k in ("vert_src", "vert_status"))
    assert all(b[k].tobytes() == host[k].tobytes() for k in ("vert_z", "vert_h", "vert_entry_z", "box"))
    n, st, src = np.diff(b["hit_off"]), b["vert_status"], b["vert_src"]
    out["lists"] = dict(points=int(n.sum()), longest=int(n.max()), mean=float(n.mean()), median=float(np.median(n)),
                        lane_route=int((n <= lifting._lib.VERT_LANE_MAX).sum()),
                        block_route_staged=int(((n > lifting._lib.VERT_LANE_MAX) & (n <= lifting._lib.VERT_LDS_KEYS)).sum()),
                        block_route_streamed=int((n > lifting._lib.VERT_LDS_KEYS).sum()))
    out["vert_status"] = dict(ok=int((st == 0).sum()), few_points=int((st == 1).sum()), empty=int((st == 2).sum()), non_finite=int((st == 4).sum()))
    out["vert_src"] = dict(untouched=int((src == 0).sum()), both_ends=int((src == 1).sum()), top_only=int((src == 2).sum()))
    out["vertical_over_bev_fit"] = out["box_vertical_alone_ms"] / out["bev_fit_alone_ms"]
    out["vertical_over_depth_cluster"] = out["box_vertical_alone_ms"] / out["depth_cluster_alone_ms"]
    out["pass_ratio"] = out["pass_ms_vertical"] / out["pass_ms_plain"]
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=256)
    ap.add_argument("--waymo-frames", type=int, default=32)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    # the frames first: their generation forks, which a process that holds the GPU must not do
    t0 = time.time()
    c2 = bench.make_batches_frames(syn.config("c2"), [0], args.frames, 16)[0]
    wcfg = syn.config("c4")
    import multiprocessing
    jobs = [(wcfg, i, min(2, args.waymo_frames - i)) for i in range(0, args.waymo_frames, 2)]
    with multiprocessing.get_context("fork").Pool(min(16, len(jobs))) as pool:
        wf = [f for chunk in pool.map(_waymo_frames, jobs) for f in chunk]
    out = dict(reps=args.reps, gen_s=round(time.time() - t0, 1),
               note="the synthetic lists are frustum points, not objects: the counts say how much work the launch had, nothing about real scenes")
    lanes = [syn.make_lane_table([600.0, 1600.0], 50000, seed=7, extent=260.0)]
    out["c2"] = measure(lifting.pack_frames(c2, lanes, [0] * len(c2)), None, args.reps)
    del c2
    classes = lifting.ClassTable.waymo()
    centre = np.asarray(wf[0].pose, np.float64).reshape(4, 4)[:2, 3]
    wl = [syn.make_lane_table(centre, 50000, seed=4, extent=400.0)]
    out["c4_waymo"] = measure(lifting.pack_frames(wf, wl, [0] * len(wf), classes), classes, args.reps)
    print(json.dumps(out), flush=True)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as fh:
            fh.write(json.dumps(out, indent=1) + "\n")


if __name__ == "__main__":
    main()
