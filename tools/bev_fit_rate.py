#!/usr/bin/env python3
"""Runs ON THE GPU BOX: what the opt-in yaw fit costs (cm3d_bev_fit, cm3d_yaw_select and the box launch again, behind the pass), on the
C2-shaped batch bench.py times and on a Waymo-shaped batch of C4 frames.  Per shape, with HIP events and the median of --reps:
  * one pass over the resident batch without and with the fit (the defaults of bevfit.YawFit unless flags say otherwise);
  * the fit's three launches alone on the resident lists, and cm3d_bev_fit alone;
  * inside the fitted pass: the span between the fit's two events (cm3d_bev_fit + cm3d_yaw_select);
  * the lists: how many are fitted, too short, empty, how many masks take the fit, and the longest list -- one workgroup walks a list
    from end to end, so the longest list sets the tail of the launch.
usage: tools/bev_fit_rate.py [--frames 256] [--waymo-frames 32] [--reps 20] [--angles 128] [--out FILE.json]"""
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
from cm3d_amd import bevfit, lifting, synthetic as syn  # noqa: E402
from tools.kitti_obb_rate import pass_ms  # noqa: E402


def _waymo_frames(job):
    cfg, first, n = job
    return [syn.make_waymo_frame(cfg, first + i) for i in range(n)]


def span_ms(eng, reps):
    """Median over `reps` fitted passes of the time between the fit's two events, in ms."""
    runs = []
    for _ in range(reps):
        ev = []
        eng.run(masks="rle", stage_events=ev)
        runs.append(ev)
    torch.cuda.synchronize()
    return float(np.median([ev[-2].elapsed_time(ev[-1]) for ev in runs]))


def measure(hb, classes, yaw, reps):
    out = dict(frames=int(hb.n_frames), masks=int(hb.n_masks))
    res = {}
    for key, y in (("plain", None), ("fitted", yaw)):
        eng = lifting.LiftEngine("cuda:0", classes=classes, yaw=y)
        eng.upload(hb)
        for _ in range(3):
            eng.run(masks="rle")
        torch.cuda.synchronize()
        out[f"pass_ms_{key}"] = pass_ms(eng, reps)
        if y is not None:
            out["three_launches_ms"] = pass_ms(eng, reps, eng.stage_yaw_fit)
            out["bev_fit_alone_ms"] = pass_ms(eng, reps, eng.stage_bev_fit)
            out["fit_span_in_pass_ms"] = span_ms(eng, reps)
        res[key] = eng.download(full=False)
        del eng
        torch.cuda.empty_cache()
    a, b = res["plain"], res["fitted"]
    for key in ("hit_off", "medoid_pos", "lane_idx"):
        assert np.array_equal(a[key], b[key]), key
    lane = b["yaw_src"] == 0
    assert a["box"][lane, :9].tobytes() == b["box"][lane, :9].tobytes()
    n, st = np.diff(a["hit_off"]), b["fit_status"]
    out["lists"] = dict(fitted=int((st == 0).sum()), few_points=int((st == 1).sum()), empty=int((st == 2).sum()), short=int((st == 3).sum()),
                        non_finite=int((st == 4).sum()), take_the_fit=int((~lane).sum()), longest=int(n.max()), mean=float(n.mean()),
                        points=int(n.sum()))
    out["pass_ratio"] = out["pass_ms_fitted"] / out["pass_ms_plain"]
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=256)
    ap.add_argument("--waymo-frames", type=int, default=32)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--angles", type=int, default=128)
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
    gen_s = round(time.time() - t0, 1)
    yaw = bevfit.YawFit(angles=args.angles)
    out = dict(angles=yaw.angles, min_points=yaw.min_points, min_length=yaw.min_length, d0=yaw.d0, reps=args.reps, gen_s=gen_s,
               chunk=lifting._lib.BEV_FIT_CHUNK)
    lanes = [syn.make_lane_table([600.0, 1600.0], 50000, seed=7, extent=260.0)]
    out["c2"] = measure(lifting.pack_frames(c2, lanes, [0] * len(c2)), None, yaw, args.reps)
    del c2
    classes = lifting.ClassTable.waymo()
    centre = np.asarray(wf[0].pose, np.float64).reshape(4, 4)[:2, 3]
    wl = [syn.make_lane_table(centre, 50000, seed=4, extent=400.0)]
    out["c4_waymo"] = measure(lifting.pack_frames(wf, wl, [0] * len(wf), classes), classes, yaw, args.reps)
    print(json.dumps(out), flush=True)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as fh:
            fh.write(json.dumps(out, indent=1) + "\n")


if __name__ == "__main__":
    main()
