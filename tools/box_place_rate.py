#!/usr/bin/env python3
"""Runs ON THE GPU BOX: what the opt-in box placement costs (cm3d_box_place, behind the yaw-fitted pass), on the C2-shaped batch bench.py
times and on a Waymo-shaped batch of C4 frames.  Per shape, with HIP events and the median of --reps:
  * one pass over the resident batch with the yaw fit alone and with the placement behind it;
  * cm3d_box_place alone on the resident rows, and cm3d_box_nms_bounded alone in the same run -- the launch of the same shape, one wave
    per frame with the same NMS -- and their ratio;
  * inside the placed pass: the span between the placement's two events;
  * how many masks take each place_src value, how far the placed centres moved, and how many verdicts of the circle NMS changed.
usage: tools/box_place_rate.py [--frames 256] [--waymo-frames 32] [--reps 20] [--thin 0.5] [--out FILE.json]"""
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
from cm3d_amd import bevfit, boxplace, lifting, synthetic as syn  # noqa: E402
from tools.bev_fit_rate import _waymo_frames, span_ms  # noqa: E402
from tools.kitti_obb_rate import pass_ms  # noqa: E402


def measure(hb, classes, yaw, place, reps):
    out = dict(frames=int(hb.n_frames), masks=int(hb.n_masks), most_masks_in_a_frame=int(np.diff(hb.mask_off).max()))
    res = {}
    for key, p in (("fitted", None), ("placed", place)):
        eng = lifting.LiftEngine("cuda:0", classes=classes, yaw=yaw, place=p)
        eng.upload(hb)
        for _ in range(3):
            eng.run(masks="rle")
        torch.cuda.synchronize()
        out[f"pass_ms_{key}"] = pass_ms(eng, reps)
        if p is not None:
            out["place_span_in_pass_ms"] = span_ms(eng, reps)                 # the placement's events are the last two
            res[key] = eng.download(full=False)                               # (before the launches alone rewrite box and flags)
            out["box_place_alone_ms"] = pass_ms(eng, reps, eng.stage_place)
            out["box_nms_alone_ms"] = pass_ms(eng, reps, eng.stage_boxes)
            out["place_over_box_launch"] = out["box_place_alone_ms"] / out["box_nms_alone_ms"]
        else:
            res[key] = eng.download(full=False)
        del eng
        torch.cuda.empty_cache()
    a, b = res["fitted"], res["placed"]
    for key in ("hit_off", "medoid_pos", "lane_idx", "fit_rect", "yaw_src"):
        assert np.array_equal(a[key], b[key]), key
    src = b["place_src"]
    off = src == 0
    assert a["box"][off, :9].tobytes() == b["box"][off, :9].tobytes() and a["box"][:, 2:9].tobytes() == b["box"][:, 2:9].tobytes()
    assert b["place_pushed"].tobytes() == a["box"][:, :2].tobytes()
    moved = np.hypot(*(b["box"][~off, :2] - a["box"][~off, :2]).T) if (~off).any() else np.zeros(1)
    out["place_src"] = dict(not_placed=int(off.sum()), corner=int((src == 1).sum()), one_axis=int((src == 2).sum()), face_centre=int((src == 3).sum()))
    out["moved_m"] = dict(median=float(np.median(moved)), max=float(moved.max()))
    out["verdicts_changed"] = int((a["flags"] != b["flags"]).sum())
    out["kept"] = dict(fitted=int(((a["flags"] & 3) == 3).sum()), placed=int(((b["flags"] & 3) == 3).sum()))
    out["pass_ratio"] = out["pass_ms_placed"] / out["pass_ms_fitted"]
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=256)
    ap.add_argument("--waymo-frames", type=int, default=32)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--thin", type=float, default=0.5)
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
    yaw, place = bevfit.YawFit(), boxplace.BoxPlace(args.thin)
    out = dict(thin=place.thin, angles=yaw.angles, reps=args.reps, gen_s=gen_s)
    lanes = [syn.make_lane_table([600.0, 1600.0], 50000, seed=7, extent=260.0)]
    out["c2"] = measure(lifting.pack_frames(c2, lanes, [0] * len(c2)), None, yaw, place, args.reps)
    del c2
    classes = lifting.ClassTable.waymo()
    centre = np.asarray(wf[0].pose, np.float64).reshape(4, 4)[:2, 3]
    wl = [syn.make_lane_table(centre, 50000, seed=4, extent=400.0)]
    out["c4_waymo"] = measure(lifting.pack_frames(wf, wl, [0] * len(wf), classes), classes, yaw, place, args.reps)
    print(json.dumps(out), flush=True)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as fh:
            fh.write(json.dumps(out, indent=1) + "\n")


if __name__ == "__main__":
    main()
