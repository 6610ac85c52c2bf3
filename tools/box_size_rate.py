#!/usr/bin/env python3
"""Runs ON THE GPU BOX: what the opt-in box size stage costs (cm3d_box_size: one call of four launches behind cm3d_box_tracks), with HIP
events and the median of --reps.  Two batches:

1. the C2-shaped batch bench.py times (256 frames x 20 masks), chained as scenes of --scene-frames keyframes 0.5 s apart as
   tools/box_velocity_rate.py does.  The synthetic frames are drawn independently of each other and their lists are frustum points, not
   vehicles: few boxes find a partner, nearly every track has one member, and what the stage pools and moves says nothing about real
   scenes.  The times are a LOWER bound of the call's on real scenes;
2. the moving-scene batch of the tests (tests/box_size_pass_cases.py: two scenes of three keyframes, a car of two faces in every frame).

Per batch: cm3d_box_size alone and cm3d_box_tracks alone in the same run -- the comparable stage: the same shape, a link walk per mask --
and their ratio; one pass over the resident batch with YawFit() + BoxPlace() + Velocity() and with BoxSize() behind them; how many
dimensions were pooled; how far centres and velocities moved.  Every timed configuration is first held against the host statement.
usage: tools/box_size_rate.py [--frames 256] [--scene-frames 16] [--reps 20] [--out FILE.json]"""
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
from cm3d_amd import bevfit, boxplace, boxsize, lifting, synthetic as syn, tracks  # noqa: E402
from tools.box_velocity_rate import chained  # noqa: E402
from tools.kitti_obb_rate import pass_ms  # noqa: E402


def measure(hb, classes, velocity, reps):
    out = dict(frames=int(hb.n_frames), masks=int(hb.n_masks), links=int((np.asarray(hb.frame_next) >= 0).sum()))
    kw = dict(classes=classes, yaw=bevfit.YawFit(), place=boxplace.BoxPlace(), velocity=velocity)
    place = kw["place"]
    res = {}
    for key, size in (("placed", None), ("sized", boxsize.BoxSize())):
        eng = lifting.LiftEngine("cuda:0", size=size, **kw)
        eng.upload(hb)
        for _ in range(3):
            eng.run(masks="rle")
        torch.cuda.synchronize()
        res[key] = eng.download(full=False)
        out[f"pass_ms_{key}"] = pass_ms(eng, reps)
        if size is not None:
            # (both calls rewrite only what a repetition writes again: the same work every time)
            out["box_size_alone_ms"] = pass_ms(eng, reps, eng.stage_size)
            out["box_tracks_alone_ms"] = pass_ms(eng, reps, eng.stage_tracks)
            out["size_over_tracks"] = out["box_size_alone_ms"] / out["box_tracks_alone_ms"]
        del eng
        torch.cuda.empty_cache()
    a, b = res["placed"], res["sized"]
    tr = tracks.box_tracks_host(a["box"], a["flags"], hb.mask_frame, a["next_match"], a["prev_match"], hb.frame_time)
    s = boxsize.BoxSize()
    host = boxsize.box_size_host(a["box"], a["flags"], hb.mask_frame, a["fit_rect"], a["place_src"], classes.prior_wlh, hb.ego_xyz, a["next_match"],
                                 a["prev_match"], tr["track_id"], tr["track_pos"], tr["track_len"], hb.frame_time, thin=place.thin,
                                 max_dt=velocity.max_dt, q=s.q, min_obs=s.min_obs, lo=s.lo, hi=s.hi)
    assert host["status"] == 0 and all(np.array_equal(b[k], host[k]) for k in ("size_src", "size_obs", "flags"))
    assert all(b[k].tobytes() == host[k].tobytes() for k in ("size_wlh", "size_ratio", "size_placed", "size_vel", "box"))
    kept = (b["flags"] & 3) == 3
    src = b["size_src"]
    moved = np.hypot(*(b["box"][:, :2] - a["box"][:, :2]).T)
    dv = np.hypot(*(b["size_vel"] - a["vel"]).T)
    on = src > 0
    out.update(kept=int(kept.sum()), tracks=int((b["track_pos"] == 0).sum()), longest_track=int(b["track_len"].max()),
               placed=int((a["place_src"] > 0).sum()), boxes_with_a_pooled_dimension=int(on.sum()),
               pooled=dict(length=int((src & 1).astype(bool).sum()), width=int((src & 2).astype(bool).sum())),
               centre_moved_m=dict(median=float(np.median(moved[on])) if on.any() else 0.0, max=float(moved.max())),
               velocity_moved_mps=dict(median=float(np.median(dv[on])) if on.any() else 0.0, max=float(dv.max())),
               pass_ratio=out["pass_ms_sized"] / out["pass_ms_placed"])
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=256)
    ap.add_argument("--scene-frames", type=int, default=16)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    # the frames first: their generation forks, which a process that holds the GPU must not do
    t0 = time.time()
    c2 = bench.make_batches_frames(syn.config("c2"), [0], args.frames, 16)[0]
    from tests import box_size_pass_cases as sp, velocity_pass_cases as pc
    moving = sp.batch()
    out = dict(reps=args.reps, scene_frames=args.scene_frames, gen_s=round(time.time() - t0, 1),
               note="the synthetic lists are frustum points, not vehicles: what is pooled and how far centres and velocities move says nothing about real scenes")
    lanes = [syn.make_lane_table([600.0, 1600.0], 50000, seed=7, extent=260.0)]
    out["c2"] = measure(chained(c2, lanes, args.scene_frames), lifting.ClassTable.nuscenes(), lifting.Velocity(), args.reps)
    del c2
    out["moving_scenes"] = measure(moving.hb, moving.classes, pc.settings()[0], args.reps)
    print(json.dumps(out), flush=True)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as fh:
            fh.write(json.dumps(out, indent=1) + "\n")


if __name__ == "__main__":
    main()
