#!/usr/bin/env python3
"""Runs ON THE GPU BOX: what the opt-in box velocity stage costs (cm3d_box_velocity: one call of eight launches behind the pass), with
HIP events and the median of --reps, on the C2-shaped batch bench.py times (256 frames x 20 masks) and on a C5-shaped one (80 masks
per frame; one sweep per frame instead of ten and --c5-frames frames: the stage sees boxes, not sweeps): the stage alone, and one
pass over the resident batch without and with it.  The frames of a batch are chained as scenes of --scene-frames keyframes 0.5 s
apart.  The synthetic frames are drawn independently of each other, so few boxes find a partner: every weight is computed
and every link solved all the same, but with nearly all weights 0 a row's search ends at the first free column -- real scenes, where most
boxes have a partner and some have several candidates, give k_track_assign more steps than this measures.
usage: tools/box_velocity_rate.py [--frames 256] [--c5-frames 64] [--scene-frames 16] [--reps 20] [--out FILE.json]"""
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
from cm3d_amd import lifting, synthetic as syn, velocity  # noqa: E402
from tools.kitti_obb_rate import pass_ms  # noqa: E402


def chained(frames, lanes, scene_frames):
    n = len(frames)
    k = np.arange(n)
    nxt = np.where(((k + 1) % scene_frames != 0) & (k + 1 < n), k + 1, -1).astype(np.int32)
    return lifting.pack_frames(frames, lanes, [0] * n, frame_next=nxt, frame_time=0.5 * (k % scene_frames))


def measure(hb, reps):
    out = dict(frames=int(hb.n_frames), masks=int(hb.n_masks), masks_per_frame=int(np.diff(hb.mask_off).max()),
               links=int((hb.frame_next >= 0).sum()))
    plain = lifting.LiftEngine("cuda:0")
    plain.upload(hb)
    for _ in range(3):
        plain.run(masks="rle")
    torch.cuda.synchronize()
    out["pass_ms_plain"] = pass_ms(plain, reps)
    base = plain.download(full=False)
    out["kept"] = int((base["flags"] == 3).sum())
    del plain
    eng = lifting.LiftEngine("cuda:0", velocity=lifting.Velocity())
    eng.upload(hb)
    for _ in range(3):
        eng.run(masks="rle")
    torch.cuda.synchronize()
    out["pairs"] = int(eng.b.vel_pairs)
    out["pass_ms_velocity"] = pass_ms(eng, reps)
    out["stage_ms"] = pass_ms(eng, reps, eng.stage_velocity)
    res = eng.download(full=False)
    assert np.array_equal(res["box"], base["box"], equal_nan=True) and np.array_equal(res["flags"], base["flags"])
    host = velocity.track_velocity_host(res["box"], res["flags"], hb.mask_off, hb.class_id, hb.frame_next, hb.frame_time,
                                        eng.classes.nms_group, eng.velocity.speed_by_group(eng.classes), eng.velocity.max_dt)
    assert all(np.array_equal(res[k], host[k]) for k in ("next_match", "prev_match", "vel_src")) and res["vel"].tobytes() == host["vel"].tobytes()
    out["matched"] = int((res["next_match"] >= 0).sum())
    out["pass_ratio"] = out["pass_ms_velocity"] / out["pass_ms_plain"]
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=256)
    ap.add_argument("--c5-frames", type=int, default=64)
    ap.add_argument("--scene-frames", type=int, default=16)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    # the frames first: their generation forks, which a process that holds the GPU must not do
    t0 = time.time()
    c2 = bench.make_batches_frames(syn.config("c2"), [0], args.frames, 16)[0]
    c5 = bench.make_batches_frames(syn.config("c5", n_sweeps=1), [0], args.c5_frames, 16)[0]
    out = dict(reps=args.reps, scene_frames=args.scene_frames, gen_s=round(time.time() - t0, 1))
    lanes = [syn.make_lane_table([600.0, 1600.0], 50000, seed=7, extent=260.0)]
    out["c2"] = measure(chained(c2, lanes, args.scene_frames), args.reps)
    del c2
    out["c5_shape"] = measure(chained(c5, lanes, args.scene_frames), args.reps)
    del c5
    print(json.dumps(out), flush=True)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as fh:
            fh.write(json.dumps(out, indent=1) + "\n")


if __name__ == "__main__":
    main()
