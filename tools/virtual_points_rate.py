#!/usr/bin/env python3
"""Runs ON THE GPU BOX: what the opt-in virtual points cost (cm3d_hit_project: one launch, a thread per list position;
cm3d_virtual_points: one launch, a workgroup per mask), with HIP events and the median of --reps, on the C2-shaped batch bench.py times
(256 frames x 20 masks).  In one run:

  * one pass over the resident batch without the option and with it, and the span of the stage's two events inside the pass;
  * each of the two launches alone, on what a pass left resident;
  * the same for every mask (kept_only off) and for 1024 points per mask, the most a call takes;
  * the counts of vp_status and the points written.

The timed default configuration is first held against the host statement on a sample of the masks.  The synthetic frames are rings on
a flat ground with cylinders: the counts say how much work the launches had, nothing about real scenes.  Run it as one step under a time
limit of its own, like the other rate tools: timeout -k 10 600 python tools/virtual_points_rate.py --out profiles/virtual_points_rate.json
usage: tools/virtual_points_rate.py [--frames 256] [--reps 20] [--check-masks 64] [--out FILE.json]"""
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
from cm3d_amd import lifting, synthetic as syn, virtualpoints as vp  # noqa: E402
from cm3d_amd._lib import check  # noqa: E402
from tools.kitti_obb_rate import pass_ms  # noqa: E402


def stage_span_ms(eng, reps):
    """Median over `reps` passes of the time between the stage's two events (the last pair), in ms."""
    runs = []
    for _ in range(reps):
        ev = []
        eng.run(masks="rle", stage_events=ev)
        runs.append(ev)
    torch.cuda.synchronize()
    return float(np.median([ev[-2].elapsed_time(ev[-1]) for ev in runs]))


def project_alone(eng):
    b, p = eng.b, lifting._ptr

    def call(st):
        xyz, off = eng.read_lists()
        check(eng.lib.cm3d_hit_project(p(xyz), p(off), p(b.mask_frame), p(b.mask_cam), p(b.cams), b.hb.n_cams, b.F, b.M, b.idx_cap, p(b.hit_uvd), st),
              "cm3d_hit_project")
    return call


def points_alone(eng):
    b, v, p = eng.b, eng.virtual, lifting._ptr

    def call(st):
        check(eng.lib.cm3d_virtual_points(p(b.packed), p(b.bbox), b.W, b.H, p(b.cams), b.hb.n_cams, p(b.mask_off), p(b.mask_frame), p(b.mask_cam),
                                          p(b.flags), b.F, b.M, p(b.hit_uvd), p(eng.read_lists()[1]), b.idx_cap, v.per_mask, v.seed, v.max_px,
                                          int(v.kept_only), p(b.frame_seed), p(b.vp_count), p(b.vp_status), p(b.vp_xyz), p(b.vp_pix), p(b.vp_src),
                                          p(b.vp_depth), p(b.vp_d2), st), "cm3d_virtual_points")
    return call


def held_against_the_host(eng, got, n_masks):
    """The first n_masks masks of the resident batch against virtualpoints.virtual_points_host; returns the points compared."""
    b, v = eng.b, eng.virtual
    hb = b.hb
    m1 = min(int(n_masks), b.M)
    f1 = int(hb.mask_frame[m1 - 1]) + 1
    m1 = int(hb.mask_off[f1])                              # whole frames
    cams = np.asarray(hb.cams, np.float32).reshape(b.F, hb.n_cams, -1)
    exp = vp.virtual_points_host(b.packed[:m1].cpu().numpy(), b.bbox[:m1].cpu().numpy(), b.W, b.H, cams[:f1], hb.mask_off[:f1 + 1], hb.mask_frame[:m1],
                                 hb.mask_cam[:m1], got["flags"][:m1], got["hit_uvd"], got["hit_off"][:m1 + 1], len(got["hit_uvd"]), v.per_mask, v.seed,
                                 v.max_px, v.kept_only, None)
    K = v.per_mask
    assert np.array_equal(got["vp_count"][:m1], exp["vp_count"]) and np.array_equal(got["vp_status"][:m1], exp["vp_status"])
    for m in range(m1):
        rows = slice(m * K, m * K + int(exp["vp_count"][m]))
        for k in ("vp_xyz", "vp_pix", "vp_src", "vp_depth", "vp_d2"):
            assert got[k][rows].tobytes() == exp[k][rows].tobytes(), (k, m)
    return int(exp["vp_count"].sum())


def measure(hb, reps, check_masks):
    out = dict(frames=int(hb.n_frames), masks=int(hb.n_masks), rows=int(hb.n_raw_rows))
    configs = (("plain", None), ("default", vp.VirtualPoints()), ("all_masks", vp.VirtualPoints(kept_only=False)),
               ("k1024", vp.VirtualPoints(per_mask=1024)))
    for key, v in configs:
        eng = lifting.LiftEngine("cuda:0", virtual=v)
        eng.upload(hb)
        for _ in range(3):
            eng.run(masks="rle")
        torch.cuda.synchronize()
        out[f"pass_ms_{key}"] = pass_ms(eng, reps)
        if v is not None:
            out[f"stage_span_in_pass_ms_{key}"] = stage_span_ms(eng, reps)
            out[f"hit_project_alone_ms_{key}"] = pass_ms(eng, reps, project_alone(eng))
            out[f"virtual_points_alone_ms_{key}"] = pass_ms(eng, reps, points_alone(eng))
            got = eng.download(full=key == "default")
            st = got["vp_status"]
            out[f"vp_status_{key}"] = dict(ok=int((st == 0).sum()), not_kept=int((st == 1).sum()), empty=int((st == 2).sum()), camera=int((st == 4).sum()))
            out[f"points_{key}"] = int(got["vp_count"].sum())
            if key == "default":
                out["list_positions"] = int(got["hit_off"][-1])
                out["points_held_against_the_host"] = held_against_the_host(eng, got, check_masks)
        del eng
        torch.cuda.empty_cache()
    out["pass_ratio_default"] = out["pass_ms_default"] / out["pass_ms_plain"]
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=256)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--check-masks", type=int, default=64)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    # the frames first: their generation forks, which a process that holds the GPU must not do
    t0 = time.time()
    c2 = bench.make_batches_frames(syn.config("c2"), [0], args.frames, 16)[0]
    out = dict(reps=args.reps, gen_s=round(time.time() - t0, 1),
               note="the synthetic frames are rings on a flat ground with cylinders: the counts say how much work the launches had, nothing "
                    "about real scenes; the defaults of VirtualPoints() are untuned")
    lanes = [syn.make_lane_table([600.0, 1600.0], 50000, seed=7, extent=260.0)]
    out["c2"] = measure(lifting.pack_frames(c2, lanes, [0] * len(c2)), args.reps, args.check_masks)
    print(json.dumps(out), flush=True)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as fh:
            fh.write(json.dumps(out, indent=1) + "\n")


if __name__ == "__main__":
    main()
