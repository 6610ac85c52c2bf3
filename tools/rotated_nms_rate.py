#!/usr/bin/env python3
"""Runs ON THE GPU BOX: what the opt-in rotated-box NMS costs (cm3d_box_rotated_nms: one launch behind the box launch of a pass),
with HIP events and the median of --reps:
  * on the C2-shaped batch bench.py times (256 frames x 20 masks) and on a C5-shaped one (80 masks per frame; one sweep per frame
    instead of ten and --c5-frames frames: the launch sees masks and boxes, not sweeps): the launch alone for both measures, beside
    the box launch (k_box_nms, which also assembles the boxes) on the same batch, and one pass over the resident batch without and
    with the NMS;
  * on one frame of 1024 boxes (a crowd: six in ten are second detections of an earlier box): cm3d_rotated_nms beside
    cm3d_circle_nms on the same centres.
usage: tools/rotated_nms_rate.py [--frames 256] [--c5-frames 64] [--reps 20] [--out FILE.json]"""
import argparse
import json
import math
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np  # noqa: E402
import torch  # noqa: E402

import bench  # noqa: E402  (make_batches_frames: the frames of a batch in forked processes)
from cm3d_amd import lifting, nms, ops, synthetic as syn  # noqa: E402
from tools.kitti_obb_rate import pass_ms  # noqa: E402


def measure(hb, reps):
    out = dict(frames=int(hb.n_frames), masks=int(hb.n_masks), masks_per_frame=int(np.diff(hb.mask_off).max()))
    plain = lifting.LiftEngine("cuda:0")
    plain.upload(hb)
    for _ in range(3):
        plain.run(masks="rle")
    torch.cuda.synchronize()
    out["pass_ms_plain"] = pass_ms(plain, reps)
    out["box_launch_ms"] = pass_ms(plain, reps, plain.stage_boxes)
    base = plain.download(full=False)
    out["boxes"] = int((base["flags"] & 1).sum())
    out["kept_circle"] = int((base["flags"] == 3).sum())
    del plain
    for measure_ in nms.MEASURES:
        eng = lifting.LiftEngine("cuda:0", nms=lifting.RotatedNms(measure_))
        eng.upload(hb)
        for _ in range(3):
            eng.run(masks="rle")
        torch.cuda.synchronize()
        out[f"pass_ms_{measure_}"] = pass_ms(eng, reps)
        out[f"rotated_launch_ms_{measure_}"] = pass_ms(eng, reps, eng.stage_rotated_nms)
        res = eng.download(full=False)
        assert np.array_equal(res["box"][:, :9], base["box"][:, :9])
        out[f"kept_{measure_}"] = int((res["flags"] == 3).sum())
        del eng
        torch.cuda.empty_cache()
    out["pass_ratio_iou"] = out["pass_ms_iou"] / out["pass_ms_plain"]
    return out


def crowd(n, rng):
    """n boxes around (600, 1600): random sizes and headings, six in ten a second or third detection of an earlier one."""
    rec = np.zeros((n, 6))
    free = []
    side = 10.0 * math.sqrt(n)
    for k in range(n):
        if free and rng.random() < 0.6:
            r = rec[free.pop(int(rng.integers(0, len(free))))]
            h = math.atan2(r[5], r[4]) + rng.normal(scale=0.1)
            rec[k] = [r[0] + rng.normal(scale=0.06 * r[2]), r[1] + rng.normal(scale=0.06 * r[2]), r[2] * rng.uniform(0.9, 1.1),
                      r[3] * rng.uniform(0.9, 1.1), math.cos(h), math.sin(h)]
        else:
            h = rng.uniform(-math.pi, math.pi)
            rec[k] = [600.0 + rng.uniform(0, side), 1600.0 + rng.uniform(0, side), rng.uniform(1.0, 6.0), rng.uniform(0.5, 2.5), math.cos(h), math.sin(h)]
            free += [k, k]
    return rec, 0.05 + 0.9 * (rng.permutation(n) + 0.5) / n


def one_frame(n, reps):
    rec, score = crowd(n, np.random.default_rng(1024))
    out = dict(boxes=n)
    for measure_ in nms.MEASURES:
        keep = ops.rotated_nms(rec, score, np.zeros(n, np.int32), [0, n], 0.4, measure_)
        assert np.array_equal(keep, nms.rotated_nms_host(rec, score, np.zeros(n, np.int32), [0, n], [0.4], measure_))
        out[f"kept_{measure_}"] = int(keep.sum())
    L = lifting._lib.lib()
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda()
    d_rec, d_sc, d_grp, d_off, d_thr = t(rec), t(score), t(np.zeros(n, np.int32)), t(np.array([0, n], np.int32)), t(np.array([0.4]))
    d_x, d_y, d_thr2 = t(rec[:, 0].copy()), t(rec[:, 1].copy()), t(np.array([4.0]))
    keep = torch.zeros(n, dtype=torch.int32, device="cuda")

    class Direct:           # pass_ms's stage(st) interface
        @staticmethod
        def iou(st):
            L.cm3d_rotated_nms(d_rec.data_ptr(), d_sc.data_ptr(), d_grp.data_ptr(), d_off.data_ptr(), 1, d_thr.data_ptr(), 1, 0, 0, keep.data_ptr(), st)

        @staticmethod
        def cover(st):
            L.cm3d_rotated_nms(d_rec.data_ptr(), d_sc.data_ptr(), d_grp.data_ptr(), d_off.data_ptr(), 1, d_thr.data_ptr(), 1, 1, 0, keep.data_ptr(), st)

        @staticmethod
        def circle(st):
            L.cm3d_circle_nms(d_x.data_ptr(), d_y.data_ptr(), d_sc.data_ptr(), d_grp.data_ptr(), d_off.data_ptr(), 1, d_thr2.data_ptr(), 1, keep.data_ptr(), st)
    for name in ("iou", "cover", "circle"):
        fn = getattr(Direct, name)
        for _ in range(3):
            fn(torch.cuda.current_stream().cuda_stream)
        torch.cuda.synchronize()
        out[f"{'rotated' if name != 'circle' else 'circle'}_launch_ms{'_' + name if name != 'circle' else ''}"] = pass_ms(None, reps, fn)
    out["kept_circle"] = int(keep.sum().item())
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=256)
    ap.add_argument("--c5-frames", type=int, default=64)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    # the frames first: their generation forks, which a process that holds the GPU must not do
    t0 = time.time()
    c2 = bench.make_batches_frames(syn.config("c2"), [0], args.frames, 16)[0]
    c5 = bench.make_batches_frames(syn.config("c5", n_sweeps=1), [0], args.c5_frames, 16)[0]
    out = dict(reps=args.reps, thr=nms.DEFAULT_THR, gen_s=round(time.time() - t0, 1))
    lanes = [syn.make_lane_table([600.0, 1600.0], 50000, seed=7, extent=260.0)]
    out["c2"] = measure(lifting.pack_frames(c2, lanes, [0] * len(c2)), args.reps)
    del c2
    out["c5_shape"] = measure(lifting.pack_frames(c5, lanes, [0] * len(c5)), args.reps)
    del c5
    out["one_frame_1024"] = one_frame(1024, args.reps)
    print(json.dumps(out), flush=True)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as fh:
            fh.write(json.dumps(out, indent=1) + "\n")


if __name__ == "__main__":
    main()
