#!/usr/bin/env python3
"""What the point ownership (cm3d_point_owner, LiftEngine(owner=PointOwner())) costs on one MI355X: a --frames-frame batch of the
synthetic --config shape, RLE masks, one batch at a time and --in-flight batches in flight (resident copies of the one batch).  Timed:
  pass_ms          wall time of a pass, host-synchronised around --steps passes, without the option and with it
  owner_ms         the stage between its two events (the "owner" bucket), the median over the timed passes that carry events
and counted on the host from the downloaded raw lists: listed points, points in more than one list, list positions.
usage: tools/point_owner_time.py [--config c2] [--frames 256] [--steps 100] [--in-flight 4] [--off-only] [--out profiles/point_owner_time.json]"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np  # noqa: E402

import bench  # noqa: E402
from cm3d_amd import lifting, synthetic as syn  # noqa: E402


def contested(hb, got):
    listed = shared = 0
    for f in range(hb.n_frames):
        lo, hi = int(got["hit_off"][hb.mask_off[f]]), int(got["hit_off"][hb.mask_off[f + 1]])
        _, cnt = np.unique(got["hit_idx"][lo:hi], return_counts=True)
        listed, shared = listed + len(cnt), shared + int((cnt > 1).sum())
    return listed, shared


def measure(torch, hb, depth, owner, steps, warmup):
    pipe = lifting.LiftPipeline("cuda:0", depth=depth, **({} if owner is None else {"owner": owner}))
    for slot in range(depth):
        with torch.cuda.stream(pipe.streams[slot]):
            pipe.engines[slot].upload(hb)
    torch.cuda.synchronize()
    for k in range(max(warmup, depth)):
        pipe.rerun(k % depth, masks="rle")
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for k in range(steps):
        pipe.rerun(k % depth, masks="rle")
    torch.cuda.synchronize()
    out = {"pass_ms": (time.perf_counter() - t0) * 1e3 / steps}
    if owner is not None:                              # passes with events, all slots busy: the stage's own pair
        evs = [[] for _ in range(steps)]
        for k in range(steps):
            pipe.rerun(k % depth, masks="rle", stage_events=evs[k])
        torch.cuda.synchronize()
        at = 5 + 2 * list(pipe.engines[0].b.timed).index("owner")
        ms = sorted(e[at].elapsed_time(e[at + 1]) for e in evs)
        out.update(owner_ms=ms[len(ms) // 2], owner_ms_min=ms[0], owner_ms_max=ms[-1])
        got = pipe.engines[0].download(full=True)
        listed, shared = contested(hb, got)
        out.update(listed_points=listed, contested_points=shared, list_positions=int(got["hit_off"][-1]),
                   positions_lost=int(got["ow_lost"].sum()), masks=int(hb.n_masks), ow_status=np.bincount(got["ow_status"], minlength=3).tolist(),
                   workspace_mb=pipe.engines[0].b.ow_ws_bytes / 1e6)
    del pipe
    torch.cuda.synchronize()
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--config", default="c2")
    ap.add_argument("--frames", type=int, default=256)
    ap.add_argument("--steps", type=int, default=100)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--in-flight", type=int, default=4)
    ap.add_argument("--off-only", action="store_true", help="only the passes without the option (a build that does not have it)")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    cfg = syn.config(args.config)
    frames = bench.make_batches_frames(cfg, [0], args.frames, 16)[0]              # (before anything initialises the GPU: it forks)
    lanes = [syn.make_lane_table([600.0, 1600.0], 50000, seed=7, extent=260.0)]
    hb = lifting.pack_frames(frames, lanes, [0] * args.frames)
    import torch
    if not args.off_only:
        from cm3d_amd import pointowner
    res = {"config": args.config, "frames": args.frames, "steps": args.steps}
    for depth in (1, args.in_flight):
        for name, owner in (("off", None),) + (() if args.off_only else (("on", pointowner.PointOwner()),)):
            res[f"in_flight_{depth}_{name}"] = measure(torch, hb, depth, owner, args.steps, args.warmup)
    text = json.dumps(res, indent=1)
    print(text)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        open(args.out, "w").write(text + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
