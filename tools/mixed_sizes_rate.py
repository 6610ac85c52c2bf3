#!/usr/bin/env python3
"""Runs ON THE GPU BOX: what the mask stage costs when a batch holds masks of two image sizes (Waymo: FRONT* 1920x1280, SIDE*
1920x886; src/waymo/2d_to_3d.py:520-521), on a Waymo-shaped synthetic batch -- the C4 shape, the masks of cameras 3 and 4 cropped
to 1920x886 -- three ways (HIP events around the mask launch alone, median of --reps):
  * sized     cm3d_rle_erode_pack_sized on the producer's run lists and a table of sizes: what the product does;
  * embedded  the only way to the same result without it: every run list re-encoded for the canvas width on the host
              (tests/mixed_size_cases.embed_runs), then cm3d_rle_erode_pack; the host time of the re-encode and the bytes the longer
              lists add to the upload are reported on their own;
  * uncropped the same frames with every mask at 1920x1280 through cm3d_rle_erode_pack (more pixels to paint).
The sized and the embedded results are compared bit for bit (bbox and every stored word) before anything is timed.
usage: tools/mixed_sizes_rate.py [--frames 64] [--points 20000] [--reps 50] [--out FILE.json]
(the mask stage does not read the points; --points only sizes the rest of the batch)"""
import argparse
import dataclasses
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np  # noqa: E402
import torch  # noqa: E402

from cm3d_amd import lifting, synthetic as syn  # noqa: E402
from tests import mixed_size_cases as X  # noqa: E402

SIDE = (1920, 886)


def mask_stage_ms(eng, reps):
    """Median and extremes of `reps` mask launches on the resident batch, in ms (the launch alone, between two events)."""
    st = torch.cuda.current_stream().cuda_stream
    for _ in range(5):
        eng.stage_masks(st, "rle")
    torch.cuda.synchronize()
    ev = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        eng.stage_masks(st, "rle")
        b.record()
        ev.append((a, b))
    torch.cuda.synchronize()
    t = np.array([a.elapsed_time(b) for a, b in ev])
    return {"median_ms": round(float(np.median(t)), 4), "min_ms": round(float(t.min()), 4), "max_ms": round(float(t.max()), 4), "reps": reps}


def stored(eng):
    b = eng.b
    return b.bbox.cpu().numpy(), b.packed.cpu().numpy()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=64)
    ap.add_argument("--points", type=int, default=20000)
    ap.add_argument("--reps", type=int, default=50)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    cfg = syn.config("c4", n_points=args.points)
    t0 = time.time()
    full = [syn.make_frame(cfg, i) for i in range(args.frames)]
    mixed = [X.crop_frame(f, {3: SIDE, 4: SIDE}) for f in full]
    lanes = [syn.make_lane_table(full[0].ego_xyz[:2], 2000, seed=1)]
    fl = [0] * args.frames
    hb_full = lifting.pack_frames(full, lanes, fl)
    hb_mixed = lifting.pack_frames(mixed, lanes, fl)
    assert hb_full.mask_wh is None and hb_mixed.mask_wh is not None and (hb_mixed.width, hb_mixed.height) == (cfg.width, cfg.height)
    W, H = hb_mixed.width, hb_mixed.height
    # the host re-encode the sized kernels avoid: only the masks smaller than the canvas need it
    lists = [hb_mixed.rle_counts[hb_mixed.rle_off[i]:hb_mixed.rle_off[i + 1]] for i in range(hb_mixed.n_masks)]
    small = np.flatnonzero((hb_mixed.mask_wh != (W, H)).any(axis=1))
    best = None
    for _ in range(3):
        t1 = time.perf_counter()
        emb = list(lists)
        for i in small:
            emb[i] = X.embed_runs(lists[i], int(hb_mixed.mask_wh[i, 0]), int(hb_mixed.mask_wh[i, 1]), W, H)
        dt = time.perf_counter() - t1
        best = dt if best is None else min(best, dt)
    emb_counts = np.concatenate(emb).astype(np.uint32)
    emb_off = np.concatenate([[0], np.cumsum([c.size for c in emb])]).astype(np.int32)
    hb_emb = dataclasses.replace(hb_mixed, rle_counts=emb_counts, rle_off=emb_off, mask_wh=None)
    print(f"setup {time.time() - t0:.1f} s: {args.frames} frames, {hb_mixed.n_masks} masks, {small.size} of them {SIDE[0]}x{SIDE[1]}", flush=True)

    eng = lifting.LiftEngine("cuda:0")
    st = torch.cuda.current_stream().cuda_stream
    out = {"workload": f"c4: {args.frames} frames x {cfg.n_masks} masks, canvas {W}x{H}, masks of cameras 3 and 4 cropped to {SIDE[0]}x{SIDE[1]}",
           "device": torch.cuda.get_device_name(0), "n_masks": hb_mixed.n_masks, "n_cropped_masks": int(small.size)}
    res = {}
    for name, hb in (("sized", hb_mixed), ("embedded", hb_emb), ("uncropped", hb_full)):
        eng.upload(hb)
        eng.b.packed.zero_()
        eng.stage_masks(st, "rle")
        torch.cuda.synchronize()
        res[name] = stored(eng)
        out[name] = dict(mask_stage_ms(eng, args.reps), total_runs=int(hb.rle_counts.size), run_bytes=int(hb.rle_counts.size) * 4)
        print(name, out[name], flush=True)
    same = bool(np.array_equal(res["sized"][0], res["embedded"][0]) and np.array_equal(res["sized"][1], res["embedded"][1]))
    out["sized_equals_embedded_bit_for_bit"] = same
    out["host_reencode"] = {"best_of_3_ms": round(best * 1e3, 3), "masks": int(small.size),
                            "extra_upload_bytes": out["embedded"]["run_bytes"] - out["sized"]["run_bytes"],
                            "size_table_bytes": int(hb_mixed.mask_wh.nbytes)}
    print(json.dumps(out, indent=1))
    if args.out:
        with open(args.out, "w") as fh:
            json.dump(out, fh, indent=1)
            fh.write("\n")
    if not same:
        raise SystemExit("the sized kernel and the plain kernel on the embedded lists differ")


if __name__ == "__main__":
    main()
