#!/usr/bin/env python3
"""What the drivable-area test and the opt-in filtered pass cost on one MI355X.  The polygon table is the generated city of
tests/drivable_cases.py (one exterior ring, 50 holes) scaled to --edges edges and moved under the batch's ego poses; the batch is the
C2 shape (--frames frames of 20 masks, the first --distinct of them generated, then repeated).  Recorded:
  (a) query_us            the cm3d_points_in_polygons launch alone for the batch's medoids (frames x 20 points), HIP events, warmed
  (b) pass_ms             the filtered pass (drivable + both lane thresholds) against the plain pass over the same resident batch,
                          alternated in one process, HIP events around each pass
  (c) eval_filter         the evaluator's filter for --boxes boxes: ops.points_in_polygons end to end (upload, launch, download) with
                          the index resident, the launch alone, the host-side index build, and eval_detection.point_in_polygons
                          timed on --host-sample of the same boxes and scaled
usage: tools/drivable_rate.py [--edges 100000] [--frames 256] [--distinct 16] [--boxes 100000] [--host-sample 200] [--reps 20]
                              [--out profiles/drivable_rate.json]"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np  # noqa: E402

from cm3d_amd import drivable, eval_detection as ev, lifting, ops, synthetic as syn  # noqa: E402
from tests import drivable_cases as dc  # noqa: E402


def timed_pass(eng, torch):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    eng.run(masks="rle")
    b.record()
    b.synchronize()
    return a.elapsed_time(b)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--edges", type=int, default=100000)
    ap.add_argument("--frames", type=int, default=256)
    ap.add_argument("--distinct", type=int, default=16)
    ap.add_argument("--boxes", type=int, default=100000)
    ap.add_argument("--host-sample", type=int, default=200)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("tools/drivable_rate.py measures on the GPU: no HIP device")
    cfg = syn.config("c2")
    distinct = [syn.make_frame(cfg, i) for i in range(min(a.distinct, a.frames))]
    frames = [distinct[i % len(distinct)] for i in range(a.frames)]
    centre = np.mean([f.ego_xyz[:2] for f in distinct], 0)
    lanes = [syn.make_lane_table(centre, 50000, seed=7, extent=260.0)]
    shift = centre - np.array([dc.OX, dc.OY])
    table = [(ext + shift, [h + shift for h in holes]) for ext, holes in dc.city_table(n_ext=max(3, a.edges - 4000), n_holes=50)]
    t0 = time.perf_counter()
    ix = drivable.build_index([table])
    build_s = time.perf_counter() - t0
    res = dict(edges=int(ix["edge"].shape[0]), rings=int(ix["ring_info"].size), slabs=int(ix["tab_slab"][0, 1]), slab_entries=int(ix["ent_edge"].size),
               index_bytes=int(sum(ix[k].nbytes for k in drivable.INDEX_ARRAYS)), index_build_s=build_s, frames=a.frames)
    hb = lifting.pack_frames(frames, lanes, [0] * a.frames)
    hb.polygons = [table]
    res["masks"] = hb.n_masks
    plain = lifting.LiftEngine("cuda:0")
    filt = lifting.LiftEngine("cuda:0", filters=lifting.Stage2Filters(True, 20.0, 4.0))
    for eng in (plain, filt):
        eng.upload(hb)
        for _ in range(3):
            eng.run(masks="rle")
    torch.cuda.synchronize()
    got = filt.download(full=True)
    has = got["medoid_pos"] >= 0
    res.update(masks_with_medoid=int(has.sum()), on_road=int(got["on_road"].sum()), dropped=int((has & (got["medoid_pos_kept"] < 0)).sum()))
    # (b) alternated passes
    p_ms, f_ms = [], []
    for _ in range(a.reps):
        p_ms.append(timed_pass(plain, torch))
        f_ms.append(timed_pass(filt, torch))
    res["pass_ms"] = dict(plain=p_ms, filtered=f_ms, plain_median=float(np.median(p_ms)), filtered_median=float(np.median(f_ms)),
                          difference_median=float(np.median(np.array(f_ms) - np.array(p_ms))))
    # (a) the query alone, on the batch's medoids
    dix = filt.b.polygon_index
    xy = got["centroid_global"][:, :2].astype(np.float64)
    ms = []
    for _ in range(3 + a.reps):
        ops.points_in_polygons(dix, xy, device_ms=ms)
    res["query_us"] = dict(points=int(xy.shape[0]), launches=[1e3 * v for v in ms[3:]], median=float(1e3 * np.median(ms[3:])))
    # (c) the evaluator's filter
    rng = np.random.default_rng(5)
    ext = table[0][0]
    boxes = ext.min(0) + rng.random((a.boxes, 2)) * (ext.max(0) - ext.min(0))
    ops.points_in_polygons(dix, boxes[:1000])
    wall, dev = [], []
    for _ in range(5):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        inside = ops.points_in_polygons(dix, boxes, device_ms=dev)
        wall.append(time.perf_counter() - t0)
    sample = rng.choice(a.boxes, min(a.host_sample, a.boxes), replace=False)
    t0 = time.perf_counter()
    host = np.array([ev.point_in_polygons(table, *boxes[i]) for i in sample])
    host_s = time.perf_counter() - t0
    if not np.array_equal(host, inside[sample].astype(bool)):
        raise SystemExit("the GPU's answers differ from the host's on the sample")
    res["eval_filter"] = dict(boxes=a.boxes, inside=int(inside.sum()), gpu_end_to_end_s=float(np.median(wall)), gpu_launch_ms=float(np.median(dev)),
                              host_sample=int(sample.size), host_sample_s=host_s, host_scaled_s=host_s * a.boxes / sample.size,
                              host_over_gpu=host_s * a.boxes / sample.size / (float(np.median(wall)) + build_s))
    print(json.dumps({k: v for k, v in res.items() if k != "pass_ms"} | {"pass_ms": {k: v for k, v in res["pass_ms"].items() if "median" in k}}, indent=1))
    if a.out:
        with open(a.out, "w") as f:
            json.dump(res, f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()
