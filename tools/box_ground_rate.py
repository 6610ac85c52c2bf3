#!/usr/bin/env python3
"""Runs ON THE GPU BOX: what the opt-in ground stage costs (cm3d_box_ground: one launch behind the pass that streams every frame's
sweep rows once more), with HIP events and the median of --reps, on the C2-shaped batch bench.py times (256 frames x 20 masks) and on
the Waymo-shaped batch of C4 frames that tools/bev_fit_rate.py uses.  Per batch, in one run:

  * cm3d_box_ground alone from the raw rows (the default route) and from the materialised cloud (keep_cloud), cm3d_box_vertical alone
    and the projection launch alone as yardsticks, and the bytes the launch has to move against the HBM peak;
  * one pass over the resident batch without the option, with it, with the vertical stage and with both, and the span of the stage's
    two events inside the pass;
  * how many masks take each ground_src and each ground_status, and the members per mask.

Every timed configuration is first held against the host statement (on the cloud the engine materialises).  The synthetic frames are
rings on a flat ground with cylinders: the counts say how much work the launch had, nothing about real scenes.  Run it as one step
under a time limit of its own, like the other rate tools: timeout -k 10 900 python tools/box_ground_rate.py --out profiles/box_ground_rate.json
usage: tools/box_ground_rate.py [--frames 256] [--waymo-frames 32] [--reps 20] [--out FILE.json]"""
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
from cm3d_amd import boxground, boxvertical, lifting, synthetic as syn  # noqa: E402
from tools.bev_fit_rate import _waymo_frames, span_ms  # noqa: E402
from tools.kitti_obb_rate import pass_ms  # noqa: E402

HBM_PEAK_TBS = 8.0                                  # MI355X, spec; about 6.3 TB/s is what a float4 copy reaches


def project_ms(eng, reps):
    """Median over `reps` passes of the time between the two events around the projection launch, in ms."""
    runs = []
    for _ in range(reps):
        pair = (torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True))
        eng.run(masks="rle", project_events=pair)
        runs.append(pair)
    torch.cuda.synchronize()
    return float(np.median([a.elapsed_time(b) for a, b in runs]))


def measure(hb, classes, reps):
    out = dict(frames=int(hb.n_frames), masks=int(hb.n_masks), rows=int(hb.n_raw_rows), max_masks_per_frame=int(np.diff(hb.mask_off).max()))
    g, v = boxground.BoxGround(), boxvertical.BoxVertical()
    res = {}
    for key, kw in (("plain", {}), ("ground", dict(ground=g)), ("ground_cloud", dict(ground=g, keep_cloud=True)), ("vertical", dict(vertical=v)),
                    ("both", dict(vertical=v, ground=g))):
        eng = lifting.LiftEngine("cuda:0", classes=classes, **kw)
        eng.upload(hb)
        for _ in range(3):
            eng.run(masks="rle")
        torch.cuda.synchronize()
        out[f"pass_ms_{key}"] = pass_ms(eng, reps)
        if key == "plain":
            out["project_launch_ms"] = project_ms(eng, reps)
        if key in ("ground", "ground_cloud"):
            # (zref = what the pass left, as a second call takes it: every timed launch does the same work)
            out[f"box_{key}_alone_ms"] = pass_ms(eng, reps, lambda st, eng=eng: eng.stage_ground(st, zref=eng.b.ground_zref))
        if key == "ground":
            out["ground_span_in_pass_ms"] = span_ms(eng, reps)
        if key == "vertical":
            out["box_vertical_alone_ms"] = pass_ms(eng, reps, eng.stage_vertical)
        if key == "both":
            out["ground_span_in_pass_with_vertical_ms"] = span_ms(eng, reps)
        eng.run(masks="rle")                          # (a stage alone left its own z: one whole pass again)
        torch.cuda.synchronize()
        res[key] = eng.download(full=key == "ground_cloud")
        del eng
        torch.cuda.empty_cache()
    prior = (classes or lifting.ClassTable.nuscenes()).prior_wlh
    cloud = res["ground_cloud"]
    host = boxground.box_ground_host(cloud["points"], cloud["pt_off"], hb.mask_off, res["plain"]["box"], res["plain"]["flags"], prior, **g.params())
    for key in ("ground", "ground_cloud"):
        assert all(res[key][k].tobytes() == host[k].tobytes() for k in boxground.RESULTS + ("box",)), key
    vert = res["vertical"]
    host2 = boxground.box_ground_host(cloud["points"], cloud["pt_off"], hb.mask_off, vert["box"], vert["flags"], prior, zref=vert["vert_entry_z"],
                                      vert=vert, **g.params())
    assert all(res["both"][k].tobytes() == host2[k].tobytes() for k in boxground.RESULTS + ("box",))
    # what the launch has to move: every row of a frame once per workgroup of the frame
    out["masks_per_workgroup"] = chunk = int(lifting._lib.lib().cm3d_box_ground_chunk(hb.n_frames, out["max_masks_per_frame"]))
    chunks = np.full(hb.n_frames, max(1, -(-out["max_masks_per_frame"] // chunk)))      # (the grid is sized by the largest frame)
    rows = np.diff(np.asarray(hb.sweep_row_off)[np.asarray(hb.frame_sweep_off)])
    for key, per_row in (("ground", hb.bytes_per_row), ("ground_cloud", 16)):
        nbytes = int((rows * chunks).sum()) * int(per_row)
        ms = out[f"box_{key}_alone_ms"]
        out[f"{key}_bytes"] = nbytes
        out[f"{key}_tb_per_s"] = nbytes / (ms * 1e-3) / 1e12
        out[f"{key}_share_of_hbm_peak"] = out[f"{key}_tb_per_s"] / HBM_PEAK_TBS
    st, src, n = host["ground_status"], host["ground_src"], host["ground_n"]
    out["members"] = dict(total=int(n.sum()), largest=int(n.max()), mean=float(n.mean()), median=float(np.median(n)))
    out["ground_status"] = dict(ok=int((st == 0).sum()), few_points=int((st == 1).sum()), empty=int((st == 2).sum()), non_finite=int((st == 4).sum()))
    out["ground_src"] = dict(untouched=int((src == 0).sum()), ground_and_top=int((src == 1).sum()), prior_on_ground=int((src == 2).sum()))
    s2 = host2["ground_src"]
    out["ground_src_with_vertical"] = dict(untouched=int((s2 == 0).sum()), ground_and_top=int((s2 == 1).sum()), prior_on_ground=int((s2 == 2).sum()))
    out["ground_over_vertical"] = out["box_ground_alone_ms"] / out["box_vertical_alone_ms"]
    out["ground_over_project"] = out["box_ground_alone_ms"] / out["project_launch_ms"]
    out["pass_ratio"] = out["pass_ms_ground"] / out["pass_ms_plain"]
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
    out = dict(reps=args.reps, gen_s=round(time.time() - t0, 1), hbm_peak_tb_per_s=HBM_PEAK_TBS,
               note="the synthetic frames are rings on a flat ground with cylinders: the counts say how much work the launch had, nothing about "
                    "real scenes; the defaults of BoxGround() are untuned")
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
