#!/usr/bin/env python3
"""Runs ON THE GPU BOX: what the opt-in ground strip costs (cm3d_ground_grid: one launch that streams every frame's sweep rows once per
tile of its grid; cm3d_ground_strip: three launches over the in-mask lists), with HIP events and the median of --reps, on the
C2-shaped batch bench.py times (256 frames x 20 masks) and on the Waymo-shaped batch of C4 frames that tools/bev_fit_rate.py uses.
Per batch, in one run:

  * the grid launch alone and the strip's three launches alone, from the raw rows (the default route) and from the materialised cloud
    (keep_cloud), cm3d_box_ground alone as the yardstick (the other stage that streams the sweep), and the bytes the grid launch has to
    move -- once from HBM, sixteen times through L2 -- against the HBM peak;
  * one pass over the resident batch without the option and with it, and the span of the stage's two events inside the pass;
  * the medoid stage alone on the raw and on the stripped lists;
  * the counts of gs_status and the points raw -> kept.

Every timed configuration is first held against the host statements (on the cloud the engine materialises).  The synthetic frames are
rings on a flat ground with cylinders: the counts say how much work the launches had, nothing about real scenes.  Run it as one step
under a time limit of its own, like the other rate tools: timeout -k 10 900 python tools/ground_strip_rate.py --out profiles/ground_strip_rate.json
usage: tools/ground_strip_rate.py [--frames 256] [--waymo-frames 32] [--reps 20] [--out FILE.json]"""
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
from cm3d_amd import boxground, groundstrip, lifting, synthetic as syn  # noqa: E402
from cm3d_amd._lib import check  # noqa: E402
from tools.bev_fit_rate import _waymo_frames  # noqa: E402
from tools.kitti_obb_rate import pass_ms  # noqa: E402

HBM_PEAK_TBS = 8.0                                  # MI355X, spec; about 6.3 TB/s is what a float4 copy reaches
TILES = 16                                          # csrc/groundstrip.hip: a frame's rows are streamed once per 16 x 16-cell tile of its grid


def strip_span_ms(eng, reps):
    """Median over `reps` stripped passes of the time between the strip's two events (the first pair behind the pass's five), in ms."""
    runs = []
    for _ in range(reps):
        ev = []
        eng.run(masks="rle", stage_events=ev)
        runs.append(ev)
    torch.cuda.synchronize()
    return float(np.median([ev[5].elapsed_time(ev[6]) for ev in runs]))


def grid_alone(eng):
    b, s = eng.b, eng.b.strip_desc
    cloud = b.points is not None
    p = lifting._ptr

    def call(st):
        check(eng.lib.cm3d_ground_grid(p(b.points) if cloud else None, p(b.pt_off) if cloud else None, None if cloud else p(b.raw), b.hb.raw_stride,
                                       p(b.sweep_xf), p(b.sweep_row_off), p(b.frame_sweep_off), b.S, b.halfw, b.pt_cap, s.origin, b.F, s.cell, s.down,
                                       s.up, s.quantile, s.min_points, s.grid_z, s.grid_n, st), "cm3d_ground_grid")
    return call


def strip_alone(eng):
    b, s = eng.b, eng.b.strip_desc
    p = lifting._ptr

    def call(st):
        check(eng.lib.cm3d_ground_strip(p(b.hit_xyz), p(b.hit_idx), p(b.hit_off), p(b.mask_frame), b.M, b.idx_cap, s.origin, s.grid_z, b.F, s.cell,
                                        s.margin, s.min_keep, s.gs_off, s.gs_tile_off, s.gs_idx, s.gs_xyz, s.gs_status, s.gs_dropped, s.ws, s.ws_bytes,
                                        st), "cm3d_ground_strip")
    return call


def medoid_on_stripped(eng):
    """cm3d_medoid2 on the stripped lists, as the pass's tail calls it (no work list of the raw lists' kind)."""
    b = eng.b
    p = lifting._ptr

    def call(st):
        check(eng.lib.cm3d_medoid2(p(b.gs_xyz), 0, 0, b.M, p(b.gs_off), p(b.gs_tile_off), 0, b.idx_cap, 0, p(b.medoid_pos), p(b.centroid), p(b.colsum),
                                   p(b.ws), b.ws_bytes, 0, eng._md_fb.data_ptr(), st), "cm3d_medoid2")
    return call


def measure(hb, classes, reps):
    out = dict(frames=int(hb.n_frames), masks=int(hb.n_masks), rows=int(hb.n_raw_rows))
    s, g = groundstrip.GroundStrip(), boxground.BoxGround()
    res = {}
    for key, kw in (("plain", {}), ("strip", dict(strip=s)), ("strip_cloud", dict(strip=s, keep_cloud=True)), ("ground", dict(ground=g))):
        eng = lifting.LiftEngine("cuda:0", classes=classes, **kw)
        eng.upload(hb)
        for _ in range(3):
            eng.run(masks="rle")
        torch.cuda.synchronize()
        out[f"pass_ms_{key}"] = pass_ms(eng, reps)
        if key == "plain":
            out["medoid_raw_lists_ms"] = pass_ms(eng, reps, eng.stage_medoid)
        if key in ("strip", "strip_cloud"):
            out[f"grid_{key}_alone_ms"] = pass_ms(eng, reps, grid_alone(eng))
            out[f"strip_{key}_alone_ms"] = pass_ms(eng, reps, strip_alone(eng))
        if key == "strip":
            out["strip_span_in_pass_ms"] = strip_span_ms(eng, reps)
            out["medoid_stripped_lists_ms"] = pass_ms(eng, reps, medoid_on_stripped(eng))
        if key == "ground":
            out["box_ground_alone_ms"] = pass_ms(eng, reps, lambda st, eng=eng: eng.stage_ground(st, zref=eng.b.ground_zref))
        eng.run(masks="rle")                          # (a stage alone left its own results: one whole pass again)
        torch.cuda.synchronize()
        res[key] = eng.download(full=key != "ground")
        del eng
        torch.cuda.empty_cache()
    cloud = res["strip_cloud"]
    grid_z, grid_n = groundstrip.ground_grid_host(cloud["points"], cloud["pt_off"], hb.ego_xyz, s.cell, s.down, s.up, s.quantile, s.min_points)
    gs_off, _, keep, status, dropped = groundstrip.strip_lists(cloud["hit_off"], cloud["hit_xyz"], hb.mask_frame, hb.ego_xyz, grid_z, s.cell, s.margin,
                                                               s.min_keep)
    for key in ("strip", "strip_cloud"):
        r = res[key]
        assert r["grid_n"].tobytes() == grid_n.tobytes() and r["grid_z"].tobytes() == grid_z.tobytes(), key
        assert r["gs_off"].tobytes() == gs_off.tobytes() and np.array_equal(r["gs_status"], status) and np.array_equal(r["gs_dropped"], dropped), key
        assert r["gs_xyz"].tobytes() == cloud["hit_xyz"][keep].tobytes() and np.array_equal(r["gs_idx"], cloud["hit_idx"][keep]), key
    # what the grid launch has to move: every row of a frame comes from HBM once and is read once per tile of the frame's grid, the
    # other fifteen times from L2
    rows = int(np.asarray(hb.sweep_row_off)[-1])
    for key, per_row in (("strip", hb.bytes_per_row), ("strip_cloud", 16)):
        ms = out[f"grid_{key}_alone_ms"]
        out[f"grid_{key}_hbm_bytes"] = nbytes = rows * int(per_row)
        out[f"grid_{key}_hbm_tb_per_s"] = nbytes / (ms * 1e-3) / 1e12
        out[f"grid_{key}_share_of_hbm_peak"] = out[f"grid_{key}_hbm_tb_per_s"] / HBM_PEAK_TBS
        out[f"grid_{key}_read_bytes"] = nbytes * TILES
        out[f"grid_{key}_read_tb_per_s"] = nbytes * TILES / (ms * 1e-3) / 1e12
    out["gs_status"] = dict(stripped=int((status == 0).sum()), kept_whole=int((status == 1).sum()), empty=int((status == 2).sum()))
    out["lists_with_drops"] = int((dropped > 0).sum())
    out["points"] = dict(raw=int(cloud["hit_off"][-1]), kept=int(gs_off[-1]))
    out["cells"] = dict(with_estimate=int(np.isfinite(grid_z).sum()), occupied=int((grid_n > 0).sum()), of=int(grid_n.size))
    out["medoids_moved"] = int((res["strip"]["centroid"] != res["plain"]["centroid"]).any(1).sum())
    out["grid_over_box_ground"] = out["grid_strip_alone_ms"] / out["box_ground_alone_ms"]
    out["pass_ratio"] = out["pass_ms_strip"] / out["pass_ms_plain"]
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
               note="the synthetic frames are rings on a flat ground with cylinders: the counts say how much work the launches had, nothing "
                    "about real scenes; the defaults of GroundStrip() are untuned")
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
