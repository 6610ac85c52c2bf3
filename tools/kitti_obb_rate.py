#!/usr/bin/env python3
"""Runs ON THE GPU BOX: what KITTI's oriented-box fit costs on the host and on the device (a18, src/kitti/2d_to_3d.py:855-876,
:1524), on a KITTI-shaped synthetic batch (256 frames of ~120 k points, one camera, 1024x309 masks, ratio 0.8366, 20 masks a frame):
  * one pass over the resident batch with and without the OBB stage, and the OBB launch alone (HIP events, median of --reps);
  * the host loop kitti.obb_yaw over the same in-mask lists (what `--obb host` runs per mask);
  * the entry point src/kitti/2d_to_3d.py end to end with --obb host and with --obb device over the frames written to disk
    (the time the script reports, from argument parsing to the last label file; the interpreter's start-up is not in it).
usage: tools/kitti_obb_rate.py [--frames 256] [--points 120000] [--reps 20] [--out FILE.json] [--pass-only]
--pass-only: only the passes (for a rocprofv3 --kernel-trace --stats run of its own)."""
import argparse
import json
import os
import pickle
import re
import subprocess
import sys
import tempfile
import time
import warnings

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np  # noqa: E402
import torch  # noqa: E402

from cm3d_amd import kitti as kt, lifting, synthetic as syn  # noqa: E402


def kitti_config(points):
    return syn.config("c2", n_points=points, n_sweeps=1, n_masks=20, n_cams=1, width=1024, height=309, ratio=kt.RATIO,
                      full_width=1224, full_height=370, focal=721.5377, n_beams=64, point_order="ring", ego_magnitude=0.0)


def pass_ms(eng, reps, stage=None):
    """Median time of `reps` passes (or of the stage alone, on the resident results) in ms."""
    st = torch.cuda.current_stream().cuda_stream
    ev = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        if stage is None:
            eng.run(masks="rle")
        else:
            stage(st)
        b.record()
        ev.append((a, b))
    torch.cuda.synchronize()
    return float(np.median([a.elapsed_time(b) for a, b in ev]))


def write_kitti_dir(d, frames, calibs):
    tr = os.path.join(d, "kitti", "training")
    mdir = os.path.join(d, "masks")
    for sub in (os.path.join(tr, "velodyne"), os.path.join(tr, "calib"), mdir):
        os.makedirs(sub, exist_ok=True)
    for i, (fr, cal) in enumerate(zip(frames, calibs)):
        fr.sweeps_raw[0].astype(np.float32).tofile(os.path.join(tr, "velodyne", f"{i:06d}.bin"))
        with open(os.path.join(tr, "calib", f"{i:06d}.txt"), "w") as fh:
            for k, v in cal.items():
                fh.write(f"{k}: " + " ".join(repr(float(x)) for x in np.asarray(v).reshape(-1)) + "\n")
        with open(os.path.join(mdir, f"{i}_masks.pkl"), "wb") as fh:
            pickle.dump(fr.rles, fh)
        with open(os.path.join(mdir, f"{i}_data.json"), "w") as fh:
            json.dump({"labels": fr.labels, "detection_scores": fr.scores}, fh)
    return os.path.join(d, "kitti"), mdir


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=256)
    ap.add_argument("--points", type=int, default=120000)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--out", default=None)
    ap.add_argument("--pass-only", action="store_true")
    args = ap.parse_args()
    cfg = kitti_config(args.points)
    t0 = time.time()
    made = [syn.make_kitti_frame(cfg, i) for i in range(args.frames)]
    frames, calibs = [m[0] for m in made], [m[1] for m in made]
    classes = lifting.ClassTable.nuscenes()
    hb = lifting.pack_frames(frames, [[[0.0, 0.0, 0.0]]], [0] * len(frames), classes)
    out = dict(frames=args.frames, points_per_frame=args.points, masks=int(hb.n_masks), width=cfg.width, height=cfg.height,
               ratio=cfg.ratio, raw_layout="quads" if hb.raw_stride == lifting._lib.RAW_QUADS else "rows", gen_s=round(time.time() - t0, 1))
    res = {}
    for obb in (False, True):
        eng = lifting.LiftEngine("cuda:0", classes=classes, obb=obb)
        eng.upload(hb)
        for _ in range(3):
            eng.run(masks="rle")
        torch.cuda.synchronize()
        key = "obb" if obb else "plain"
        out[f"pass_ms_{key}"] = pass_ms(eng, args.reps)
        if obb:
            out["obb_stage_ms"] = pass_ms(eng, args.reps, eng.stage_obb)
            out["medoid_stage_ms"] = pass_ms(eng, args.reps, eng.stage_medoid)
        res[key] = eng.download(full=True)
        del eng
        torch.cuda.empty_cache()
    for key in ("plain", "obb"):
        out[f"frames_per_s_pass_{key}"] = args.frames / (out[f"pass_ms_{key}"] * 1e-3)
    r = res["obb"]
    st = r["obb_status"]
    off = r["hit_off"]
    sizes = np.diff(off)
    out["obb_status_counts"] = {int(k): int(v) for k, v in zip(*np.unique(st, return_counts=True))}
    out["in_mask_points"] = dict(total=int(off[-1]), max=int(sizes.max()), median=int(np.median(sizes)))
    for key in ("hit_off", "hit_idx", "box", "flags", "medoid_pos"):
        assert np.array_equal(res["plain"][key], r[key]), key
    if not args.pass_only:
        # the host loop of --obb host over the same lists
        lists = [r["hit_xyz"][off[m]:off[m + 1], :3] for m in range(len(off) - 1) if off[m + 1] - off[m] > 3]
        with warnings.catch_warnings():
            warnings.simplefilter("ignore")
            t = time.perf_counter()
            for p in lists:
                try:
                    kt.obb_yaw(p)
                except Exception:
                    pass
            host_s = time.perf_counter() - t
        out["host_obb_loop_s"] = host_s
        out["host_obb_ms_per_list"] = host_s / max(1, len(lists)) * 1e3
        out["host_lists"] = len(lists)
        # the entry point end to end, both modes, on the same files
        with tempfile.TemporaryDirectory() as d:
            kdir, mdir = write_kitti_dir(d, frames, calibs)
            for mode in ("host", "device"):
                p = subprocess.run([sys.executable, "2d_to_3d.py", "--kitti-dir", kdir, "--mask-dir", mdir, "--ratio", str(cfg.ratio),
                                    "--obb", mode], cwd=os.path.join(ROOT, "src", "kitti"), capture_output=True, text=True, timeout=1800)
                if p.returncode != 0:
                    raise SystemExit(f"--obb {mode} failed: {p.stderr[-2000:]}")
                m = re.search(r"wrote (\d+) labels for (\d+) frames in ([0-9.]+) s", p.stdout)
                n_lab, n_fr, secs = int(m.group(1)), int(m.group(2)), float(m.group(3))
                out[f"e2e_{mode}"] = dict(labels=n_lab, frames=n_fr, seconds=secs, frames_per_s=n_fr / secs)
    line = json.dumps(out)
    print(line, flush=True)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as fh:
            fh.write(json.dumps(out, indent=1) + "\n")


if __name__ == "__main__":
    main()
