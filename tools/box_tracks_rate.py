#!/usr/bin/env python3
"""Runs ON THE GPU BOX: what the opt-in box track stage costs (cm3d_box_tracks: one call of three launches behind cm3d_box_velocity),
with HIP events and the median of --reps.

1. On the C2-shaped batch bench.py times (256 frames x 20 masks), chained as scenes of --scene-frames keyframes 0.5 s apart as
   tools/box_velocity_rate.py does: the call alone, and one pass over the resident batch with the velocity stage only and with both.
   The synthetic frames are drawn independently of each other, so few boxes find a partner and nearly every track has one member: this
   number is a LOWER bound of the call's time on real scenes.
2. On synthetic link arrays whose tracks all run --lengths frames (16 and 40), --tracks of them side by side, the masks of a frame in
   a random order: the call alone.  Here the head's walk is as long as a scene.

The call alone is timed with min_length 1 and score "max", which leave the kept set and -- after the first call -- the scores as they
are, so that every repetition does the same work; the pass writes box and flags anew each time and runs with min_length 2 and "mean".
usage: tools/box_tracks_rate.py [--frames 256] [--scene-frames 16] [--tracks 320] [--lengths 16,40] [--window 2] [--reps 20] [--out FILE.json]"""
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
from cm3d_amd import _lib, lifting, synthetic as syn, tracks  # noqa: E402
from tools.box_velocity_rate import chained  # noqa: E402
from tools.kitti_obb_rate import pass_ms  # noqa: E402


def measure_batch(hb, reps, window):
    out = dict(frames=int(hb.n_frames), masks=int(hb.n_masks), links=int((hb.frame_next >= 0).sum()))
    vel = lifting.LiftEngine("cuda:0", velocity=lifting.Velocity())
    vel.upload(hb)
    for _ in range(3):
        vel.run(masks="rle")
    torch.cuda.synchronize()
    out["pass_ms_velocity"] = pass_ms(vel, reps)
    base = vel.download(full=False)
    del vel
    for name, tr in (("pass", tracks.Tracks(2, "mean", window)), ("stage", tracks.Tracks(1, "max", window))):
        eng = lifting.LiftEngine("cuda:0", velocity=lifting.Velocity(), tracks=tr)
        eng.upload(hb)
        for _ in range(3):
            eng.run(masks="rle")
        torch.cuda.synchronize()
        res = eng.download(full=False)
        host = tracks.box_tracks_host(base["box"], base["flags"], hb.mask_frame, base["next_match"], base["prev_match"], hb.frame_time,
                                      tr.min_length, tr.score, tr.smooth_window)
        assert all(np.array_equal(res[k], host[k]) for k in ("track_id", "track_pos", "track_len", "flags"))
        assert all(res[k].tobytes() == host[k].tobytes() for k in ("track_stat", "vel_smooth", "box")) and host["status"] == 0
        if name == "pass":
            out["pass_ms_tracks"] = pass_ms(eng, reps)
            out["dropped_by_min_length_2"] = int(((base["flags"] & 3) == 3).sum() - ((res["flags"] & 3) == 3).sum())
        else:
            out["stage_ms"] = pass_ms(eng, reps, eng.stage_tracks)
            out["kept"] = int(((res["flags"] & 3) == 3).sum())
            out["tracks"] = int((res["track_pos"] == 0).sum())
            out["longest_track"] = int(res["track_len"].max())
        del eng
    out["pass_ratio"] = out["pass_ms_tracks"] / out["pass_ms_velocity"]
    return out


def synthetic_links(n_tracks, length, seed=0):
    """n_tracks tracks through `length` frames 0.5 s apart, the masks of a frame in a random order: the arrays of cm3d_box_tracks."""
    rng = np.random.default_rng(seed)
    M = n_tracks * length
    slot = np.stack([rng.permutation(n_tracks) for _ in range(length)]) + (np.arange(length) * n_tracks)[:, None]      # [frame][track] -> mask
    nm, pm = np.full(M, -1, np.int32), np.full(M, -1, np.int32)
    nm[slot[:-1].ravel()], pm[slot[1:].ravel()] = slot[1:].ravel(), slot[:-1].ravel()
    box = np.zeros((M, _lib.BOX_STRIDE), np.float64)
    v = rng.uniform(-10, 10, (n_tracks, 2))
    for f in range(length):                       # track k starts at (8 k, 8 k) and moves at v[k]
        box[slot[f], 0:2] = v * (0.5 * f) + np.arange(n_tracks)[:, None] * 8.0
    box[:, 7], box[:, 9] = rng.random(M), 3.0
    return dict(box=box, flags=np.full(M, 3, np.int32), mask_frame=np.repeat(np.arange(length), n_tracks).astype(np.int32), next_match=nm,
                prev_match=pm, frame_time=0.5 * np.arange(length))


def measure_links(n_tracks, length, reps, window):
    L = _lib.lib()
    a = synthetic_links(n_tracks, length)
    M = len(a["flags"])
    host = tracks.box_tracks_host(a["box"], a["flags"], a["mask_frame"], a["next_match"], a["prev_match"], a["frame_time"], 1, "max", window)
    d = {k: torch.from_numpy(np.ascontiguousarray(v)).cuda() for k, v in a.items()}
    e = lambda *s, dtype=torch.int32: torch.empty(*s, dtype=dtype, device="cuda")
    tid, pos, ln, stat, vs = e(M), e(M), e(M), e(M, 4, dtype=torch.float64), e(M, 2, dtype=torch.float64)
    status = torch.zeros(1, dtype=torch.int32, device="cuda")
    ws = torch.empty(int(L.cm3d_box_tracks_workspace_bytes(M)), dtype=torch.uint8, device="cuda")
    st = torch.cuda.current_stream().cuda_stream

    def call():
        _lib.check(L.cm3d_box_tracks(d["box"].data_ptr(), d["flags"].data_ptr(), d["mask_frame"].data_ptr(), d["next_match"].data_ptr(),
                                     d["prev_match"].data_ptr(), d["frame_time"].data_ptr(), M, length, 1, tracks.score_code("max"), window, tid.data_ptr(),
                                     pos.data_ptr(), ln.data_ptr(), stat.data_ptr(), vs.data_ptr(), status.data_ptr(), ws.data_ptr(),
                                     ws.numel(), st), "cm3d_box_tracks")
    call()
    torch.cuda.synchronize()
    assert int(status.item()) == 0 and np.array_equal(ln.cpu().numpy(), host["track_len"]) and (host["track_len"] == length).all()
    assert stat.cpu().numpy().tobytes() == host["track_stat"].tobytes() and vs.cpu().numpy().tobytes() == host["vel_smooth"].tobytes()
    for _ in range(3):
        call()
    ev = []
    for _ in range(reps):
        x, y = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        x.record(); call(); y.record()
        ev.append((x, y))
    torch.cuda.synchronize()
    return dict(masks=M, tracks=n_tracks, length=length, stage_ms=float(np.median([x.elapsed_time(y) for x, y in ev])))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=256)
    ap.add_argument("--scene-frames", type=int, default=16)
    ap.add_argument("--tracks", type=int, default=320)
    ap.add_argument("--lengths", default="16,40")
    ap.add_argument("--window", type=int, default=2)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    # the frames first: their generation forks, which a process that holds the GPU must not do
    t0 = time.time()
    c2 = bench.make_batches_frames(syn.config("c2"), [0], args.frames, 16)[0]
    out = dict(reps=args.reps, scene_frames=args.scene_frames, window=args.window, gen_s=round(time.time() - t0, 1))
    lanes = [syn.make_lane_table([600.0, 1600.0], 50000, seed=7, extent=260.0)]
    out["c2"] = measure_batch(chained(c2, lanes, args.scene_frames), args.reps, args.window)
    del c2
    out["synthetic_links"] = [measure_links(args.tracks, int(n), args.reps, args.window) for n in args.lengths.split(",")]
    print(json.dumps(out), flush=True)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as fh:
            fh.write(json.dumps(out, indent=1) + "\n")


if __name__ == "__main__":
    main()
