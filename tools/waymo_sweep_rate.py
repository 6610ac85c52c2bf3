#!/usr/bin/env python3
"""What the SAM3D fusion grid search of src/waymo/linear_matching.py costs per alpha, loop against sweep, on one MI355X.
The set is the G11 generator's random_set (tests/golden/gen_golden_waymo_metrics.py) at --frames frames; the SAM3D file holds
jittered copies of --share of the predictions (so that matched pairs exist) and a few boxes of its own, scores in [0.25, 1]
(a grid of about 100 alphas).  Timed, after a warm-up of both paths on a small set:
  (a) loop_s          fusion.waymo_grid_search with the in-process GPU evaluator (CM3D_WAYMO_METRICS=native), end to end, once
  (b) loop_gpu_calls_s  the ops.waymo_metrics calls inside (a) alone (upload, kernels, download; host packing excluded)
  (c) sweep_s         fusion.waymo_grid_search_device end to end, median of --reps
  (d) sweep_device_ms the cm3d_waymo_metrics_sweep call(s) on the device, HIP events, median of --reps
and where (c) goes: parse + match, candidates + pack, ops.waymo_metrics_sweep, counts -> 32 lines -> score, two files.
usage: tools/waymo_sweep_rate.py [--frames 2000] [--share 0.6] [--reps 3] [--out profiles/waymo_sweep_rate.json]"""
import argparse
import importlib.util
import json
import os
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np  # noqa: E402

from cm3d_amd import fusion, ops, waymo as wm, waymo_eval as we  # noqa: E402


def generator():
    spec = importlib.util.spec_from_file_location("gen_g11", os.path.join(ROOT, "tests", "golden", "gen_golden_waymo_metrics.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def make_set(frames, share, seed):
    rng = np.random.default_rng(seed)
    P, G = generator().random_set(rng, frames, gt_rate=6, fp_rate=3)
    pred = wm.decode_objects(wm.encode_objects(P))
    S = []
    for o in pred:
        if rng.uniform() < share:
            c = [o["center"][0] + float(rng.normal(0, 0.1)), o["center"][1] + float(rng.normal(0, 0.1)), o["center"][2] + float(rng.normal(0, 0.05))]
            S.append(wm.encode_object(c, o["length"] * float(rng.uniform(0.95, 1.05)), o["width"], o["height"],
                                      o["heading"] + float(rng.normal(0, 0.1)), o["type"], float(rng.uniform(0.25, 1)), o["context_name"],
                                      o["timestamp_micros"]))
        elif rng.uniform() < 0.3:          # a SAM3D box of its own in the same frame
            S.append(wm.encode_object([float(rng.uniform(-75, 75)), float(rng.uniform(-75, 75)), 0.5], 4.5, 2.0, 1.6, float(rng.uniform(-3, 3)), 1,
                                      float(rng.uniform(0.25, 1)), o["context_name"], o["timestamp_micros"]))
    return pred, wm.decode_objects(wm.encode_objects(S)), we.decode_objects(wm.encode_objects(G))


def run_loop(pred, sam, gt, d):
    calls, scores = [], []

    def evaluate(path):
        packed = we.pack(we.read_objects(path), gt)
        t0 = time.perf_counter()
        counts, hsum = ops.waymo_metrics(packed)                # returns host arrays: the call has finished
        calls.append(time.perf_counter() - t0)
        scores.append(we._finish(counts, hsum)[0]["Overall/L2 mAP"])
        print(f"loop alpha {len(scores)}: {scores[-1]}", flush=True)
        return scores[-1]
    t0 = time.perf_counter()
    alpha, score = fusion.waymo_grid_search(pred, sam, evaluate, os.path.join(d, "loop_cur.bin"), os.path.join(d, "loop_best.bin"), verbose=False)
    return time.perf_counter() - t0, calls, scores, alpha, score


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=2000)
    ap.add_argument("--share", type=float, default=0.6)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("tools/waymo_sweep_rate.py measures on the GPU: no HIP device")
    with tempfile.TemporaryDirectory() as d:
        small = make_set(24, a.share, 1)                        # warm-up: code objects, allocator, both paths
        run_loop(*small, d)
        fusion.waymo_grid_search_device(*small, os.path.join(d, "w_cur.bin"), os.path.join(d, "w_best.bin"), verbose=False)
        torch.cuda.synchronize()

        t0 = time.perf_counter()
        pred, sam, gt = make_set(a.frames, a.share, 2)
        res = dict(frames=a.frames, predictions=len(pred), sam3d_boxes=len(sam), ground_truth=len(gt), gen_s=time.perf_counter() - t0)
        # where the sweep's time goes, stage by stage
        t0 = time.perf_counter()
        sb, ss, s_max, s_min = fusion.waymo_parse(sam, zero_min_quirk=True)
        pb, ps, p_max, p_min = fusion.waymo_parse(pred)
        pm, sm = fusion.match_samples(pb, sb)
        alphas = fusion.waymo_alpha_grid(p_min, p_max, s_min, s_max)
        t1 = time.perf_counter()
        packed = we.pack_candidates(*fusion.waymo_candidates(pb, ps, sb, ss, pm, sm), gt)
        t2 = time.perf_counter()
        dev_ms, call_s = [], []
        for _ in range(a.reps):
            ms = []
            t = time.perf_counter()
            counts, hsum = ops.waymo_metrics_sweep(packed, alphas, device_ms=ms)
            call_s.append(time.perf_counter() - t)
            dev_ms.append(sum(ms))
        t3 = time.perf_counter()
        for i in range(len(alphas)):
            fusion.parse_waymo_metrics(we.format_metrics(we.metrics_from_counts(counts[i], hsum[i])))
        t4 = time.perf_counter()
        wm.encode_objects(fusion.fuse_waymo(pb, ps, sb, ss, pm, sm, alphas[-1]))
        wm.encode_objects(fusion.fuse_waymo(pb, ps, sb, ss, pm, sm, alphas[0]))
        t5 = time.perf_counter()
        co, go, static = packed["cand_off"], packed["gt_off"], packed["group_static"].astype(bool)
        n_cand = np.diff(co)
        res.update(alphas=len(alphas), alpha_range=[float(alphas[-1]), float(alphas[0])], matched_pairs=sum(len(v) for v in pm.values()),
                   groups=int(static.size), candidates_in_groups=int(n_cand.sum()), pairs_cand_x_gt=int(np.sum(n_cand * np.diff(go))),
                   largest_group_side=int(max(n_cand.max(), np.diff(go).max())), static_groups=int(static.sum()),
                   static_group_share=float(static.mean()), static_groups_with_candidates=int((static & (n_cand > 0)).sum()),
                   moving_groups=int((~static).sum()), candidates_in_static_groups_share=float(n_cand[static].sum() / max(n_cand.sum(), 1)),
                   sweep_stages_s=dict(parse_and_match=t1 - t0, candidates_and_pack=t2 - t1, counts_to_scores=t4 - t3, two_files=t5 - t4),
                   sweep_call_s=[float(x) for x in call_s], sweep_call_s_median=float(np.median(call_s)),
                   sweep_device_ms=[float(x) for x in dev_ms], sweep_device_ms_median=float(np.median(dev_ms)))
        print(json.dumps(res, indent=1), flush=True)
        # (c) end to end
        sweep_s = []
        for _ in range(a.reps):
            t0 = time.perf_counter()
            s_alpha, s_score, s_scores = fusion.waymo_grid_search_device(pred, sam, gt, os.path.join(d, "cur.bin"), os.path.join(d, "best.bin"),
                                                                         verbose=False)
            sweep_s.append(time.perf_counter() - t0)
        res.update(sweep_s=[float(x) for x in sweep_s], sweep_s_median=float(np.median(sweep_s)))
        print(json.dumps(dict(sweep_s=sweep_s)), flush=True)
        # (a), (b): the loop, once -- its length leaves no room for repeats; the spread of its calls is in loop_gpu_call_s_*
        loop_s, calls, l_scores, l_alpha, l_score = run_loop(pred, sam, gt, d)
        same_files = all(open(os.path.join(d, x), "rb").read() == open(os.path.join(d, "loop_" + x), "rb").read() for x in ("cur.bin", "best.bin"))
        res.update(loop_s=loop_s, loop_gpu_calls_s=float(np.sum(calls)), loop_gpu_call_s_median=float(np.median(calls)),
                   loop_gpu_call_s_min_max=[float(np.min(calls)), float(np.max(calls))], loop_s_per_alpha=loop_s / len(alphas),
                   same_scores=bool(l_scores == s_scores), same_best=bool((l_alpha, l_score) == (s_alpha, s_score)), same_files=bool(same_files),
                   best_alpha=float(s_alpha), best_score=float(s_score),
                   loop_over_sweep=loop_s / res["sweep_s_median"],
                   loop_gpu_calls_over_sweep_call=float(np.sum(calls)) / res["sweep_call_s_median"])
    print(json.dumps(res, indent=1))
    if a.out:
        with open(a.out, "w") as f:
            json.dump(res, f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()
