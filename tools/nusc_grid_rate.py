#!/usr/bin/env python3
"""What the SAM3D fusion grid search of src/nuscenes/linear_matching.py costs per alpha, loop against sweep, on one MI355X.
The set is seeded and val-shaped: --samples samples with the box counts of `bench.py --fusion` (5..44 lifted boxes a sample, 70 % of
them with a jittered SAM3D twin, 10..49 SAM3D boxes of its own) and 20..49 annotations a sample, written as a nuScenes table set so
that the evaluator's own loaders and filters run; scores in [0.05, 1] x [0.25, 1] (a grid of about 100 alphas).  Timed, after a
warm-up of both paths on a small set:
  (a) loop_s_per_alpha    the loop of fusion.grid_search with eval_detection.DetectionEval (fuse, dump, reload, filter, Python
                          matching) on --loop-alphas alphas of a SUBSET of --subset samples, once
  (b) sweep_s             fusion.grid_search_device end to end on the same subset and on the full set, --reps runs each
  (c) match_device_ms     the cm3d_nusc_match call(s) alone, HIP events
  (d) stages_s            where (b) goes on the full set: parse + box matching, candidates, filters + pack, the matcher call,
                          the host tail (sort, curves, AP per alpha), the two files
usage: tools/nusc_grid_rate.py [--samples 6019] [--subset 600] [--loop-alphas 4] [--reps 3] [--out profiles/nusc_grid_rate.json]"""
import argparse
import json
import os
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np  # noqa: E402

from cm3d_amd import eval_detection as ev, fusion, nusc_eval, nusc_io, ops  # noqa: E402

CLASSES = list(ev.CVPR_2019["class_range"])
CATEGORY = {"car": "vehicle.car", "truck": "vehicle.truck", "bus": "vehicle.bus.rigid", "trailer": "vehicle.trailer",
            "construction_vehicle": "vehicle.construction", "pedestrian": "human.pedestrian.adult", "motorcycle": "vehicle.motorcycle",
            "bicycle": "vehicle.bicycle", "traffic_cone": "movable_object.trafficcone", "barrier": "movable_object.barrier"}


def make_set(root, n_samples, seed):
    """-> (tables, pred_objects, sam3d_objects)"""
    rng = np.random.default_rng(seed)
    ver = "v1.0-rate"
    t = {k: [] for k in nusc_io.TABLES + nusc_io.ANNOTATION_TABLES}
    t["sensor"].append({"token": "lidar", "channel": "LIDAR_TOP", "modality": "lidar"})
    t["calibrated_sensor"].append({"token": "cs", "sensor_token": "lidar", "translation": [0, 0, 0], "rotation": [1, 0, 0, 0], "camera_intrinsic": []})
    t["log"].append({"token": "log", "location": "nowhere"})
    t["scene"].append({"token": "scene", "name": "scene-0001", "log_token": "log", "nbr_samples": n_samples, "first_sample_token": "s0",
                       "last_sample_token": f"s{n_samples - 1}"})
    for name in CLASSES:
        t["category"].append({"token": "cat-" + name, "name": CATEGORY[name]})
        t["instance"].append({"token": "inst-" + name, "category_token": "cat-" + name})
    pred, sam = {}, {}

    def obj(tok, xy, name, score):
        yaw = float(rng.uniform(-np.pi, np.pi))
        return dict(sample_token=tok, translation=[float(xy[0]), float(xy[1]), 1.0], size=[float(rng.uniform(0.8, 2.5)), float(rng.uniform(1.5, 5.5)), 1.5],
                    rotation=[float(np.cos(yaw / 2)), 0.0, 0.0, float(np.sin(yaw / 2))], velocity=[0, 0], detection_name=name,
                    detection_score=score, attribute_name="")
    for i in range(n_samples):
        tok = f"s{i}"
        centre = rng.uniform(-1, 1, 2) * (700.0, 1500.0)
        t["sample"].append({"token": tok, "scene_token": "scene", "timestamp": 1000000 * i, "prev": f"s{i - 1}" if i else "",
                            "next": f"s{i + 1}" if i + 1 < n_samples else ""})
        t["ego_pose"].append({"token": "ep" + tok, "translation": [float(centre[0]), float(centre[1]), 0.0], "rotation": [1, 0, 0, 0], "timestamp": 1000000 * i})
        t["sample_data"].append({"token": "sd" + tok, "sample_token": tok, "ego_pose_token": "ep" + tok, "calibrated_sensor_token": "cs",
                                 "is_key_frame": True, "filename": "", "timestamp": 1000000 * i, "prev": "", "next": ""})
        n_gt = int(rng.integers(20, 50))
        g = centre + rng.uniform(-40, 40, (n_gt, 2))
        g_name = [CLASSES[int(k)] for k in rng.integers(0, 10, n_gt)]
        for k in range(n_gt):
            t["sample_annotation"].append({"token": f"a{i}-{k}", "sample_token": tok, "instance_token": "inst-" + g_name[k],
                                           "translation": [float(g[k, 0]), float(g[k, 1]), 1.0], "size": [2.0, 4.5, 1.5], "rotation": [1, 0, 0, 0],
                                           "prev": "", "next": "", "num_lidar_pts": 10, "num_radar_pts": 0, "attribute_tokens": [], "visibility_token": "4"})
        pred[tok], sam[tok] = [], []
        for _ in range(int(rng.integers(5, 45))):
            if rng.random() < 0.6:
                k = int(rng.integers(n_gt))
                pred[tok].append(obj(tok, g[k] + rng.normal(0, 0.5, 2), g_name[k], round(float(rng.uniform(0.05, 1.0)), 2)))
            else:
                pred[tok].append(obj(tok, centre + rng.uniform(-40, 40, 2), CLASSES[int(rng.integers(10))], round(float(rng.uniform(0.05, 0.7)), 2)))
            if rng.random() < 0.7:
                b = pred[tok][-1]
                sam[tok].append(dict(b, translation=[b["translation"][0] + float(rng.normal(0, 0.2)), b["translation"][1] + float(rng.normal(0, 0.2)), 1.0],
                                     detection_score=round(float(rng.uniform(0.25, 1.0)), 2)))
        for _ in range(int(rng.integers(10, 50))):
            sam[tok].append(obj(tok, centre + rng.uniform(-40, 40, 2), CLASSES[int(rng.integers(10))], round(float(rng.uniform(0.25, 1.0)), 2)))
    os.makedirs(os.path.join(root, ver), exist_ok=True)
    for name, rows in t.items():
        with open(os.path.join(root, ver, name + ".json"), "w") as f:
            json.dump(rows, f)
    return nusc_io.NuscTables(ver, root), {"meta": {}, "results": pred}, {"meta": {}, "results": sam}


def run_loop(tables, cfg, pred, sam, d, n_alphas):
    """The body of fusion.grid_search on n_alphas alphas spread over the grid."""
    sb, ss, s_max, s_min = fusion.parse_results(sam["results"], zero_min_quirk=True)
    pb, ps, p_max, p_min = fusion.parse_results(pred["results"])
    pm, sm = fusion.match_samples(pb, sb)
    grid = fusion.alpha_grid(p_min, p_max, s_min, s_max)
    pick = [grid[int(i)] for i in np.linspace(0, len(grid) - 1, n_alphas)]
    per, scores = [], []
    for alpha in pick:
        t0 = time.perf_counter()
        fused, _ = fusion.fuse(pb, ps, sb, ss, pm, sm, alpha)
        path = os.path.join(d, "loop_cur.json")
        with open(path, "w") as f:
            json.dump(fused, f)
        scores.append(ev.DetectionEval(tables, cfg, path, None, None, False, False, verbose=False).main()["mean_ap"])
        per.append(time.perf_counter() - t0)
        print(f"loop alpha {alpha}: {scores[-1]} in {per[-1]:.2f} s", flush=True)
    return pick, per, scores, grid


def sweep_runs(scorer, pred, sam, d, reps):
    out = []
    for _ in range(reps):
        t0 = time.perf_counter()
        r = fusion.grid_search_device(pred, sam, scorer, os.path.join(d, "cur.json"), os.path.join(d, "best.json"), verbose=False)
        out.append(time.perf_counter() - t0)
    return out, r


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--samples", type=int, default=6019)
    ap.add_argument("--subset", type=int, default=600)
    ap.add_argument("--loop-alphas", type=int, default=4)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("tools/nusc_grid_rate.py measures on the GPU: no HIP device")
    cfg = ev.config_factory()
    with tempfile.TemporaryDirectory() as d:
        tb, p, s = make_set(os.path.join(d, "warm"), 24, 1)                     # warm-up: code objects, allocator, both paths
        run_loop(tb, cfg, p, s, d, 1)
        fusion.grid_search_device(p, s, nusc_eval.GridScorer(tb, cfg), os.path.join(d, "w_cur.json"), os.path.join(d, "w_best.json"), verbose=False)
        torch.cuda.synchronize()

        t0 = time.perf_counter()
        tables, pred, sam = make_set(os.path.join(d, "full"), a.samples, 2)
        res = dict(samples=a.samples, predictions=sum(len(v) for v in pred["results"].values()), sam3d_boxes=sum(len(v) for v in sam["results"].values()),
                   ground_truth=len(tables.t["sample_annotation"]), gen_s=time.perf_counter() - t0)
        # the subset as a table set of its own (the loop reloads and refilters the ground truth of its tables per alpha)
        sub_tables, sub_pred, sub_sam = make_set(os.path.join(d, "sub"), a.subset, 2)      # same seed: the first samples of the full set
        # (a)
        pick, per, l_scores, grid = run_loop(sub_tables, cfg, sub_pred, sub_sam, d, a.loop_alphas)
        res.update(subset_samples=a.subset, subset_alphas_in_grid=len(grid), loop_alphas=[float(x) for x in pick], loop_s=[float(x) for x in per],
                   loop_s_per_alpha=float(np.mean(per)), loop_scores=l_scores)
        # (b) subset
        t0 = time.perf_counter()
        sub_scorer = nusc_eval.GridScorer(sub_tables, cfg)
        res["subset_scorer_init_s"] = time.perf_counter() - t0
        sub_s, r = sweep_runs(sub_scorer, sub_pred, sub_sam, d, a.reps)
        same = [r[2][grid.index(al)] == sc for al, sc in zip(pick, l_scores)]
        res.update(subset_sweep_s=[float(x) for x in sub_s], subset_sweep_s_median=float(np.median(sub_s)), subset_same_scores=bool(all(same)),
                   subset_loop_scaled_to_grid_s=float(np.mean(per)) * len(grid),
                   subset_loop_over_sweep=float(np.mean(per)) * len(grid) / (float(np.median(sub_s)) + res["subset_scorer_init_s"]))
        print(json.dumps(res, indent=1), flush=True)
        # (d) the full set, stage by stage
        t0 = time.perf_counter()
        scorer = nusc_eval.GridScorer(tables, cfg)
        res["scorer_init_s"] = time.perf_counter() - t0
        t0 = time.perf_counter()
        sb, ss, s_max, s_min = fusion.parse_results(sam["results"], zero_min_quirk=True)
        pb, ps, p_max, p_min = fusion.parse_results(pred["results"])
        pm, sm = fusion.match_samples(pb, sb)
        alphas = fusion.alpha_grid(p_min, p_max, s_min, s_max)
        t1 = time.perf_counter()
        cands = fusion.nusc_candidates(pb, ps, sb, ss, pm, sm)
        t2 = time.perf_counter()
        packed = nusc_eval.pack(scorer.filtered(cands), scorer.gt_boxes, cfg.class_names, cfg.dist_ths)
        t3 = time.perf_counter()
        dev_ms, call_s = [], []

        def matcher(pk, al):
            ms = []
            t = time.perf_counter()
            out = ops.nusc_match(pk, al, device_ms=ms)
            call_s.append(time.perf_counter() - t)
            dev_ms.append(sum(ms))
            return out
        score_s = []
        for _ in range(a.reps):
            t = time.perf_counter()
            scorer.score(cands, alphas, matcher)
            score_s.append(time.perf_counter() - t)
        t4 = time.perf_counter()
        for al in (alphas[-1], alphas[len(alphas) // 2]):
            with open(os.path.join(d, "f.json"), "w") as f:
                json.dump(fusion.fuse(pb, ps, sb, ss, pm, sm, al)[0], f)
        t5 = time.perf_counter()
        n_cand, n_gt = np.diff(packed["cand_off"]), np.diff(packed["gt_off"])
        tail = float(np.median(score_s)) - (t3 - t2) - float(np.median(call_s))
        res.update(alphas=len(alphas), matched_pairs=sum(len(v) for v in pm.values()), candidates=len(cands[0]), candidates_after_filters=int(n_cand.sum()),
                   groups=int(n_cand.size), groups_with_candidates=int((n_cand > 0).sum()), largest_group=[int(n_cand.max()), int(n_gt.max())],
                   static_groups_with_candidates=int(sum(1 for g in np.flatnonzero(n_cand > 0)
                                                         if not packed["cand_kind"][packed["cand_off"][g]:packed["cand_off"][g + 1]].any())),
                   stages_s=dict(parse_and_box_matching=t1 - t0, candidates=t2 - t1, filters_and_pack=t3 - t2, matcher_call=float(np.median(call_s)),
                                 host_tail=tail, two_files=t5 - t4),
                   matcher_call_s=[float(x) for x in call_s], match_device_ms=[float(x) for x in dev_ms], match_device_ms_median=float(np.median(dev_ms)))
        print(json.dumps(res, indent=1), flush=True)
        # (b) full set
        full_s, r = sweep_runs(scorer, pred, sam, d, a.reps)
        total = float(np.median(full_s))
        res.update(sweep_s=[float(x) for x in full_s], sweep_s_median=total, sweep_s_per_alpha=total / len(alphas), best_alpha=float(r[0]), best_score=float(r[1]),
                   host_tail_share=tail / total, matcher_call_share=float(np.median(call_s)) / total,
                   loop_s_per_alpha_scaled_by_samples=float(np.mean(per)) * a.samples / a.subset)
    print(json.dumps(res, indent=1))
    if a.out:
        with open(a.out, "w") as f:
            json.dump(res, f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()
