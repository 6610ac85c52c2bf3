#!/usr/bin/env python3
"""CPU model of the lane search's control flow (csrc/boxes.hip k_lane_nn_grid): what a query costs in dependent load rounds
and in sequential candidate evaluations of its busiest lane, under the rule that gave every row segment of a ring batch to one lane
(and a long one to the whole wave, one after the other) and under the flat rule, where the wave scans the segments' points as one list.
numpy only.  It is a model of the control flow, not a measurement.

A query is one wave.  It visits ring batches [0..2], [3..5], [6..9], ... until the best distance is inside the rings seen; a batch is
cut into row segments, 64 per step.  Per step, behind one round of cell_start loads:
  segment rule   a segment of at most BIG_CELL points is scanned by its lane, PF points per round; a longer one by the wave, 64 per
                 round, one such segment after the other.  rounds = max ceil(len / PF) + sum ceil(len_big / 64); evaluations in the
                 busiest lane = max len + sum ceil(len_big / 64)
  flat rule      the step's T points are one list, 64 per round, the loads of ROUNDS rounds in flight together.
                 rounds = ceil(T / (64 ROUNDS)); evaluations = ceil(T / 64)
The exact scan behind MAX_RINGS costs the same under both.

    python tools/lane_flat_sim.py                       # bench.py's lane table, 5 000 centroids
    python tools/lane_flat_sim.py --points 3000 --extent 120 --queries 500
"""
import argparse
import json
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

MAX_CELLS, CELL0, MAX_RINGS = 32768, 4.0, 64
BIG_CELL, PF = 12, 4               # the segment rule's constants
ROUNDS = 4                         # LF_ROUNDS


def build_grid(lane):
    """k_lane_grid_build on the host: float32 geometry and binning, cells in row-major order, a stable cell sort."""
    f = np.float32
    l32 = np.asarray(lane, np.float64).astype(f).reshape(-1, 3)
    x, y = l32[:, 0], l32[:, 1]
    x0, y0 = x.min(), y.min()
    ex, ey = f(x.max() - x0), f(y.max() - y0)
    h = f(CELL0)
    while (float(np.floor(ex / h)) + 2.0) * (float(np.floor(ey / h)) + 1.0) > MAX_CELLS:
        h = f(h * f(1.25))
    inv_h = f(1.0) / h
    gw, gh = (int(np.floor(ex / h)) + 1) | 1, int(np.floor(ey / h)) + 1
    big = max(abs(float(x0)), abs(float(x.max())), abs(float(y0)), abs(float(y.max())))
    margin = f(f(f(16.0) * f(1.1920929e-7)) * f(big)) + f(f(1e-4) * h)
    ci = np.clip(np.floor((x - x0) * inv_h).astype(np.int64), 0, gw - 1)
    cj = np.clip(np.floor((y - y0) * inv_h).astype(np.int64), 0, gh - 1)
    cell = cj * gw + ci
    order = np.argsort(cell, kind="stable")
    start = np.zeros(gw * gh + 1, np.int64)
    np.cumsum(np.bincount(cell, minlength=gw * gh), out=start[1:])
    return dict(x0=float(x0), y0=float(y0), h=float(h), inv_h=float(inv_h), gw=gw, gh=gh, margin=float(margin), start=start, order=order,
                xy=l32[:, :2].astype(np.float64))


def batch_segments(g, qi, qj, r_lo, r_hi):
    """The batch's row segments as (a, b) ranges of the sorted table, in the kernel's order; a dead segment is (0, 0)."""
    w = r_hi - r_lo + 1
    segs = []
    if r_lo == 0:
        segs = [(qj - 2 + s, qi - 2, qi + 2) for s in range(5)]
    else:
        segs += [(qj - r_hi + s, qi - r_hi, qi + r_hi) for s in range(w)]
        segs += [(qj + r_lo + s, qi - r_hi, qi + r_hi) for s in range(w)]
        for m in range(2 * (2 * r_lo - 1)):
            row = qj - r_lo + 1 + (m >> 1)
            segs.append((row, qi + r_lo, qi + r_hi) if m & 1 else (row, qi - r_hi, qi - r_lo))
    out = []
    for row, c0, c1 in segs:
        c0, c1 = max(c0, 0), min(c1, g["gw"] - 1)
        if 0 <= row < g["gh"] and c0 <= c1:
            out.append((int(g["start"][row * g["gw"] + c0]), int(g["start"][row * g["gw"] + c1 + 1])))
        else:
            out.append((0, 0))
    return out


def step_cost(lens):
    """(rounds, evaluations) of one step under the segment rule and under the flat rule, the cell_start round not counted."""
    lens = np.asarray(lens, np.int64)
    small, big = lens[lens <= BIG_CELL], lens[lens > BIG_CELL]
    whole = int(((big + 63) // 64).sum())
    m = int(small.max(initial=0))
    T = int(lens.sum())
    return ((m + PF - 1) // PF + whole, m + whole), ((T + 64 * ROUNDS - 1) // (64 * ROUNDS), (T + 63) // 64)


def simulate(g, cent):
    """Every float32 centroid (K, >= 2) through the search.  Arrays over the queries: index (the neighbour found), batches, steps,
    rounds_old / rounds_flat (dependent load rounds behind the header, cell_start rounds included), evals_old / evals_flat (sequential
    evaluations in the busiest lane), points_old / points_flat (points evaluated in all) and step_points (a list: T of every step)."""
    K = cent.shape[0]
    res = {k: np.zeros(K, np.int64) for k in ("index", "batches", "steps", "rounds_old", "rounds_flat", "evals_old", "evals_flat",
                                               "points_old", "points_flat")}
    step_points = []
    N = g["xy"].shape[0]
    for k in range(K):
        cx, cy = float(np.float32(cent[k, 0])), float(np.float32(cent[k, 1]))
        qi = int(max(-1e6, min(1e6, np.floor((cx - g["x0"]) * g["inv_h"]))))
        qj = int(max(-1e6, min(1e6, np.floor((cy - g["y0"]) * g["inv_h"]))))
        out_i = -qi if qi < 0 else (qi - g["gw"] + 1 if qi >= g["gw"] else 0)
        out_j = -qj if qj < 0 else (qj - g["gh"] + 1 if qj >= g["gh"] else 0)
        best, r_done, resolved = (np.inf, 2 ** 31 - 1), max(out_i, out_j) - 1, False
        while r_done < MAX_RINGS:
            r_lo = r_done + 1
            r_hi = 2 if r_lo == 0 else min(MAX_RINGS, r_lo + max(2, r_lo // 2))
            segs = batch_segments(g, qi, qj, r_lo, r_hi)
            res["batches"][k] += 1
            for s0 in range(0, len(segs), 64):
                step = segs[s0:s0 + 64]
                (ro, eo), (rf, ef) = step_cost([b - a for a, b in step])
                T = sum(b - a for a, b in step)
                step_points.append(T)
                res["steps"][k] += 1
                res["rounds_old"][k] += 1 + ro; res["rounds_flat"][k] += 1 + rf
                res["evals_old"][k] += eo; res["evals_flat"][k] += ef
                res["points_old"][k] += T; res["points_flat"][k] += T
                if T:
                    j = np.concatenate([g["order"][a:b] for a, b in step])
                    d = np.sqrt((cx - g["xy"][j, 0]) ** 2 + (cy - g["xy"][j, 1]) ** 2)
                    i = np.lexsort((j, d))[0]
                    best = min(best, (float(d[i]), int(j[i])))
            r_done = r_hi
            if best[0] < r_done * g["h"] - g["margin"]:
                resolved = True
                break
            if qi - r_done <= 0 and qi + r_done >= g["gw"] - 1 and qj - r_done <= 0 and qj + r_done >= g["gh"] - 1:
                resolved = True
                break
        if not resolved:                                     # the exact scan of the whole table: eight loads per lane in flight
            d = np.sqrt((cx - g["xy"][:, 0]) ** 2 + (cy - g["xy"][:, 1]) ** 2)
            best = (float(d.min()), int(d.argmin()))
            for key, v in (("rounds", 1 + (N + 511) // 512), ("evals", (N + 63) // 64), ("points", N)):
                res[key + "_old"][k] += v; res[key + "_flat"][k] += v
        res["index"][k] = best[1]
    res["step_points"] = np.array(step_points, np.int64)
    return res


def summary(res):
    """mean, p90, p99 and max per query of the four cost columns."""
    return {k: [round(float(res[k].mean()), 2)] + [int(np.percentile(res[k], q)) for q in (90, 99)] + [int(res[k].max())]
            for k in ("rounds_old", "rounds_flat", "evals_old", "evals_flat")}


def main():
    from cm3d_amd import synthetic as syn
    ap = argparse.ArgumentParser()
    ap.add_argument("--points", type=int, default=50000)
    ap.add_argument("--extent", type=float, default=260.0)
    ap.add_argument("--seed", type=int, default=7)
    ap.add_argument("--queries", type=int, default=5000)
    args = ap.parse_args()
    lane = syn.make_lane_table([600.0, 1600.0], args.points, seed=args.seed, extent=args.extent)
    g = build_grid(lane)
    rng = np.random.default_rng(1)
    # the bench's objects: ego positions (600, 1600) +- 200 m, objects up to 55 m further out
    cent = np.array([600.0, 1600.0]) + rng.uniform(-200.0, 200.0, (args.queries, 2)) + rng.uniform(-55.0, 55.0, (args.queries, 2))
    res = simulate(g, cent.astype(np.float32))
    cc = np.diff(g["start"])
    occ = cc[cc > 0]
    sp = res["step_points"]
    print(json.dumps({
        "grid": {"gw": g["gw"], "gh": g["gh"], "h": g["h"], "occupied_cells": int(occ.size), "points_per_occupied_cell_p50_p90":
                 [int(np.percentile(occ, 50)), int(np.percentile(occ, 90))]},
        "per_query_mean_p90_p99_max": summary(res),
        "points_per_step_p50_p90_p99": [int(np.percentile(sp, q)) for q in (50, 90, 99)],
        "steps_of_at_most_256_points": round(float((sp <= 256).mean()), 3),
        "batches_per_query": round(float(res["batches"].mean()), 2),
        "queries_done_in_the_first_batch": round(float((res["batches"] == 1).mean()), 3),
    }, indent=1))


if __name__ == "__main__":
    main()
