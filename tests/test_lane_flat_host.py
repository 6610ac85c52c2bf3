"""CPU: the lane search's flat scan.  (i) The map from a flat position to its segment and sorted-table index (cm3d_amd/csrc/lane_flat.h),
checked against a linear walk by a stand-alone program (tests/lane_flat_map.cpp) built with the address and undefined-behaviour
sanitizers.  (ii) The model of the search's control flow (tools/lane_flat_sim.py) on a small table: both rules visit the same points
and find the brute-force answer, and the flat rule never needs more load rounds or evaluations in a lane than the rule before it."""
import os
import shutil
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SANITIZED = ["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Wextra", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
             "-static-libasan", "-static-libubsan"]      # the runtimes inside the program, as tests/test_pipe_sched_host.py has them


def test_flat_position_map_under_sanitizers(tmp_path):
    """All-empty vectors, one segment of 1, lengths 12 .. 600 around 64 and 256, 64 live segments, totals 63 .. 600 over five segments,
    3000 random vectors: every position's index is the linear walk's, by binary search and (five segments) by compares."""
    if shutil.which("g++") is None:
        pytest.skip("no g++")
    exe = tmp_path / "lane_flat_map"
    r = subprocess.run(SANITIZED + ["-I", os.path.join(ROOT, "cm3d_amd", "csrc"), os.path.join(ROOT, "tests", "lane_flat_map.cpp"), "-o", str(exe)],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    r = subprocess.run([str(exe)], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "lane_flat_map ok" in r.stdout


def _sim():
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    try:
        import lane_flat_sim
    finally:
        sys.path.pop(0)
    return lane_flat_sim


def test_flat_scan_model_on_a_small_table():
    """3 000 lane points, 300 centroids (some outside the grid): the model's search finds the float64 brute-force neighbour under both
    rules, both evaluate the same number of points, and per query the flat rule needs at most as many dependent load rounds and at most
    as many evaluations in its busiest lane."""
    sim = _sim()
    from cm3d_amd import synthetic as syn
    lane = syn.make_lane_table([600.0, 1600.0], 3000, seed=5, extent=120.0)
    rng = np.random.default_rng(3)
    cent = np.array([600.0, 1600.0]) + rng.uniform(-150.0, 150.0, (300, 2))
    grid = sim.build_grid(lane)
    res = sim.simulate(grid, cent.astype(np.float32))
    l64 = lane[:, :2].astype(np.float32).astype(np.float64)
    c64 = cent.astype(np.float32).astype(np.float64)
    d = np.sqrt(((c64[:, None, :] - l64[None, :, :]) ** 2).sum(-1))
    assert np.array_equal(res["index"], d.argmin(1))
    assert np.array_equal(res["points_old"], res["points_flat"])
    assert (res["rounds_flat"] <= res["rounds_old"]).all() and (res["evals_flat"] <= res["evals_old"]).all()
    assert res["rounds_flat"].mean() < res["rounds_old"].mean() and res["evals_flat"].mean() < res["evals_old"].mean()
    assert (res["batches"] >= 1).all() and res["batches"].max() > 1
    table = sim.summary(res)
    assert set(table) == {"rounds_old", "rounds_flat", "evals_old", "evals_flat"} and all(len(v) == 4 for v in table.values())
