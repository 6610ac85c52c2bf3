"""GPU: points in drivable-area polygons (cm3d_points_in_polygons), the stage-2 filters (cm3d_stage2_filter) and the filtered pass
(cm3d_lift_pass_filtered) through LiftEngine and the entry points.  The reference of the point test is
eval_detection.point_in_polygons on the cases of tests/drivable_cases.py (computed once per process); of the filtered pass, the
host restatement of the rule (drivable.filter_rule) on an unfiltered pass and the oracle's stage 2 on the masks it keeps.

Box columns: flags, lane yaw / distance, score and class are compared exactly with the oracle, the translation and rotation of the
classes that are not pushed too.  For the pushed classes k_box_nms (unchanged here) differs from the C oracle by the ulp between the
device's and the host's float32 cos / sin (tests/test_gpu_stage2.py: at most 2.2e-6 seen, bound BOX_TIGHT = 1e-5): those columns
are held to that bound against the oracle and, exactly, to the bytes the plain pass writes for the same mask."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

from tests import drivable_cases as dc
from tests.optin_pass_cases import expected_filtered         # the host restatement of the filtered pass (moved there: the composed expectation uses it)

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BOX_TIGHT = 1e-5        # tests/test_gpu_stage2.py


@pytest.mark.parametrize("name", dc.CASE_NAMES)
def test_points_in_polygons_equals_brute_force(name):
    from cm3d_amd import ops
    c = dc.all_cases()[name]
    got = ops.points_in_polygons(c["tables"], c["xy"], c["table"])
    exp = dc.expected(name)
    assert got.dtype == np.uint8 and np.array_equal(got, exp), f"{name}: {np.flatnonzero(got != exp)[:8]}"


def test_points_in_polygons_edge_arguments():
    from cm3d_amd import drivable, ops
    a = dc.all_cases()["A_square_hole"]
    assert ops.points_in_polygons(a["tables"], np.zeros((0, 2))).size == 0
    assert ops.points_in_polygons([], a["xy"][:5]).tolist() == [0] * 5
    # a table number out of range reads as "outside"; NaN and inf coordinates are outside
    inside = a["xy"][dc.expected("A_square_hole") == 1][:4]
    assert ops.points_in_polygons(a["tables"], inside, [0, 1, -1, 0]).tolist() == [1, 0, 0, 1]
    odd = np.array([(np.nan, dc.OY), (dc.OX, np.nan), (np.inf, dc.OY), (-np.inf, dc.OY), (dc.OX, np.inf)])
    assert ops.points_in_polygons(a["tables"], odd).tolist() == drivable.points_on_road(a["tables"], odd, [0] * 5).tolist() == [0] * 5
    # an index uploaded once serves several calls
    dix = ops.upload_polygon_index(drivable.build_index(a["tables"]))
    assert np.array_equal(ops.points_in_polygons(dix, a["xy"]), dc.expected("A_square_hole"))


# ------------------------------------------------------------------------------------------------ the filtered pass
def _half_mask(rle):
    """The mask with the pixels behind its middle run dropped: a second, different detection of the same object."""
    from cm3d_amd import rle as rlemod
    c = rlemod.string_to_counts(rle["counts"]).astype(np.int64)         # 0-run, 1-run, 0-run, ...
    ones = np.arange(1, c.size, 2)
    cut = int(ones[ones.size // 2])
    rest = int(c[cut + 1:].sum())
    out = np.concatenate([c[:cut + 1], [rest]]) if rest else c[:cut + 1]
    assert out.sum() == c.sum()
    return {"size": list(rle["size"]), "counts": rlemod.counts_to_string(out.astype(np.uint32))}


def _scenario_frames():
    """Three frames: one of 70 masks (the LDS route of the NMS), two of a handful; all ten classes."""
    from cm3d_amd import synthetic as syn
    from cm3d_amd.lifting import ClassTable
    names = ClassTable.nuscenes().names
    frames = [syn.make_frame(syn.config("tiny", n_masks=70, seed=777), 0), syn.make_frame(syn.config("tiny", seed=778), 1),
              syn.make_frame(syn.config("tiny", n_masks=6, seed=779), 2)]
    for fr in frames:
        fr.labels = [names[(3 * k + 1) % len(names)] for k in range(len(fr.labels))]
    return frames


def _lanes_for(frames, extra=()):
    from cm3d_amd import synthetic as syn
    lanes = [syn.make_lane_table(fr.ego_xyz[:2], 1500, seed=30 + k, extent=60.0) for k, fr in enumerate(frames)]
    if len(extra):
        lanes[0] = np.concatenate([lanes[0], np.asarray(extra, np.float64).reshape(-1, 3)], 0)
    return lanes


def build_scenario(run_plain):
    """run_plain(frames, lanes, frame_lane) -> (HostBatch, results of a plain pass: hit_off, medoid_pos, centroid, lane_dist, box,
    flags).  Returns (frames, lanes, frame_lane, polygon tables, plain results of the final frames, pairs): the masks of frame 0 with
    the most points get a second detection each -- half the mask, labelled car like the whole one, with the higher score -- and a lane
    point next to them; every table gets the synthetic map's square with its hole, plus small square holes around the half masks'
    medoids (so the high-score cars are off the road, the whole masks' beside them on it) and around every fifth other medoid."""
    frames = _scenario_frames()
    frame_lane = [0, 1, 2]
    hb, res = run_plain(frames, _lanes_for(frames), frame_lane)
    n0 = int(hb.mask_off[1])
    top = [int(k) for k in np.argsort(-np.diff(res["hit_off"])[:n0], kind="stable")[:6]]
    f0 = frames[0]
    for rank, k in enumerate(top):
        f0.rles.append(_half_mask(f0.rles[k]))
        f0.labels[k] = "car"
        f0.labels.append("car")
        f0.scores[k] = 0.5 + 0.01 * rank
        f0.scores.append(0.99 - 0.01 * rank)
        f0.cam_nums.append(f0.cam_nums[k])
    extra = [(res["centroid"][k, 0] + 0.5, res["centroid"][k, 1] - 0.25, 0.3) for k in top]
    lanes = _lanes_for(frames, extra)
    hb, res = run_plain(frames, lanes, frame_lane)
    cg = res["centroid"].astype(np.float64)
    has = res["medoid_pos"] >= 0
    tables, pairs = [], []
    for t, fr in enumerate(frames):
        cx, cy = float(fr.ego_xyz[0]), float(fr.ego_xyz[1])
        holes = [dc._rect(cx + 20, cy + 20, cx + 44, cy + 44)]
        m0, m1 = int(hb.mask_off[t]), int(hb.mask_off[t + 1])
        if t == 0:
            for rank, k in enumerate(top):
                j = n0 + rank
                d = np.abs(cg[k, :2] - cg[j, :2]).max()
                if has[k] and has[j] and d > 0:
                    h = 0.45 * d
                    holes.append(dc._rect(cg[j, 0] - h, cg[j, 1] - h, cg[j, 0] + h, cg[j, 1] + h))
                    pairs.append((k, j))
        for m in range(m0, m1, 5):
            if has[m] and not any(m in p for p in pairs):
                holes.append(dc._rect(cg[m, 0] - 0.05, cg[m, 1] - 0.05, cg[m, 0] + 0.05, cg[m, 1] + 0.05))
        tables.append([(dc._rect(cx - 80, cy - 80, cx + 80, cy + 80), holes)])
    return frames, lanes, frame_lane, tables, hb, res, pairs


def check_scenario(hb, plain, pairs, exp):
    """The scenario holds what the test is about (also run on the host against the oracle alone:
    tests/test_optin_pass_cases_host.py)."""
    from cm3d_amd.lifting import ClassTable
    names = ClassTable.nuscenes().names
    n_per = np.diff(hb.mask_off)
    assert 64 < n_per[0] <= 96 and n_per[1] <= 10 and n_per[2] <= 10
    assert set(hb.class_id.tolist()) == set(range(len(names)))
    assert (plain["medoid_pos"] < 0).any() and (plain["medoid_pos"] >= 0).sum() > 30
    # a pair: the half mask (higher score, off the road) suppresses the whole mask in the plain pass; filtered, the whole mask survives
    good = [(k, j) for k, j in pairs if plain["flags"][j] == 3 and plain["flags"][k] == 1 and exp["on_road"][k] == 1 and exp["on_road"][j] == 0
            and exp["medoid_pos_kept"][k] >= 0 and exp["flags"][k] == 3 and exp["flags"][j] == 0]
    assert good, pairs
    dropped = (plain["medoid_pos"] >= 0) & (exp["medoid_pos_kept"] < 0)
    assert dropped.sum() >= 5 and ((plain["medoid_pos"] >= 0) & ~dropped).sum() >= 10
    return good


def _engine_run(eng, hb):
    import torch
    eng.upload(hb)
    eng.run(masks="rle")
    torch.cuda.synchronize()
    return eng.download(full=True)


def _gpu_plain(frames, lanes, frame_lane):
    from cm3d_amd import lifting
    hb = lifting.pack_frames(frames, lanes, frame_lane)
    return hb, _engine_run(lifting.LiftEngine("cuda:0"), hb)


FILTERS = [dict(drivable=True, lane_max_dist=20.0, vehicle_lane_max_dist=4.0), dict(drivable=True),
           dict(lane_max_dist=15.0), dict(vehicle_lane_max_dist=2.5)]


@pytest.fixture(scope="module")
def scenario():
    return build_scenario(_gpu_plain)


@pytest.mark.parametrize("kw", FILTERS, ids=["all", "drivable", "lane", "vehicle_lane"])
def test_filtered_pass_equals_the_host_rule_and_the_oracle(oracle, scenario, kw):
    import torch
    from cm3d_amd import lifting
    frames, lanes, frame_lane, tables, hb, plain, pairs = scenario
    filters = lifting.Stage2Filters(**kw)
    hb_f = lifting.pack_frames(frames, lanes, frame_lane)
    hb_f.polygons = tables
    exp = expected_filtered(oracle, hb, plain, lanes, frame_lane, frames, tables, filters)
    if kw == FILTERS[0]:
        check_scenario(hb, plain, pairs, exp)
    eng = lifting.LiftEngine("cuda:0", filters=filters)
    marks = []
    eng.upload(hb_f)
    eng.run(masks="rle", stage_events=marks)
    torch.cuda.synchronize()
    got = eng.download(full=True)
    assert len(marks) == 7 and marks[5].elapsed_time(marks[6]) >= 0.0
    assert got["on_road"].dtype == np.uint8 and np.array_equal(got["on_road"], exp["on_road"])
    assert np.array_equal(got["medoid_pos_kept"], exp["medoid_pos_kept"])
    assert np.array_equal(got["flags"], exp["flags"])
    for key in ("medoid_pos", "centroid", "lane_idx", "lane_dist", "hit_off", "hit_idx"):       # everything in front of the filter is the plain pass
        assert np.array_equal(got[key], plain[key]), key
    box, ebox = got["box"], exp["box"]
    assert np.array_equal(box[:, 5:10], ebox[:, 5:10])
    pushed = lifting.ClassTable.nuscenes().is_vehicle[hb.class_id].astype(bool)
    assert np.array_equal(box[~pushed, 0:5], ebox[~pushed, 0:5])
    assert np.abs(box[:, 0:5] - ebox[:, 0:5]).max() < BOX_TIGHT
    kept = exp["medoid_pos_kept"] >= 0
    assert np.array_equal(box[kept, 0:9], plain["box"][kept, 0:9])                 # a kept mask's box: the plain pass's bytes
    assert np.array_equal(box[~kept, 0:5], ebox[~kept, 0:5]) and np.array_equal(box[~kept, 0:5], np.tile([0.0, 0, 0, 1, 0], ((~kept).sum(), 1)))
    # a second pass over the resident batch, and the same batch through a pipeline slot (rerun takes its Python branch)
    eng.run(masks="rle")
    torch.cuda.synchronize()
    again = eng.download(full=True)
    assert all(np.array_equal(again[k], got[k]) for k in got)
    if kw == FILTERS[0]:
        pipe = lifting.LiftPipeline("cuda:0", depth=2, filters=filters)
        slot = pipe.submit(hb_f, "rle")
        pipe.rerun(slot)
        _, res = pipe.collect(slot)
        assert all(np.array_equal(res[k], got[k]) for k in got)
        with pytest.raises(ValueError, match="polygon"):
            eng.upload(hb)                      # the drivable filter without polygon tables


def test_engine_without_filters_is_the_plain_pass(oracle, scenario):
    """No filters, or filters with every switch off: the plain pass's calls, buffers and bytes (and they are the oracle's)."""
    from cm3d_amd import lifting
    from tests.helpers import oracle_batch
    from tests.test_gpu_parity import _compare
    frames, lanes, frame_lane, tables, hb, plain, pairs = scenario
    off = lifting.LiftEngine("cuda:0", filters=lifting.Stage2Filters())
    assert off.filters is None and off.needs_road is None
    hb2 = lifting.pack_frames(frames, lanes, frame_lane)
    hb2.polygons = tables                        # polygons on the batch change nothing without the switch
    got = _engine_run(off, hb2)
    assert set(got) == set(plain) and "on_road" not in got and not hasattr(off.b, "medoid_pos_kept")
    for k in plain:
        assert got[k].dtype == plain[k].dtype and got[k].tobytes() == plain[k].tobytes(), k
    _compare(hb, plain, oracle_batch(oracle, frames, lanes, frame_lane, hb))


# ------------------------------------------------------------------------------------------------ entry points
def _nusc_dataset(tmp_path):
    from cm3d_amd import nusc_io, synthetic as syn
    cfg = syn.config("tiny", n_masks=16)
    dataroot, mask_dir, names = nusc_io.write_synthetic_dataset(str(tmp_path), cfg, n_scenes=2, frames_per_scene=2)
    return cfg, dataroot, mask_dir, names


def test_nuscenes_entry_point_with_filters(tmp_path, oracle):
    """--drivable-filter --lane-max-dist 20 --vehicle-lane-max-dist 4 on the synthetic dataset, both host routes: the JSON equals the
    host restatement applied to an unfiltered pass (download(full=True)) over the same files."""
    from cm3d_amd import drivable, eval_detection as ev, lifting, nusc_io
    cfg, dataroot, mask_dir, names = _nusc_dataset(tmp_path)
    env = dict(os.environ, CM3D_VER_NAME="v1.0-synth", CM3D_INPUT_PATH=dataroot, CM3D_INPUT_DIR=mask_dir)
    flags = ["--drivable-filter", "--lane-max-dist", "20", "--vehicle-lane-max-dist", "4"]
    outs = {}
    for route, extra in (("native", []), ("python", ["--reader-threads", "-1"]), ("plain", None)):
        r = subprocess.run([sys.executable, "2d_to_3d.py", "--ratio", str(cfg.ratio)] + (flags + extra if extra is not None else []),
                           cwd=os.path.join(ROOT, "src", "nuscenes"), env=dict(env, CM3D_OUTPUT_DIR=str(tmp_path / route)),
                           capture_output=True, text=True, timeout=600)
        assert r.returncode == 0, r.stderr[-2000:]
        outs[route] = json.load(open(tmp_path / route / "pseudolabels_minival.json"))
        if extra is not None:
            line = [l for l in r.stdout.splitlines() if l.startswith("drivable :")]
            assert line and float(line[0].split()[-1]) > 0.0              # the reference's timer bucket is filled
    assert outs["native"] == outs["python"]
    # the restatement: an unfiltered pass per scene, the rule, the NMS of the kept boxes
    tables = nusc_io.NuscTables("v1.0-synth", dataroot)
    classes = lifting.ClassTable.nuscenes()
    filters = lifting.Stage2Filters(True, 20.0, 4.0)
    eng = lifting.LiftEngine("cuda:0")
    want, n_dropped = {}, 0
    for name in names:
        scene = tables.scene_by_name(name)
        frames = nusc_io.frames_of_scene(tables, scene, mask_dir, n_sweeps=3, ratio=cfg.ratio)
        lanes = [nusc_io.load_lane_points(dataroot, tables.location(scene))]
        polys = [ev.load_drivable_polygons(dataroot, tables.location(scene))]
        hb = lifting.pack_frames(frames, lanes, [0] * len(frames))
        plain = _engine_run(eng, hb)
        exp = expected_filtered(oracle, hb, plain, lanes, [0] * len(frames), frames, polys, filters)
        res = dict(plain, flags=exp["flags"])                  # a kept mask's box is the plain pass's; the flags are the restatement's
        want.update(lifting.box_records(hb, res, classes))
        n_dropped += int(((plain["medoid_pos"] >= 0) & (exp["medoid_pos_kept"] < 0)).sum())
    assert n_dropped >= 3
    assert outs["native"]["results"] == want
    assert outs["plain"]["results"] != want and sum(map(len, want.values())) > 5


def test_waymo_entry_point_has_the_lane_flags_only(tmp_path):
    """src/waymo/2d_to_3d.py: --drivable-filter is an argparse error; the lane flags give the file an engine with those filters gives,
    whose kept positions are the host rule's on its own lane distances; thresholds at inf change no byte."""
    from tests.test_gpu_entrypoint import _write_waymo_scene
    from cm3d_amd import drivable, lifting, pipeline_waymo as pw, waymo as wm
    scene = "segment-synthetic-0"
    _write_waymo_scene(tmp_path, scene, 0, 4)
    cwd = os.path.join(ROOT, "src", "waymo")
    args = ["--frames-dir", str(tmp_path / "frames"), "--mask-dir", str(tmp_path / "masks")]
    r = subprocess.run([sys.executable, "2d_to_3d.py", *args, "--drivable-filter"], cwd=cwd, capture_output=True, text=True, timeout=600)
    assert r.returncode == 2 and "unrecognized arguments: --drivable-filter" in r.stderr
    blobs = {}
    for key, extra in (("plain", []), ("off", ["--lane-max-dist", "inf"]), ("lane", ["--lane-max-dist", "160", "--vehicle-lane-max-dist", "100"])):
        r = subprocess.run([sys.executable, "2d_to_3d.py", *args, "--output", str(tmp_path / f"{key}.bin"), *extra], cwd=cwd,
                           capture_output=True, text=True, timeout=600)
        assert r.returncode == 0, r.stderr[-2000:]
        blobs[key] = open(tmp_path / f"{key}.bin", "rb").read()
    assert blobs["off"] == blobs["plain"] and blobs["lane"] != blobs["plain"]
    frames, lanes = pw.load_scene(str(tmp_path / "frames"), str(tmp_path / "masks"), scene)
    classes = lifting.ClassTable.waymo()
    hb = lifting.pack_frames(frames, [lanes], [0] * len(frames), classes)
    got = _engine_run(lifting.LiftEngine("cuda:0", classes=classes, filters=lifting.Stage2Filters(False, 160.0, 100.0)), hb)
    kept = drivable.filter_rule(got["medoid_pos"], hb.class_id, got["lane_dist"], None, classes.is_vehicle, classes.needs_road, 160.0, 100.0)
    assert np.array_equal(got["medoid_pos_kept"], kept) and not got["on_road"].any()
    # (the scene's lane distances are 4.7 and 63.9 m for two vehicles, 162.9 m for a pedestrian, 153.7 m for a vehicle: one mask
    # goes by each threshold)
    has, veh = got["medoid_pos"] >= 0, classes.is_vehicle[hb.class_id].astype(bool)
    assert (has & (kept < 0) & veh).any() and (has & (kept < 0) & ~veh).any() and (kept >= 0).sum() >= 2
    assert np.array_equal(got["flags"] & 1, (kept >= 0).astype(np.int32))
    objs = wm.objects_from_results(hb, got, classes, [(f.context_name, f.timestamp_micros) for f in frames])
    assert blobs["lane"] == wm.encode_objects(objs) and 0 < len(objs) < len(wm.decode_objects(blobs["plain"]))


def test_eval_custom_device_drivable_filter_equals_host(tmp_path):
    """eval_custom.py --drivable_filtering 1: --metrics device (one cm3d_points_in_polygons call per box set) writes the summary
    --metrics host writes, apart from the time field, and prints the same counts."""
    cfg, dataroot, mask_dir, names = _nusc_dataset(tmp_path)
    env = dict(os.environ, CM3D_VER_NAME="v1.0-synth", CM3D_INPUT_PATH=dataroot, CM3D_INPUT_DIR=mask_dir, CM3D_OUTPUT_DIR=str(tmp_path / "out"))
    cwd = os.path.join(ROOT, "src", "nuscenes")
    r = subprocess.run([sys.executable, "2d_to_3d.py", "--ratio", str(cfg.ratio)], cwd=cwd, env=env, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-2000:]
    summaries, counts = {}, {}
    for where in ("host", "device"):
        r = subprocess.run([sys.executable, "eval_custom.py", str(tmp_path / "out" / "pseudolabels_minival.json"), "--output_dir",
                            str(tmp_path / where), "--dataroot", dataroot, "--version", "v1.0-synth", "--object_only", "1",
                            "--drivable_filtering", "1", "--metrics", where], cwd=cwd, capture_output=True, text=True, timeout=300)
        assert r.returncode == 0, r.stderr[-2000:]
        summaries[where] = json.load(open(tmp_path / where / "metrics_summary.json"))
        counts[where] = [l for l in r.stdout.splitlines() if l.startswith("> ")]
        summaries[where].pop("eval_time")
    assert counts["host"] == counts["device"] and sum("drivable area" in l for l in counts["host"]) == 2
    before, after = (int(counts["host"][k].rsplit(" ", 1)[1]) for k in (3, 4))          # predictions: after bike racks, after the drivable filter
    assert 0 < after < before
    assert json.dumps(summaries["host"], sort_keys=True) == json.dumps(summaries["device"], sort_keys=True)
