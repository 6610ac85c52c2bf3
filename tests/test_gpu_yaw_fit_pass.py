"""GPU: LiftEngine(yaw=YawFit(...)) -- the yaw-fitted pass alone, behind the clustered and the filtered pass and in front of the rotated
NMS -- against the composed CPU expectation of tests/yaw_fit_pass_cases.py (nothing in it comes from the device), on a two-frame
nuScenes batch and a two-frame Waymo batch that each hold a car standing across the lanes; that nothing moves without the option; and
src/nuscenes/2d_to_3d.py --yaw fit on a scene with such a car."""
import json
import math
import os
import pickle
import subprocess
import sys

import numpy as np
import pytest

from cm3d_amd import bevfit
from cm3d_amd import cluster as clustermod
from cm3d_amd import nms as nmsmod
from tests import bev_fit_cases as fc
from tests import optin_pass_cases as oc
from tests import yaw_fit_pass_cases as yc
from tests.test_gpu_optin_passes import _check_nms, _check_pass, _poison, _run, _same_bytes, _sync_download

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
Y = bevfit.YawFit()


def _engine(b, **kw):
    from cm3d_amd import lifting
    return lifting.LiftEngine("cuda:0", classes=b.classes, **kw)


def _check_fitted(b, got, exp, front):
    """got: a downloaded yaw-fitted pass; exp: yaw_fit_pass_cases.fitted of `front`, the expectation of the pass in front of the fit."""
    _check_pass(b.hb, got, exp)                    # lists, medoids, lane results, filter outputs, flags; box within test_gpu_parity's tolerance
    for key in ("yaw_src", "fit_status", "fit_k"):
        assert got[key].dtype == np.int32 and np.array_equal(got[key], exp[key]), key
    assert np.array_equal(got["fit_rect"].view(np.uint64), exp["fit_rect"].view(np.uint64))
    # column 5 holds the yaw that was used: the lane's to the bit, the fitted one within one float32 ulp at pi
    lane = exp["yaw_src"] == 0
    assert np.array_equal(got["box"][lane, 5], exp["box"][lane, 5])
    assert np.abs(got["box"][~lane, 5] - exp["box"][~lane, 5]).max() <= 2.0 ** -22
    return lane


@pytest.mark.parametrize("name", ["nusc", "waymo"])
def test_yaw_fitted_pass_equals_the_composed_oracle(oracle, name):
    b = yc.batch(name)
    front = yc.plain(oracle, name)
    exp = yc.fitted(oracle, b, front, Y)
    assert 30 <= b.hb.n_masks <= 60 and set(exp["yaw_src"]) == {0, 1} and {0, 1, 2} <= set(exp["fit_status"])
    eng = _engine(b, yaw=Y)
    got = _run(eng, b.hb)
    lane = _check_fitted(b, got, exp, front)
    # every mask that kept the lane's yaw has the plain pass's record byte for byte (column 9, the NMS's verdict, depends on the others)
    base = _run(_engine(b), b.hb)
    _check_pass(b.hb, base, front)
    assert got["box"][lane, :9].tobytes() == base["box"][lane, :9].tobytes()
    for key in base:
        if key not in ("box", "flags"):
            assert got[key].tobytes() == base[key].tobytes(), key
    # the car across the lanes: fitted, its yaw the true heading's axis within the derived bound, the lane's more than 45 degrees off
    for m, heading in zip(b.l_masks, b.l_heading):
        assert got["yaw_src"][m] == 1 and got["fit_status"][m] == 0 and got["flags"][m] & 1
        ax = lambda a: abs((a - heading + math.pi / 2) % math.pi - math.pi / 2)
        assert ax(got["box"][m, 5]) <= fc.known_answer_bound(Y.angles, yc.CAR_L, Y.d0)
        assert ax(base["box"][m, 5]) > math.pi / 4
    # a second pass over the resident batch rewrites everything; a captured graph of the fitted pass gives the same bytes
    import torch
    _poison(eng)
    for k in ("fit_k", "fit_status", "yaw_src", "yaw_idx"):
        getattr(eng.b, k).fill_(-3)
    eng.b.fit_rect.fill_(-3.0); eng.b.yaw_tab.fill_(-3.0)
    _same_bytes(_run(eng), got)
    g = eng.capture_graph(masks="rle")
    _poison(eng)
    eng.b.fit_rect.fill_(-3.0); eng.b.yaw_src.fill_(-3)
    g.replay()
    torch.cuda.synchronize()
    _same_bytes(eng.download(full=True), got)


@pytest.mark.parametrize("name", ["nusc", "waymo"])
def test_yaw_fit_behind_the_clustered_pass(oracle, name):
    """The fit sees the cl_* lists."""
    b = yc.batch(name)
    c = clustermod.DepthCluster(1.0, 20)
    front = yc.expected_of(oracle, name, cluster=c)
    exp = yc.fitted(oracle, b, front, Y)
    plain_fit = yc.fitted(oracle, b, yc.plain(oracle, name), Y)
    assert not np.array_equal(exp["fit_rect"], plain_fit["fit_rect"])             # the clustering changes what is fitted
    got = _run(_engine(b, yaw=Y, cluster=c), b.hb)
    _check_fitted(b, got, exp, front)


@pytest.mark.parametrize("name", ["nusc", "waymo"])
def test_yaw_fit_behind_the_filtered_pass(oracle, name):
    """The masks the filter dropped get no box and no fitted yaw: medoid_pos_kept decides."""
    b = yc.batch(name)
    f = oc.lane_filters(yc.plain(oracle, name))
    front = yc.expected_of(oracle, name, filters=f)
    exp = yc.fitted(oracle, b, front, Y)
    dropped = (front["medoid_pos"] >= 0) & (front["medoid_pos_kept"] < 0)
    assert dropped.sum() >= 3 and not exp["yaw_src"][dropped].any() and exp["yaw_src"].any()
    got = _run(_engine(b, yaw=Y, filters=f), b.hb)
    _check_fitted(b, got, exp, front)


def test_yaw_fit_in_front_of_the_rotated_nms(oracle):
    """The rotated NMS stays last and judges the fitted boxes."""
    b = yc.batch("nusc")
    r = nmsmod.RotatedNms(class_agnostic=True)
    base = _run(_engine(b, yaw=Y), b.hb)
    _check_fitted(b, base, yc.fitted(oracle, b, yc.plain(oracle, "nusc"), Y), None)
    both = _run(_engine(b, yaw=Y, nms=r), b.hb)
    took, keep = _check_nms(b.hb, both, base, r)
    assert took.sum() >= 10
    lane_only = _run(_engine(b, nms=r), b.hb)
    assert lane_only["box"][:, :9].tobytes() != both["box"][:, :9].tobytes()


def _all_four(oracle, name):
    """The batch, the four options and the CPU expectation of the pass with the first three (the rotated NMS judges what they wrote)."""
    b = yc.batch(name)
    c = clustermod.DepthCluster(1.0, 20)
    f = oc.lane_filters(yc.expected_of(oracle, name, cluster=c))
    front = yc.expected_of(oracle, name, cluster=c, filters=f)
    return b, c, f, nmsmod.RotatedNms(class_agnostic=True), front, yc.fitted(oracle, b, front, Y)


def _check_verdict_only(both, base):
    """both: the pass with the rotated NMS, base: the same pass without.  Only bit 1 of flags and column 9 of box may differ."""
    assert set(both) == set(base)
    for key in base:
        if key not in ("box", "flags"):
            assert both[key].dtype == base[key].dtype and both[key].tobytes() == base[key].tobytes(), key
    assert both["box"][:, :9].tobytes() == base["box"][:, :9].tobytes() and np.array_equal(both["flags"] & 1, base["flags"] & 1)
    assert np.array_equal(both["box"][:, 9], both["flags"].astype(np.float64)) and set(np.unique(both["flags"]).tolist()) <= {0, 1, 3}


@pytest.mark.parametrize("name", ["nusc", "waymo"])
def test_all_four_options_in_one_pass(oracle, name):
    """Clustering, filters, yaw fit and rotated NMS together: one cm3d_lift_pass_opt call.  The fit sees the clustered lists and the
    kept positions, the rotated NMS the fitted boxes."""
    b, c, f, r, front, exp = _all_four(oracle, name)
    dropped = (front["medoid_pos"] >= 0) & (front["medoid_pos_kept"] < 0)
    assert dropped.sum() >= 3 and not exp["yaw_src"][dropped].any() and exp["yaw_src"].any()
    assert not np.array_equal(exp["fit_rect"], yc.fitted(oracle, b, yc.plain(oracle, name), Y)["fit_rect"])
    if name == "nusc":
        cpu_keep = oc.rotated_keep(exp["box"], exp["flags"], b.hb, r, b.classes)
        assert (((exp["flags"] & 1) == 1) & (cpu_keep == 0)).sum() >= 1
    three = _run(_engine(b, cluster=c, filters=f, yaw=Y), b.hb)
    _check_fitted(b, three, exp, front)
    eng = _engine(b, cluster=c, filters=f, yaw=Y, nms=r)
    got = _run(eng, b.hb)
    if name == "nusc":
        took, keep = _check_nms(b.hb, got, three, r)
        assert (took & (keep == 0)).sum() >= 1
    else:                          # (the host statement of the decision reads nuScenes records: tests/test_gpu_rotated_nms.py has Waymo's)
        _check_verdict_only(got, three)

    def poison():
        _poison(eng)
        for k in ("fit_k", "fit_status", "yaw_src", "yaw_idx", "medoid_pos_kept"):
            getattr(eng.b, k).fill_(-3)
        eng.b.fit_rect.fill_(-3.0); eng.b.yaw_tab.fill_(-3.0); eng.b.on_road.fill_(7)
    poison()
    _same_bytes(_run(eng), got)
    g = eng.capture_graph(masks="rle")
    poison()
    g.replay()
    _same_bytes(_sync_download(eng), got)


def test_pipeline_with_all_four_options_times_every_stage_and_reruns(oracle):
    """submit(stage_events=) hands back the five events of the plain pass and a pair per opt-in stage, each where the header puts its
    stage; a rerun gives the first pass's bytes and records into none of those events."""
    import torch
    from cm3d_amd import lifting
    b, c, f, r, _, _ = _all_four(oracle, "nusc")
    pipe = lifting.LiftPipeline("cuda:0", depth=2, classes=b.classes, cluster=c, filters=f, yaw=Y, nms=r)
    ev = []
    slot = pipe.submit(b.hb, "rle", stage_events=ev)
    assert len(ev) == 11
    first = pipe.collect(slot)[1]
    torch.cuda.synchronize()
    five, (f0, f1), (c0, c1), (y0, y1) = ev[:5], ev[5:7], ev[7:9], ev[9:11]
    order = [five[0], five[1], c0, c1, five[2], five[3], five[4], f0, f1, y0, y1]
    before = [a.elapsed_time(z) for a, z in zip(order, order[1:])]
    assert min(before) >= 0.0
    eng = pipe.engines[slot]
    _poison(eng)
    for k in ("fit_k", "fit_status", "yaw_src", "medoid_pos_kept"):
        getattr(eng.b, k).fill_(-3)
    torch.cuda.synchronize()                       # (the fills ran on another stream than the pass will)
    pipe.rerun(slot)
    again = pipe.collect(slot)[1]
    torch.cuda.synchronize()
    _same_bytes(first, again)
    assert [a.elapsed_time(z) for a, z in zip(order, order[1:])] == before


@pytest.mark.parametrize("name", ["nusc", "waymo"])
def test_off_by_default(oracle, name):
    """LiftEngine(yaw=None) leaves every buffer of the plain pass byte-identical to an engine built without the argument, and
    allocates nothing for the fit."""
    b = yc.batch(name)
    without, off = _engine(b), _engine(b, yaw=None)
    a, c = _run(without, b.hb), _run(off, b.hb)
    _same_bytes(a, c)
    assert "yaw_src" not in c and off.yaw is None
    for attr in ("fit_k", "fit_rect", "fit_status", "yaw_tab", "yaw_idx", "yaw_src", "yaw_desc"):
        assert not hasattr(off.b, attr), attr
    on = _engine(b, yaw=Y)
    _run(on, b.hb)
    assert all(hasattr(on.b, attr) for attr in ("fit_rect", "yaw_tab", "yaw_desc"))


def test_pipeline_rerun_takes_the_python_branch(oracle):
    """cm3d_pipe_submit knows only the plain pass: a LiftPipeline whose engines fit yaws reruns through LiftEngine.run."""
    import torch
    from cm3d_amd import lifting
    b = yc.batch("nusc")
    exp = yc.fitted(oracle, b, yc.plain(oracle, "nusc"), Y)
    pipe = lifting.LiftPipeline("cuda:0", depth=2, classes=b.classes, yaw=Y)
    slot = pipe.submit(b.hb, "rle")
    first = pipe.collect(slot)[1]
    pipe.engines[slot].b.box.fill_(-3.0)
    pipe.engines[slot].b.yaw_src.fill_(-3)
    torch.cuda.synchronize()                       # (the fills ran on another stream than the pass will)
    pipe.rerun(slot)
    again = pipe.collect(slot)[1]
    torch.cuda.synchronize()
    _same_bytes(first, again)
    assert np.array_equal(again["yaw_src"], exp["yaw_src"]) and np.array_equal(again["flags"], exp["flags"])


# ------------------------------------------------------------------------------------------------ the entry point
def _scene_with_l_vehicle(tmp_path):
    """One synthetic nuScenes scene of one frame on disk, then the frame read back, given the car across the lanes and written again:
    sweeps, masks, detections, and a lane file of parallel lanes.  Returns (cfg, dataroot, mask_dir, the car's heading)."""
    from cm3d_amd import nusc_io, synthetic as syn
    cfg = syn.config("tiny", n_points=9000, n_masks=12, width=512, height=288, ratio=0.32, max_area=12000.0)
    dataroot, mask_dir, names = nusc_io.write_synthetic_dataset(str(tmp_path), cfg, n_scenes=1, frames_per_scene=1)
    tables = nusc_io.NuscTables("v1.0-synth", dataroot)
    scene = tables.scene_by_name(names[0])
    fr = nusc_io.frames_of_scene(tables, scene, mask_dir, n_sweeps=cfg.n_sweeps, ratio=cfg.ratio)[0]
    fr.sweeps_raw = [np.array(r) for r in fr.sweeps_raw]
    fr.rles, fr.labels, fr.scores, fr.cam_nums = list(fr.rles), list(fr.labels), list(fr.scores), list(fr.cam_nums)
    heading = yc.add_l_vehicle(fr, yc.LANE_YAW["nusc"])
    for k, raw in enumerate(fr.sweeps_raw):
        assert raw.shape[1] == 5
        raw.astype(np.float32).tofile(os.path.join(dataroot, "sweeps", "LIDAR_TOP", f"{names[0]}_0_{k}.bin"))
    with open(os.path.join(mask_dir, names[0], "0_masks.pkl"), "rb") as fh:
        rles = list(pickle.load(fh))
    with open(os.path.join(mask_dir, names[0], "0_masks.pkl"), "wb") as fh:
        pickle.dump(rles + [fr.rles[-1]], fh)
    with open(os.path.join(mask_dir, names[0], "0_data.json")) as fh:
        data = json.load(fh)
    data["labels"].append("car"); data["detection_scores"].append(0.987); data["cam_nums"].append(int(fr.cam_nums[-1]))   # (no other detection has this score)
    with open(os.path.join(mask_dir, names[0], "0_data.json"), "w") as fh:
        json.dump(data, fh)
    np.save(os.path.join(dataroot, "lanes", tables.location(scene) + ".npy"), yc.parallel_lanes(fr.ego_xyz[:2], yc.LANE_YAW["nusc"]))
    return cfg, dataroot, mask_dir, heading


def test_nuscenes_entry_point(tmp_path):
    """src/nuscenes/2d_to_3d.py --yaw fit, both host routes: the rotation the JSON holds for the car across the lanes is its true heading's
    axis within the derived bound and more than 45 degrees from what the run without the flag wrote; --yaw lane writes the bytes of no flag."""
    cfg, dataroot, mask_dir, heading = _scene_with_l_vehicle(tmp_path)
    env = dict(os.environ, CM3D_VER_NAME="v1.0-synth", CM3D_INPUT_PATH=dataroot, CM3D_INPUT_DIR=mask_dir)
    blobs = {}
    for route, extra in (("plain", []), ("lane", ["--yaw", "lane", "--yaw-fit-angles", "64", "--yaw-fit-d0", "0.5"]), ("native", ["--yaw", "fit"]),
                         ("python", ["--yaw", "fit", "--reader-threads", "-1"])):
        p = subprocess.run([sys.executable, "2d_to_3d.py", "--ratio", str(cfg.ratio), "--n-sweeps", str(cfg.n_sweeps)] + extra,
                           cwd=os.path.join(ROOT, "src", "nuscenes"), env=dict(env, CM3D_OUTPUT_DIR=str(tmp_path / route)), capture_output=True,
                           text=True, timeout=600)
        assert p.returncode == 0, p.stderr[-2000:]
        blobs[route] = open(tmp_path / route / "pseudolabels_minival.json", "rb").read()
    assert blobs["lane"] == blobs["plain"] and blobs["native"] != blobs["plain"]
    assert json.loads(blobs["native"]) == json.loads(blobs["python"])

    def car_yaw(blob):
        boxes = [bx for v in json.loads(blob)["results"].values() for bx in v if bx["detection_score"] == 0.987]
        assert len(boxes) == 1 and boxes[0]["detection_name"] == "car"
        q = boxes[0]["rotation"]
        return 2.0 * math.atan2(q[3], q[0])
    ax = lambda a: abs((a - heading + math.pi / 2) % math.pi - math.pi / 2)
    fit, lane = car_yaw(blobs["native"]), car_yaw(blobs["plain"])
    print(f"car across the lanes: heading {heading:.4f}, --yaw fit {fit:.4f} ({ax(fit):.4f} off the axis), no flag {lane:.4f} ({ax(lane):.4f} off)")
    assert ax(fit) <= fc.known_answer_bound(128, yc.CAR_L, 0.05)
    assert abs((fit - lane + math.pi) % (2 * math.pi) - math.pi) > math.pi / 4 and ax(lane) > math.pi / 4


def test_waymo_entry_point(tmp_path):
    """src/waymo/2d_to_3d.py --yaw fit: the file is the one an engine with the fit gives; --yaw lane writes the bytes of no flag.  (The
    scene's lists are a few points long: 2 points and no least length let one of its vehicles take the fit.)"""
    from tests.test_gpu_entrypoint import _write_waymo_scene
    from cm3d_amd import lifting, pipeline_waymo as pw, waymo as wm
    scene = "segment-synthetic-0"
    _write_waymo_scene(tmp_path, scene, 0, 3)
    cwd = os.path.join(ROOT, "src", "waymo")
    args = ["--frames-dir", str(tmp_path / "frames"), "--mask-dir", str(tmp_path / "masks")]
    blobs = {}
    for key, extra in (("plain", []), ("lane", ["--yaw", "lane", "--yaw-fit-min-points", "2"]),
                       ("fit", ["--yaw", "fit", "--yaw-fit-min-points", "2", "--yaw-fit-min-length", "0"])):
        p = subprocess.run([sys.executable, "2d_to_3d.py", *args, "--output", str(tmp_path / f"{key}.bin"), *extra], cwd=cwd,
                           capture_output=True, text=True, timeout=600)
        assert p.returncode == 0, p.stderr[-2000:]
        blobs[key] = open(tmp_path / f"{key}.bin", "rb").read()
    assert blobs["lane"] == blobs["plain"] and blobs["fit"] != blobs["plain"]
    frames, lanes = pw.load_scene(str(tmp_path / "frames"), str(tmp_path / "masks"), scene)
    classes = lifting.ClassTable.waymo()
    hb = lifting.pack_frames(frames, [lanes], [0] * len(frames), classes)
    got = _run(lifting.LiftEngine("cuda:0", classes=classes, yaw=bevfit.YawFit(min_points=2, min_length=0.0)), hb)
    assert got["yaw_src"].sum() >= 1
    objs = wm.objects_from_results(hb, got, classes, [(f.context_name, f.timestamp_micros) for f in frames])
    assert blobs["fit"] == wm.encode_objects(objs) and len(objs) >= 2
