"""GPU: LiftEngine(yaw=YawFit(), place=BoxPlace()) -- the placed pass alone, behind the clustered and the filtered pass, in front of the
rotated NMS and of the velocity stage, through a captured graph and through LiftPipeline.rerun -- on the two-frame batches of
tests/yaw_fit_pass_cases.py, whose last mask per frame is a car of two faces.  The expectation is composed on the CPU and takes nothing
from the device: yaw_fit_pass_cases.fitted followed by boxplace.box_place_host.  That nothing moves without the option; and the nuScenes
and Waymo entry points with --place fit."""
import json
import math
import os
import subprocess
import sys

import numpy as np
import pytest

from cm3d_amd import bevfit, boxplace
from cm3d_amd import cluster as clustermod
from cm3d_amd import nms as nmsmod
from tests import bev_fit_cases as fc
from tests import optin_pass_cases as oc
from tests import yaw_fit_pass_cases as yc
from tests.test_gpu_optin_passes import _check_nms, _poison, _run, _same_bytes
from tests.test_gpu_yaw_fit_pass import _check_fitted, _engine, _scene_with_l_vehicle

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
Y = bevfit.YawFit()
P = boxplace.BoxPlace()
PLACE_KEYS = ("place_src", "place_pushed")


def placed(b, exp, p=P):
    """exp (yaw_fit_pass_cases.fitted) with the box, flags, place_src and place_pushed of the placed pass: box_place_host on the
    composed rows, with the engine's launch bound (32 masks per plane of hit words)."""
    hb = b.hb
    planes = (int(np.diff(hb.mask_off).max()) + 31) // 32
    r = boxplace.box_place_host(exp["box"], exp["flags"], hb.mask_off, exp["fit_rect"], exp["yaw_src"], b.classes.prior_wlh, b.classes.nms_group,
                                b.classes.nms_thr, None if hb.pose_rt is not None else hb.ego_xyz, p.thin, min(32 * planes, 1024))
    return dict(exp, **r)


def _check_placed(b, got, exp, base):
    """got: a downloaded placed pass; exp: placed(fitted(front)); base: the yaw-fitted pass of the same engine without the placement,
    downloaded (the device's own: what an unplaced mask must keep byte for byte)."""
    _check_fitted(b, got, exp, None)               # flags exact; every column of box under test_gpu_yaw_fit_pass's rules
    assert got["place_src"].dtype == np.int32 and np.array_equal(got["place_src"], exp["place_src"])
    on = exp["place_src"] > 0
    assert got["box"][on, :2].tobytes() == exp["box"][on, :2].tobytes()                  # from fit_rect, which is exact: to the bit
    assert got["box"][~on, :9].tobytes() == base["box"][~on, :9].tobytes() and got["box"][:, 2:9].tobytes() == base["box"][:, 2:9].tobytes()
    assert got["place_pushed"].tobytes() == base["box"][:, :2].tobytes()
    assert np.array_equal(got["box"][:, 9], got["flags"].astype(np.float64)) and np.array_equal(got["flags"] & 1, base["flags"] & 1)
    for key in base:
        if key not in ("box", "flags"):
            assert got[key].tobytes() == base[key].tobytes(), key
    return on


@pytest.mark.parametrize("name", ["nusc", "waymo"])
def test_placed_pass_equals_the_composed_oracle(oracle, name):
    b = yc.batch(name)
    fit = yc.fitted(oracle, b, yc.plain(oracle, name), Y)
    exp = placed(b, fit)
    assert set(exp["place_src"]) >= {0, 1} and np.array_equal(exp["place_src"] > 0, (fit["yaw_src"] == 1) & ((fit["flags"] & 1) == 1))
    base = _run(_engine(b, yaw=Y), b.hb)
    eng = _engine(b, yaw=Y, place=P)
    got = _run(eng, b.hb)
    on = _check_placed(b, got, exp, base)
    moved = np.hypot(*(got["box"][on, :2] - base["box"][on, :2]).T)
    print(f"{name}: {int(on.sum())} of {b.hb.n_masks} masks placed, place_src counts {np.bincount(exp['place_src'], minlength=4).tolist()}, "
          f"moved {moved.min():.3f} .. {moved.max():.3f} m; flags changed on {int((got['flags'] != base['flags']).sum())}")
    assert moved.max() > 0.05
    for m in b.l_masks:                            # the car of two faces: both seen, anchored at the corner
        assert got["place_src"][m] == 1 and got["flags"][m] & 1
    # a second pass over the resident batch rewrites everything; a captured graph of the placed pass gives the same bytes
    import torch

    def poison():
        _poison(eng)
        for k in ("fit_k", "fit_status", "yaw_src", "yaw_idx", "place_src"):
            getattr(eng.b, k).fill_(-3)
        eng.b.fit_rect.fill_(-3.0); eng.b.yaw_tab.fill_(-3.0); eng.b.place_pushed.fill_(-3.0)
    poison()
    _same_bytes(_run(eng), got)
    g = eng.capture_graph(masks="rle")
    poison()
    g.replay()
    torch.cuda.synchronize()
    _same_bytes(eng.download(full=True), got)
    # download(full=False) carries the two arrays too
    assert all(np.array_equal(eng.download(full=False)[k], got[k]) for k in PLACE_KEYS)


@pytest.mark.parametrize("name", ["nusc", "waymo"])
def test_placement_behind_the_clustered_pass(oracle, name):
    b = yc.batch(name)
    c = clustermod.DepthCluster(1.0, 20)
    exp = placed(b, yc.fitted(oracle, b, yc.expected_of(oracle, name, cluster=c), Y))
    assert not np.array_equal(exp["box"][:, :2], placed(b, yc.fitted(oracle, b, yc.plain(oracle, name), Y))["box"][:, :2])
    base = _run(_engine(b, yaw=Y, cluster=c), b.hb)
    assert _check_placed(b, _run(_engine(b, yaw=Y, cluster=c, place=P), b.hb), exp, base).any()


@pytest.mark.parametrize("name", ["nusc", "waymo"])
def test_placement_behind_the_filtered_pass(oracle, name):
    """The masks the filter dropped have no box: they are not placed."""
    b = yc.batch(name)
    f = oc.lane_filters(yc.plain(oracle, name))
    front = yc.expected_of(oracle, name, filters=f)
    exp = placed(b, yc.fitted(oracle, b, front, Y))
    dropped = (front["medoid_pos"] >= 0) & (front["medoid_pos_kept"] < 0)
    assert dropped.sum() >= 3 and not exp["place_src"][dropped].any() and exp["place_src"].any()
    base = _run(_engine(b, yaw=Y, filters=f), b.hb)
    _check_placed(b, _run(_engine(b, yaw=Y, filters=f, place=P), b.hb), exp, base)


def test_placement_in_front_of_the_rotated_nms(oracle):
    """The rotated NMS stays last: it judges the placed boxes and overwrites the circle NMS's second verdict."""
    b = yc.batch("nusc")
    r = nmsmod.RotatedNms(class_agnostic=True)
    base = _run(_engine(b, yaw=Y, place=P), b.hb)
    both = _run(_engine(b, yaw=Y, place=P, nms=r), b.hb)
    took, keep = _check_nms(b.hb, both, base, r)   # everything but the verdict is base's bytes; the verdict is the host's on the placed rows
    assert took.sum() >= 10
    unplaced = _run(_engine(b, yaw=Y, nms=r), b.hb)
    assert unplaced["box"][:, :2].tobytes() != both["box"][:, :2].tobytes()


def test_velocity_stage_sees_the_placed_centres():
    """cm3d_box_velocity stays the caller's call behind the pass: on the moving scenes of tests/velocity_pass_cases.py its outputs are
    the host statement's on the device's own placed rows, to the bit, and the pass's buffers are those of the engine without it."""
    from cm3d_amd import lifting
    from tests import velocity_pass_cases as vc
    from tests.test_gpu_velocity_pass import _assert_statement
    hb, v = vc.batch().hb, vc.settings()[0]
    base = _run(lifting.LiftEngine("cuda:0", yaw=Y, place=P), hb)
    got = _run(lifting.LiftEngine("cuda:0", yaw=Y, place=P, velocity=v), hb)
    for k, a in base.items():
        assert a.tobytes() == got[k].tobytes(), k
    _assert_statement(hb, got)
    unplaced = _run(lifting.LiftEngine("cuda:0", yaw=Y, velocity=v), hb)
    linked = (got["place_src"] > 0) & ((got["flags"] & 3) == 3) & (got["vel_src"] > 0)
    print(f"{int((got['place_src'] > 0).sum())} placed, {int(linked.sum())} of them kept and linked")
    assert linked.sum() >= 1 and (got["box"][linked, :2] != unplaced["box"][linked, :2]).any(1).all()


def test_pipeline_rerun_takes_the_python_branch(oracle):
    """cm3d_pipe_submit knows only the plain pass: a LiftPipeline whose engines place boxes reruns through LiftEngine.run; and
    submit(stage_events=) hands back the placement's pair of events behind the yaw fit's."""
    import torch
    from cm3d_amd import lifting
    b = yc.batch("nusc")
    exp = placed(b, yc.fitted(oracle, b, yc.plain(oracle, "nusc"), Y))
    pipe = lifting.LiftPipeline("cuda:0", depth=2, classes=b.classes, yaw=Y, place=P)
    ev = []
    slot = pipe.submit(b.hb, "rle", stage_events=ev)
    first = pipe.collect(slot)[1]
    torch.cuda.synchronize()
    assert len(ev) == 9 and not pipe.engines[slot].b.plain_pass
    assert min(a.elapsed_time(z) for a, z in zip(ev[4:], ev[5:])) >= 0.0             # boxes, the fit's pair, the placement's pair: in this order
    eng = pipe.engines[slot]
    eng.b.box.fill_(-3.0); eng.b.place_src.fill_(-3); eng.b.place_pushed.fill_(-3.0); eng.b.yaw_src.fill_(-3)
    torch.cuda.synchronize()                       # (the fills ran on another stream than the pass will)
    pipe.rerun(slot)
    again = pipe.collect(slot)[1]
    torch.cuda.synchronize()
    _same_bytes(first, again)
    assert np.array_equal(again["place_src"], exp["place_src"]) and np.array_equal(again["flags"], exp["flags"])
    on = exp["place_src"] > 0
    assert again["box"][on, :2].tobytes() == exp["box"][on, :2].tobytes()


@pytest.mark.parametrize("name", ["nusc", "waymo"])
def test_off_by_default(name):
    """LiftEngine(yaw=..., place=None) leaves every buffer of the yaw-fitted pass byte-identical to an engine built without the argument
    and allocates nothing for the placement; a placement without a yaw fit is refused."""
    from cm3d_amd import lifting
    b = yc.batch(name)
    without, off = _engine(b, yaw=Y), _engine(b, yaw=Y, place=None)
    a, c = _run(without, b.hb), _run(off, b.hb)
    _same_bytes(a, c)
    assert not set(PLACE_KEYS) & set(c) and off.place is None
    for attr in ("place_src", "place_pushed", "place_desc"):
        assert not hasattr(off.b, attr), attr
    assert "place" not in off.b.timed
    on = _engine(b, yaw=Y, place=P)
    got = _run(on, b.hb)
    assert all(hasattr(on.b, attr) for attr in ("place_src", "place_pushed", "place_desc")) and set(got) == set(a) | set(PLACE_KEYS)
    with pytest.raises(ValueError, match="needs yaw=YawFit"):
        lifting.LiftEngine("cuda:0", classes=b.classes, place=P)


# ------------------------------------------------------------------------------------------------ the entry points
def test_nuscenes_entry_point(tmp_path):
    """src/nuscenes/2d_to_3d.py --yaw fit --place fit on the scene with the car of two faces, both host routes: the translation the JSON
    holds for it lies within eps * (L + W) + hypot(|len - CAR_L|, |wid - CAR_W|) / 2 of the car's true centre -- the fit's angle bound
    times the lever of the corner, plus what the class prior is off by -- and nearer than what --yaw fit alone wrote; --place push
    writes the bytes of no flag."""
    from cm3d_amd import lifting, nusc_io
    cfg, dataroot, mask_dir, heading = _scene_with_l_vehicle(tmp_path)
    env = dict(os.environ, CM3D_VER_NAME="v1.0-synth", CM3D_INPUT_PATH=dataroot, CM3D_INPUT_DIR=mask_dir)
    blobs = {}
    for route, extra in (("plain", []), ("push", ["--place", "push", "--place-thin", "2"]), ("yaw", ["--yaw", "fit"]),
                         ("native", ["--yaw", "fit", "--place", "fit"]), ("python", ["--yaw", "fit", "--place", "fit", "--reader-threads", "-1"])):
        p = subprocess.run([sys.executable, "2d_to_3d.py", "--ratio", str(cfg.ratio), "--n-sweeps", str(cfg.n_sweeps)] + extra,
                           cwd=os.path.join(ROOT, "src", "nuscenes"), env=dict(env, CM3D_OUTPUT_DIR=str(tmp_path / route)), capture_output=True,
                           text=True, timeout=600)
        assert p.returncode == 0, p.stderr[-2000:]
        blobs[route] = open(tmp_path / route / "pseudolabels_minival.json", "rb").read()
    assert blobs["push"] == blobs["plain"] and blobs["native"] != blobs["yaw"]
    assert json.loads(blobs["native"]) == json.loads(blobs["python"])
    # the car's true centre: where add_l_vehicle put it, from the frame's camera record
    tables = nusc_io.NuscTables("v1.0-synth", dataroot)
    fr = nusc_io.frames_of_scene(tables, tables.scenes()[0], mask_dir, n_sweeps=cfg.n_sweeps, ratio=cfg.ratio)[0]
    centre = yc._unproject_camera_point(np.asarray(fr.cams[0], np.float64), [0.4, 0.3, 12.0])[:2]

    def car_centre(blob):
        boxes = [bx for v in json.loads(blob)["results"].values() for bx in v if bx["detection_score"] == 0.987]
        assert len(boxes) == 1 and boxes[0]["detection_name"] == "car"
        return np.array(boxes[0]["translation"][:2])
    classes = lifting.ClassTable.nuscenes()
    wid, ln = classes.prior_wlh[classes.index("car")][:2]
    eps = fc.known_answer_bound(128, yc.CAR_L, 0.05)
    bound = eps * (yc.CAR_L + yc.CAR_W) + math.hypot(abs(ln - yc.CAR_L), abs(wid - yc.CAR_W)) / 2
    d_fit, d_push = (float(np.hypot(*(car_centre(blobs[k]) - centre))) for k in ("native", "yaw"))
    print(f"car of two faces: --yaw fit --place fit {d_fit:.4f} m from the true centre (bound {bound:.4f}), --yaw fit alone {d_push:.4f} m")
    assert d_fit <= bound
    assert d_push > d_fit


def test_waymo_entry_point(tmp_path):
    """src/waymo/2d_to_3d.py --yaw fit --place fit: the file is the one an engine with the option gives, and not the one of an engine
    without.  (The scene's lists are a few points long: 2 points and no least length let its vehicles take the fit.)"""
    from tests.test_gpu_entrypoint import _write_waymo_scene
    from cm3d_amd import lifting, pipeline_waymo as pw, waymo as wm
    scene = "segment-synthetic-0"
    _write_waymo_scene(tmp_path, scene, 0, 3)
    cwd = os.path.join(ROOT, "src", "waymo")
    args = ["--frames-dir", str(tmp_path / "frames"), "--mask-dir", str(tmp_path / "masks")]
    p = subprocess.run([sys.executable, "2d_to_3d.py", *args, "--output", str(tmp_path / "placed.bin"), "--yaw", "fit", "--yaw-fit-min-points", "2",
                        "--yaw-fit-min-length", "0", "--place", "fit", "--place-thin", "0.25"], cwd=cwd, capture_output=True, text=True, timeout=600)
    assert p.returncode == 0, p.stderr[-2000:]
    blob = open(tmp_path / "placed.bin", "rb").read()
    frames, lanes = pw.load_scene(str(tmp_path / "frames"), str(tmp_path / "masks"), scene)
    classes = lifting.ClassTable.waymo()
    hb = lifting.pack_frames(frames, [lanes], [0] * len(frames), classes)
    y = bevfit.YawFit(min_points=2, min_length=0.0)
    got = _run(lifting.LiftEngine("cuda:0", classes=classes, yaw=y, place=boxplace.BoxPlace(0.25)), hb)
    assert (got["place_src"] > 0).sum() >= 1
    ids = [(f.context_name, f.timestamp_micros) for f in frames]
    objs = wm.objects_from_results(hb, got, classes, ids)
    assert blob == wm.encode_objects(objs) and len(objs) >= 2
    unplaced = _run(lifting.LiftEngine("cuda:0", classes=classes, yaw=y), hb)
    assert blob != wm.encode_objects(wm.objects_from_results(hb, unplaced, classes, ids))
