"""GPU: LiftEngine(vertical=BoxVertical()) on the two-frame nuScenes and Waymo batches of tests/yaw_fit_pass_cases.py -- alone, behind
the clustered and the filtered pass, with every other stage on (the moving scenes of tests/box_size_pass_cases.py, which have the
sample links the velocity stage needs), through a captured graph and through LiftPipeline.rerun with two batches in flight -- and both
entry points on scenes written to disk.

The expectation is boxvertical.box_vertical_host on the CPU oracle's lists and the composed CPU pass's boxes and flags; nothing in it
comes from the device.  vert_status, vert_src, vert_z, vert_h and column 2 of the judged masks are functions of the float32 lists, of
bit 0 of flags, the class and the prior alone: to the bit.  Every other column and every unjudged mask are the bytes of the same engine
without the option."""
import os
import subprocess
import sys

import numpy as np
import pytest

from cm3d_amd import boxvertical as bv
from cm3d_amd import cluster as clustermod
from tests import box_size_pass_cases as sp
from tests import optin_pass_cases as oc
from tests import velocity_pass_cases as pc
from tests import yaw_fit_pass_cases as yc
from tests.test_gpu_optin_passes import _run, _same_bytes, _sync_download

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
V = bv.BoxVertical()
OTHERS = [0, 1, 3, 4, 5, 6, 7, 8, 9]


def _engine(b, **kw):
    from cm3d_amd import lifting
    return lifting.LiftEngine("cuda:0", classes=b.classes, **kw)


def _expect(b, front, box, flags, v=V):
    """The host statement on the oracle's lists (the clustered ones where the expectation has them) and a composed pass's box, flags."""
    if "cl_off" in front:
        off, xyz = front["cl_off"], front["cl_xyz"]
    else:
        off, xyz = front["hit_off"], oc.hit_xyz_of(b.hb, front)
    xyz = np.asarray(xyz, np.float32)
    xyz4 = np.zeros((len(xyz), 4), np.float32)
    xyz4[:, :xyz.shape[1]] = xyz
    return bv.box_vertical_host(xyz4, off, len(xyz4), box, flags, b.classes.prior_wlh, v.q_bot, v.q_top, v.min_points, v.lo, v.hi)


def _bits(a):
    return np.ascontiguousarray(a, np.float64).view(np.uint64)


def _check(got, base, exp):
    """got: the engine with the option; base: the same engine without; exp: _expect."""
    assert set(got) == set(base) | set(bv.RESULTS)
    for k in ("vert_status", "vert_src"):
        assert got[k].dtype == np.int32 and np.array_equal(got[k], exp[k]), k
    for k in ("vert_z", "vert_h"):
        assert np.array_equal(_bits(got[k]), _bits(exp[k])), k
    judged = exp["vert_src"] > 0
    assert np.array_equal(_bits(got["box"][judged, 2]), _bits(exp["box"][judged, 2]))
    assert got["box"][:, OTHERS].tobytes() == base["box"][:, OTHERS].tobytes()
    assert got["box"][~judged, 2].tobytes() == base["box"][~judged, 2].tobytes() and got["vert_entry_z"].tobytes() == base["box"][:, 2].tobytes()
    for k in base:
        if k != "box":
            assert got[k].dtype == base[k].dtype and got[k].tobytes() == base[k].tobytes(), k
    print(f"{len(judged)} masks: vert_src {np.bincount(exp['vert_src'], minlength=3).tolist()}, vert_status "
          f"{dict(zip(*[a.tolist() for a in np.unique(exp['vert_status'], return_counts=True)]))}, z moved by up to "
          f"{np.abs(got['box'][judged, 2] - base['box'][judged, 2]).max() if judged.any() else 0.0:.3f} m")
    return judged


def _poison_vertical(eng):
    for k in bv.RESULTS:
        getattr(eng.b, k).fill_(-3)
    eng.b.box.fill_(-3.0)


@pytest.mark.parametrize("name", ["nusc", "waymo"])
def test_the_engine_equals_the_host_statement_on_the_oracles_lists(oracle, name):
    import torch
    b = yc.batch(name)
    front = yc.plain(oracle, name)
    exp = _expect(b, front, front["box"], front["flags"])
    base = _run(_engine(b), b.hb)
    eng = _engine(b, vertical=V)
    got = _run(eng, b.hb)
    judged = _check(got, base, exp)
    assert judged.sum() >= 5 and {0, 1, 2} <= set(exp["vert_status"])
    # the car of two faces: five rings over 0.8 m, less than 0.7 priors: its prior height hung on the top ring
    for m in b.l_masks:
        h0 = b.classes.prior_wlh[b.hb.class_id[m], 2]
        assert got["vert_src"][m] == 2 and got["vert_h"][m] == h0 and got["box"][m, 2] == got["vert_z"][m, 1] - h0 * 0.5
    # a second pass rewrites everything; stage_vertical alone on what it left gives the same box; so does a captured graph
    _poison_vertical(eng)
    _same_bytes(_run(eng), got)
    eng.stage_vertical(torch.cuda.current_stream().cuda_stream)
    again = _sync_download(eng)
    assert again["box"].tobytes() == got["box"].tobytes() and again["vert_entry_z"].tobytes() == got["box"][:, 2].tobytes()
    eng.run(masks="rle")
    g = eng.capture_graph(masks="rle")
    _poison_vertical(eng)
    g.replay()
    _same_bytes(_sync_download(eng), got)
    assert all(np.array_equal(eng.download(full=False)[k], got[k]) for k in bv.RESULTS)


@pytest.mark.parametrize("name", ["nusc", "waymo"])
def test_behind_the_clustered_pass_on_the_clustered_lists(oracle, name):
    b = yc.batch(name)
    c = clustermod.DepthCluster(1.0, 20)
    front = yc.expected_of(oracle, name, cluster=c)
    exp = _expect(b, front, front["box"], front["flags"])
    plain = yc.plain(oracle, name)
    assert not np.array_equal(exp["vert_z"], _expect(b, plain, plain["box"], plain["flags"])["vert_z"])      # the clustering changes the lists
    _check(_run(_engine(b, cluster=c, vertical=V), b.hb), _run(_engine(b, cluster=c), b.hb), exp)


@pytest.mark.parametrize("name", ["nusc", "waymo"])
def test_behind_the_filtered_pass(oracle, name):
    """A mask the filter dropped has no box: bit 0 of its flags is clear and it is not judged."""
    b = yc.batch(name)
    f = oc.lane_filters(yc.plain(oracle, name))
    front = yc.expected_of(oracle, name, filters=f)
    exp = _expect(b, front, front["box"], front["flags"])
    dropped = (front["medoid_pos"] >= 0) & (front["medoid_pos_kept"] < 0)
    assert dropped.sum() >= 3 and not exp["vert_src"][dropped].any() and exp["vert_src"].any()
    _check(_run(_engine(b, filters=f, vertical=V), b.hb), _run(_engine(b, filters=f), b.hb), exp)


def test_with_every_other_stage_on_and_the_kept_rows(oracle):
    """Yaw fit, placement, velocity, tracks and size: the stage runs in front of the velocity stage and changes nothing they see;
    kept_box_sizes' column 2 is vert_h, columns 0 and 1 the size stage's."""
    from cm3d_amd import lifting
    from cm3d_amd import tracks as T
    b = sp.batch()
    kw = dict(yaw=sp.Y, place=sp.P, velocity=pc.settings()[0], tracks=T.Tracks(2, "mean", 2), size=sp.S)
    before, out = sp.composed(oracle, tracks=(2, "mean", 2))
    front = oc._frozen(oc.oracle_batch(oracle, b.frames, b.lanes, b.frame_lane, b.hb))
    exp = _expect(b, front, out["box"], before["flags"])
    base = _run(_engine(b, **kw), b.hb)
    eng = _engine(b, vertical=V, **kw)
    got = _run(eng, b.hb)
    judged = _check(got, base, exp)
    assert judged.sum() >= 6 and (got["size_src"] > 0).sum() >= 6
    keep = (got["flags"] & 3) == 3
    rows = lifting.kept_box_sizes(eng.b).cpu().numpy()
    assert rows[:, 2].tobytes() == got["vert_h"][keep].tobytes() and rows[:, :2].tobytes() == np.ascontiguousarray(got["size_wlh"][keep, :2]).tobytes()
    assert (rows[:, 2] != got["size_wlh"][keep, 2]).any()
    # without a size stage: the class's prior beside vert_h
    alone = _engine(b, vertical=V)
    res = _run(alone, b.hb)
    k2 = (res["flags"] & 3) == 3
    rows = lifting.kept_box_sizes(alone.b).cpu().numpy()
    assert rows[:, :2].tobytes() == np.ascontiguousarray(b.classes.prior_wlh[b.hb.class_id[k2], :2]).tobytes()
    assert rows[:, 2].tobytes() == res["vert_h"][k2].tobytes()


def test_pipeline_rerun_with_two_batches_in_flight_and_the_timer_pair(oracle):
    import torch
    from cm3d_amd import lifting
    b = yc.batch("nusc")
    front = yc.plain(oracle, "nusc")
    exp = _expect(b, front, front["box"], front["flags"])
    pipe = lifting.LiftPipeline("cuda:0", depth=2, classes=b.classes, vertical=V)
    ev = []
    slots = [pipe.submit(b.hb, "rle", stage_events=ev), pipe.submit(b.hb, "rle")]
    assert len(ev) == 7 and not pipe.engines[0].b.plain_pass          # the plain pass's five events, then the stage's pair
    before = pipe.native_passes
    for s in slots:
        pipe.rerun(s)
    pipe.rerun(slots[0])
    assert pipe.native_passes == before + 3
    for s in slots:
        got = pipe.collect(s, full=False)[1]
        torch.cuda.synchronize()
        for k in ("vert_status", "vert_src"):
            assert np.array_equal(got[k], exp[k]), k
        judged = exp["vert_src"] > 0
        assert np.array_equal(_bits(got["vert_z"]), _bits(exp["vert_z"])) and np.array_equal(_bits(got["box"][judged, 2]), _bits(exp["box"][judged, 2]))
    assert ev[4].elapsed_time(ev[5]) >= 0.0 and ev[5].elapsed_time(ev[6]) >= 0.0


@pytest.mark.parametrize("name", ["nusc", "waymo"])
def test_without_the_option_nothing_changes(name):
    from cm3d_amd import lifting
    b = yc.batch(name)
    without, off = _engine(b), _engine(b, vertical=None)
    a, c = _run(without, b.hb), _run(off, b.hb)
    _same_bytes(a, c)
    assert off.vertical is None and off.b.plain_pass and not any(hasattr(off.b, k) for k in bv.RESULTS + ("prior_wlh",))
    on = _engine(b, vertical=V)
    on.upload(b.hb)
    assert all(hasattr(on.b, k) for k in bv.RESULTS) and not on.b.plain_pass
    with pytest.raises(ValueError, match="KITTI"):
        lifting.LiftEngine("cuda:0", classes=b.classes, obb=True, vertical=V)


# ------------------------------------------------------------------------------------------------ the entry points
def test_nuscenes_entry_point_writes_the_engines_heights(tmp_path):
    """src/nuscenes/2d_to_3d.py --vertical fit on scenes written to disk, both host routes: the file is the text writer's for the
    records and size rows of an engine with the option on the batch packed from the same files; --vertical medoid writes the bytes of
    no flag."""
    from cm3d_amd import lifting
    from cm3d_amd.pipeline_nuscenes import META
    dataroot, mask_dir, names = sp.write_dataset(tmp_path)
    env = dict(os.environ, CM3D_VER_NAME="v1.0-synth", CM3D_INPUT_PATH=dataroot, CM3D_INPUT_DIR=mask_dir)
    runs = {"none": (), "medoid": ("--vertical", "medoid"), "native": ("--vertical", "fit"),
            "python": ("--vertical", "fit", "--reader-threads", "-1")}
    out = {}
    for key, flags in runs.items():
        r = subprocess.run([sys.executable, "2d_to_3d.py", "--ratio", str(sp.config().ratio), *flags], cwd=os.path.join(ROOT, "src", "nuscenes"),
                           env=dict(env, CM3D_OUTPUT_DIR=str(tmp_path / key)), capture_output=True, text=True, timeout=300)
        assert r.returncode == 0, r.stderr[-2000:]
        out[key] = open(tmp_path / key / "pseudolabels_minival.json", "rb").read()
    assert out["medoid"] == out["none"] and out["native"] != out["none"] and out["native"] == out["python"]
    hb = sp.dataset_batch(dataroot, mask_dir, names)
    classes = lifting.ClassTable.nuscenes()
    ids = np.stack([np.arange(hb.n_frames), np.zeros(hb.n_frames)], 1)
    eng = lifting.LiftEngine("cuda:0", classes=classes, vertical=V)
    got = _run(eng, hb)
    rec = lifting.kept_box_records(eng.b, ids).cpu().numpy()
    sizes = lifting.kept_box_sizes(eng.b).cpu().numpy()
    assert (got["vert_src"] > 0).sum() >= 6 and (sizes[:, 2] != classes.prior_wlh[rec[:, 8].astype(int), 2]).any()
    text, n = lifting.nuscenes_results_json(rec, hb.tokens, classes, dict(META), size=sizes)
    assert out["native"] == text.encode() and n == len(rec)


def test_waymo_entry_point_writes_the_engines_heights(tmp_path):
    """src/waymo/2d_to_3d.py --vertical fit: the file is objects_from_results' for an engine with the option; --vertical medoid writes
    the bytes of no flag.  (The scene's lists are a few points long: with min_points 1 every box is judged -- it has a medoid, so a point.)"""
    from tests.test_gpu_entrypoint import _write_waymo_scene
    from cm3d_amd import lifting, pipeline_waymo as pw, waymo as wm
    scene = "segment-synthetic-0"
    _write_waymo_scene(tmp_path, scene, 0, 3)
    args = ["--frames-dir", str(tmp_path / "frames"), "--mask-dir", str(tmp_path / "masks")]
    blobs = {}
    for key, extra in (("plain", []), ("medoid", ["--vertical", "medoid"]), ("fit", ["--vertical", "fit", "--vertical-min-points", "1"])):
        p = subprocess.run([sys.executable, "2d_to_3d.py", *args, "--output", str(tmp_path / f"{key}.bin"), *extra],
                           cwd=os.path.join(ROOT, "src", "waymo"), capture_output=True, text=True, timeout=300)
        assert p.returncode == 0, p.stderr[-2000:]
        blobs[key] = open(tmp_path / f"{key}.bin", "rb").read()
    assert blobs["medoid"] == blobs["plain"] and blobs["fit"] != blobs["plain"]
    frames, lanes = pw.load_scene(str(tmp_path / "frames"), str(tmp_path / "masks"), scene)
    classes = lifting.ClassTable.waymo()
    hb = lifting.pack_frames(frames, [lanes], [0] * len(frames), classes)
    got = _run(lifting.LiftEngine("cuda:0", classes=classes, vertical=bv.BoxVertical(min_points=1)), hb)
    assert ((got["vert_src"] > 0) & ((got["flags"] & 3) == 3)).sum() >= 1
    objs = wm.objects_from_results(hb, got, classes, [(f.context_name, f.timestamp_micros) for f in frames])
    assert blobs["fit"] == wm.encode_objects(objs) and len(objs) >= 2
