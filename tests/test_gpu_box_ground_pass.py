"""GPU: LiftEngine(ground=BoxGround()) on the two-frame nuScenes and Waymo batches of tests/box_ground_cases.py (pass_batch: the batches
of tests/yaw_fit_pass_cases.py with a tilted ground sheet of rings in every frame) -- alone, with the vertical stage, behind the
clustered and the filtered pass, with every other stage on (the moving scenes of tests/box_size_pass_cases.py, which have the sample
links the velocity stage needs; their ground is the synthetic sweeps' own), with the cloud materialised, through a captured graph and
through LiftPipeline.rerun with two batches in flight -- and both entry points on scenes written to disk.

The expectation is boxground.box_ground_host on the oracle's sweep preparation of the batch's rows and on the composed CPU pass's boxes
and flags, behind boxvertical.box_vertical_host where the engine has that stage; nothing in it comes from the device.  The six results
and column 2 of the judged masks: to the bit.  Every other column, every unjudged mask and every other download key are the bytes of
the same engine without the option."""
import os
import subprocess
import sys

import numpy as np
import pytest

from cm3d_amd import boxground as bg
from cm3d_amd import boxvertical as bv
from cm3d_amd import cluster as clustermod
from tests import box_ground_cases as gc
from tests import box_size_pass_cases as sp
from tests import optin_pass_cases as oc
from tests import velocity_pass_cases as pc
from tests.test_gpu_optin_passes import _run, _same_bytes, _sync_download

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
G, V = bg.BoxGround(), bv.BoxVertical()
OTHERS = [0, 1, 3, 4, 5, 6, 7, 8, 9]
INT_KEYS = ("ground_status", "ground_src", "ground_n")
F64_KEYS = ("ground_z", "ground_h", "ground_zref")


def _engine(b, **kw):
    from cm3d_amd import lifting
    return lifting.LiftEngine("cuda:0", classes=b.classes, **kw)


def _bits(a):
    return np.ascontiguousarray(a, np.float64).view(np.uint64)


def _check(got, base, exp):
    """got: the engine with the option; base: the same engine without; exp: the ground stage's dict of box_ground_cases.pass_expected."""
    assert set(got) == set(base) | set(bg.RESULTS)
    for k in INT_KEYS:
        assert got[k].dtype == np.int32 and np.array_equal(got[k], exp[k]), (k, np.flatnonzero(got[k] != exp[k]))
    for k in F64_KEYS:
        assert np.array_equal(_bits(got[k]), _bits(exp[k])), (k, np.flatnonzero(_bits(got[k]) != _bits(exp[k])))
    judged = exp["ground_src"] > 0
    assert np.array_equal(_bits(got["box"][judged, 2]), _bits(exp["box"][judged, 2]))
    assert got["box"][:, OTHERS].tobytes() == base["box"][:, OTHERS].tobytes()
    assert got["box"][~judged, 2].tobytes() == base["box"][~judged, 2].tobytes()
    for k in base:
        if k != "box":
            assert got[k].dtype == base[k].dtype and got[k].tobytes() == base[k].tobytes(), k
    print(f"{len(judged)} masks: ground_src {np.bincount(exp['ground_src'], minlength=3).tolist()}, ground_status "
          f"{dict(zip(*[a.tolist() for a in np.unique(exp['ground_status'], return_counts=True)]))}, z moved by up to "
          f"{np.abs(got['box'][judged, 2] - base['box'][judged, 2]).max() if judged.any() else 0.0:.3f} m")
    return judged


def _poison_ground(eng):
    for k in bg.RESULTS:
        getattr(eng.b, k).fill_(-3)
    eng.b.box.fill_(-3.0)


@pytest.mark.parametrize("name", ["nusc", "waymo"])
def test_the_engine_alone_equals_the_host_statement_on_the_oracles_cloud(oracle, name):
    import torch
    b = gc.pass_batch(name)
    front = gc.pass_plain(oracle, name)
    _, exp = gc.pass_expected(b, front, front["box"], front["flags"], G)
    base = _run(_engine(b), b.hb)
    eng = _engine(b, ground=G)
    got = _run(eng, b.hb)
    judged = _check(got, base, exp)
    # what the scenes are built for: every status, both sources an engine without a vertical stage has, enough judged masks
    assert judged.sum() >= 5 and {0, 1, 2} <= set(exp["ground_status"]) and set(exp["ground_src"]) == {0, 2}
    assert got["ground_zref"].tobytes() == base["box"][:, 2].tobytes() and eng.b.points is None         # the default route: no cloud
    # a second pass rewrites everything; stage_ground alone on what it left, zref = ground_zref, gives the same arrays; so does a graph
    _poison_ground(eng)
    _same_bytes(_run(eng), got)
    eng.stage_ground(torch.cuda.current_stream().cuda_stream, zref=eng.b.ground_zref)
    _same_bytes(_sync_download(eng), got)
    eng.run(masks="rle")
    g = eng.capture_graph(masks="rle")
    _poison_ground(eng)
    g.replay()
    _same_bytes(_sync_download(eng), got)
    assert all(np.array_equal(eng.download(full=False)[k], got[k]) for k in bg.RESULTS)
    # the cloud materialised: the stage reads it in place of the raw rows, the same bytes
    kept = _engine(b, ground=G, keep_cloud=True)
    cloud = _run(kept, b.hb)
    assert kept.b.points is not None and "points" in cloud
    _same_bytes({k: v for k, v in cloud.items() if k != "points"}, got)


@pytest.mark.parametrize("name", ["nusc", "waymo"])
def test_with_the_vertical_stage(oracle, name):
    """zref is the pass's z (vert_entry_z), the top is the vertical stage's: all three sources occur."""
    b = gc.pass_batch(name)
    front = gc.pass_plain(oracle, name)
    vert, exp = gc.pass_expected(b, front, front["box"], front["flags"], G, V)
    base = _run(_engine(b, vertical=V), b.hb)
    got = _run(_engine(b, vertical=V, ground=G), b.hb)
    judged = _check(got, base, exp)
    assert judged.sum() >= 5 and {0, 1, 2} <= set(exp["ground_status"]) and set(exp["ground_src"]) == {0, 1, 2}
    assert np.array_equal(_bits(got["ground_zref"]), _bits(vert["vert_entry_z"])) and got["ground_zref"].tobytes() == got["vert_entry_z"].tobytes()
    left = exp["ground_src"] == 0                    # left alone: the vertical stage's height, bit for bit
    assert got["ground_h"][left].tobytes() == got["vert_h"][left].tobytes()


@pytest.mark.parametrize("name", ["nusc", "waymo"])
def test_behind_the_clustered_pass(oracle, name):
    b = gc.pass_batch(name)
    c = clustermod.DepthCluster(1.0, 20)
    front = oc.expected(oracle, b.frames, b.lanes, b.frame_lane, b.hb, cluster=c, base=gc.pass_plain(oracle, name))
    _, exp = gc.pass_expected(b, front, front["box"], front["flags"], G, V)
    _check(_run(_engine(b, cluster=c, vertical=V, ground=G), b.hb), _run(_engine(b, cluster=c, vertical=V), b.hb), exp)
    assert exp["ground_src"].any()


@pytest.mark.parametrize("name", ["nusc", "waymo"])
def test_behind_the_filtered_pass(oracle, name):
    """A mask the filter dropped has no box: bit 0 of its flags is clear and it is not judged; its status and ground are written."""
    b = gc.pass_batch(name)
    plain = gc.pass_plain(oracle, name)
    f = oc.lane_filters(plain)
    front = oc.expected(oracle, b.frames, b.lanes, b.frame_lane, b.hb, filters=f, base=plain)
    _, exp = gc.pass_expected(b, front, front["box"], front["flags"], G)
    dropped = (front["medoid_pos"] >= 0) & (front["medoid_pos_kept"] < 0)
    assert dropped.sum() >= 3 and not exp["ground_src"][dropped].any() and exp["ground_src"].any()
    _check(_run(_engine(b, filters=f, ground=G), b.hb), _run(_engine(b, filters=f), b.hb), exp)


def test_with_every_other_stage_on_and_the_kept_rows(oracle):
    """Yaw fit, placement, velocity, tracks, size and the vertical stage: the stage runs in front of the velocity stage and changes
    nothing they see; kept_box_sizes' column 2 is ground_h, columns 0 and 1 the size stage's."""
    from cm3d_amd import lifting
    from cm3d_amd import tracks as T
    b = sp.batch()
    kw = dict(yaw=sp.Y, place=sp.P, velocity=pc.settings()[0], tracks=T.Tracks(2, "mean", 2), size=sp.S, vertical=V)
    before, out = sp.composed(oracle, tracks=(2, "mean", 2))
    front = oc._frozen(oc.oracle_batch(oracle, b.frames, b.lanes, b.frame_lane, b.hb))
    # (the stage stands in front of the velocity, track and size stages: it sees the centres the placement left, not the sized ones)
    _, exp = gc.pass_expected(b, front, before["box"], before["flags"], G, V)
    base = _run(_engine(b, **kw), b.hb)
    eng = _engine(b, ground=G, **kw)
    got = _run(eng, b.hb)
    judged = _check(got, base, exp)
    assert judged.sum() >= 5
    keep = (got["flags"] & 3) == 3
    rows = lifting.kept_box_sizes(eng.b).cpu().numpy()
    assert rows[:, 2].tobytes() == got["ground_h"][keep].tobytes() and rows[:, :2].tobytes() == np.ascontiguousarray(got["size_wlh"][keep, :2]).tobytes()
    # without a size or vertical stage: the class's prior beside ground_h
    alone = _engine(b, ground=G)
    res = _run(alone, b.hb)
    k2 = (res["flags"] & 3) == 3
    rows = lifting.kept_box_sizes(alone.b).cpu().numpy()
    assert rows[:, :2].tobytes() == np.ascontiguousarray(b.classes.prior_wlh[b.hb.class_id[k2], :2]).tobytes()
    assert rows[:, 2].tobytes() == res["ground_h"][k2].tobytes()


def test_pipeline_rerun_with_two_batches_in_flight_and_the_timer_pair(oracle):
    import torch
    from cm3d_amd import lifting
    b = gc.pass_batch("nusc")
    front = gc.pass_plain(oracle, "nusc")
    _, exp = gc.pass_expected(b, front, front["box"], front["flags"], G, V)
    pipe = lifting.LiftPipeline("cuda:0", depth=2, classes=b.classes, vertical=V, ground=G)
    ev = []
    slots = [pipe.submit(b.hb, "rle", stage_events=ev), pipe.submit(b.hb, "rle")]
    assert len(ev) == 9 and not pipe.engines[0].b.plain_pass          # the plain pass's five events, the vertical stage's pair, then this one's
    before = pipe.native_passes
    for s in slots:
        pipe.rerun(s)
    pipe.rerun(slots[0])
    assert pipe.native_passes == before + 3
    for s in slots:
        got = pipe.collect(s, full=False)[1]
        torch.cuda.synchronize()
        for k in INT_KEYS:
            assert np.array_equal(got[k], exp[k]), k
        judged = exp["ground_src"] > 0
        assert all(np.array_equal(_bits(got[k]), _bits(exp[k])) for k in F64_KEYS)
        assert np.array_equal(_bits(got["box"][judged, 2]), _bits(exp["box"][judged, 2]))
    assert ev[6].elapsed_time(ev[7]) >= 0.0 and ev[7].elapsed_time(ev[8]) >= 0.0


@pytest.mark.parametrize("name", ["nusc", "waymo"])
def test_without_the_option_nothing_changes(name):
    from cm3d_amd import lifting
    b = gc.pass_batch(name)
    without, off = _engine(b), _engine(b, ground=None)
    a, c = _run(without, b.hb), _run(off, b.hb)
    _same_bytes(a, c)
    assert off.ground is None and off.b.plain_pass and not any(hasattr(off.b, k) for k in bg.RESULTS + ("prior_wlh", "nm_max"))
    on = _engine(b, ground=G)
    on.upload(b.hb)
    assert all(hasattr(on.b, k) for k in bg.RESULTS) and not on.b.plain_pass and on.b.points is None
    with pytest.raises(ValueError, match="KITTI"):
        lifting.LiftEngine("cuda:0", classes=b.classes, obb=True, ground=G)


# ------------------------------------------------------------------------------------------------ the entry points
def test_nuscenes_entry_point_writes_the_engines_heights(tmp_path):
    """src/nuscenes/2d_to_3d.py --ground fit on scenes written to disk, both host routes: the file is the text writer's for the records
    and size rows of an engine with the option on the batch packed from the same files -- the third number of "size" is ground_h --;
    --ground medoid writes the bytes of no flag."""
    from cm3d_amd import lifting
    from cm3d_amd.pipeline_nuscenes import META
    dataroot, mask_dir, names = sp.write_dataset(tmp_path)
    env = dict(os.environ, CM3D_VER_NAME="v1.0-synth", CM3D_INPUT_PATH=dataroot, CM3D_INPUT_DIR=mask_dir)
    runs = {"none": (), "medoid": ("--ground", "medoid"), "native": ("--ground", "fit"), "python": ("--ground", "fit", "--reader-threads", "-1")}
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
    eng = lifting.LiftEngine("cuda:0", classes=classes, ground=G)
    got = _run(eng, hb)
    rec = lifting.kept_box_records(eng.b, ids).cpu().numpy()
    sizes = lifting.kept_box_sizes(eng.b).cpu().numpy()
    keep = (got["flags"] & 3) == 3
    assert (got["ground_src"] > 0).sum() >= 5 and sizes[:, 2].tobytes() == got["ground_h"][keep].tobytes()
    text, n = lifting.nuscenes_results_json(rec, hb.tokens, classes, dict(META), size=sizes)
    assert out["native"] == text.encode() and n == len(rec)


def test_waymo_entry_point_writes_the_engines_heights(tmp_path):
    """src/waymo/2d_to_3d.py --ground fit with --vertical fit: the file is objects_from_results' for an engine with both options, whose
    heights are ground_h; --ground medoid writes the bytes of no flag.  (The scene's sweeps are a few points: with min_points 1 every
    box with a point around it is judged.)"""
    from tests.test_gpu_entrypoint import _write_waymo_scene
    from cm3d_amd import lifting, pipeline_waymo as pw, waymo as wm
    scene = "segment-synthetic-0"
    _write_waymo_scene(tmp_path, scene, 0, 3)
    args = ["--frames-dir", str(tmp_path / "frames"), "--mask-dir", str(tmp_path / "masks")]
    fit = ["--ground", "fit", "--ground-min-points", "1", "--vertical", "fit", "--vertical-min-points", "1"]
    blobs = {}
    for key, extra in (("plain", []), ("medoid", ["--ground", "medoid"]), ("fit", fit), ("vertical", fit[4:])):
        p = subprocess.run([sys.executable, "2d_to_3d.py", *args, "--output", str(tmp_path / f"{key}.bin"), *extra],
                           cwd=os.path.join(ROOT, "src", "waymo"), capture_output=True, text=True, timeout=300)
        assert p.returncode == 0, p.stderr[-2000:]
        blobs[key] = open(tmp_path / f"{key}.bin", "rb").read()
    assert blobs["medoid"] == blobs["plain"] and blobs["fit"] != blobs["plain"] and blobs["fit"] != blobs["vertical"]
    frames, lanes = pw.load_scene(str(tmp_path / "frames"), str(tmp_path / "masks"), scene)
    classes = lifting.ClassTable.waymo()
    hb = lifting.pack_frames(frames, [lanes], [0] * len(frames), classes)
    got = _run(lifting.LiftEngine("cuda:0", classes=classes, vertical=bv.BoxVertical(min_points=1), ground=bg.BoxGround(min_points=1)), hb)
    assert ((got["ground_src"] > 0) & ((got["flags"] & 3) == 3)).sum() >= 1
    objs = wm.objects_from_results(hb, got, classes, [(f.context_name, f.timestamp_micros) for f in frames])
    assert blobs["fit"] == wm.encode_objects(objs) and len(objs) >= 2
