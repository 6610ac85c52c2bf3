"""GPU: LiftEngine(owner=PointOwner()) on the two-frame nuScenes and Waymo batches of tests/box_ground_cases.py (pass_batch) -- alone,
under both rules, with the ground strip, the clustering, the vertical stage, the yaw fit, the virtual points, with every other stage on
(the moving scenes of tests/box_size_pass_cases.py), with the cloud materialised, through a captured graph and through
LiftPipeline.rerun with two different batches in flight -- and the entry points on scenes written to disk.

The expectation is tests/point_owner_pass_cases.expected: the host statement of the ownership on the oracle's lists, then the strip,
the clustering, the oracle's medoid and its stage 2 as ground_strip_pass_cases and optin_pass_cases compose them; nothing in it comes
from the device.  Lists, statuses, ow_owner, medoid_pos and centroids: to the bit.  The box columns: test_gpu_parity's tolerance."""
import os
import subprocess
import sys

import numpy as np
import pytest

from cm3d_amd import bevfit
from cm3d_amd import boxvertical as bv
from cm3d_amd import cluster as clustermod
from cm3d_amd import groundstrip as gs
from cm3d_amd import pointowner as po
from cm3d_amd import virtualpoints as vp
from tests import box_ground_cases as bgc
from tests import box_size_pass_cases as sp
from tests import optin_pass_cases as oc
from tests import point_owner_pass_cases as pc
from tests import velocity_pass_cases as vc
from tests import yaw_fit_pass_cases as yc
from tests.test_gpu_optin_passes import _check_pass, _run, _same_bytes, _sync_download
from tests.test_gpu_yaw_fit_pass import _check_fitted

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
O, S, V, Y = pc.OWNER, gs.GroundStrip(), bv.BoxVertical(), bevfit.YawFit()
C = clustermod.DepthCluster(1.0, 20)
OW_BUFFERS = ("ow_owner", "ow_off", "ow_tile_off", "ow_idx", "ow_xyz", "ow_status", "ow_lost", "ow_ws", "owner_desc")
GS_KEYS = ("gs_off", "gs_status", "gs_dropped", "gs_idx", "gs_xyz", "grid_z", "grid_n")


def _engine(b, **kw):
    from cm3d_amd import lifting
    return lifting.LiftEngine("cuda:0", classes=b.classes, **kw)


def _bits(a):
    return np.ascontiguousarray(a, np.float64).view(np.uint64)


def _check_owner(eng, got, exp):
    """The stage's own outputs, to the bit."""
    for k in ("ow_off", "ow_status", "ow_lost", "ow_owner", "ow_idx"):
        assert got[k].dtype == np.int32 and got[k].shape == exp[k].shape and np.array_equal(got[k], exp[k]), (k, np.flatnonzero(got[k] != exp[k])[:8])
    assert np.array_equal(eng.b.ow_tile_off.cpu().numpy(), exp["ow_tile_off"])
    assert got["ow_xyz"].shape == exp["ow_xyz"].shape and got["ow_xyz"].tobytes() == np.ascontiguousarray(exp["ow_xyz"], np.float32).tobytes()


def _check_strip(eng, got, exp):
    for k in ("gs_off", "gs_status", "gs_dropped", "gs_idx", "grid_n"):
        assert np.array_equal(got[k], exp[k]), (k, np.flatnonzero(got[k] != exp[k])[:8])
    assert np.array_equal(eng.b.gs_tile_off.cpu().numpy(), exp["gs_tile_off"])
    assert got["gs_xyz"].tobytes() == np.ascontiguousarray(exp["gs_xyz"], np.float32).tobytes()
    assert np.array_equal(_bits(got["grid_z"]), _bits(exp["grid_z"]))


def _poison_owner(eng, results=True):
    b = eng.b
    for k in ("ow_owner", "ow_off", "ow_tile_off", "ow_idx", "ow_status", "ow_lost") + (("medoid_pos",) if results else ()):
        getattr(b, k).fill_(-3)
    b.ow_xyz.fill_(-3.0), b.ow_ws.fill_(0x7F)
    if results:
        b.centroid.fill_(-3.0), b.box.fill_(-3.0)


@pytest.mark.parametrize("name", ["nusc", "waymo"])
def test_the_engine_alone_equals_the_composed_cpu_pass(oracle, name):
    import torch
    b = pc.batch(name)
    exp = pc.expected_of(oracle, name)
    eng = _engine(b, owner=O)
    got = _run(eng, b.hb)
    _check_pass(b.hb, got, exp)                      # raw lists, medoids (positions in the exclusive lists), lane results, flags, boxes
    _check_owner(eng, got, exp)
    assert eng.b.points is None and not eng.b.plain_pass and eng.b.max_pts == pc.max_pts(b.hb)
    base = _run(_engine(b), b.hb)
    assert set(got) == set(base) | set(pc.OW_KEYS)
    # conditions on the inputs, at the defaults: the test does not pass on nothing
    moved = (got["centroid"] != base["centroid"]).any(1)
    status = np.bincount(got["ow_status"], minlength=3)
    print(f"{name}: ow_status {status.tolist()}, {int((got['ow_lost'] > 0).sum())} masks lose points, {int(got['ow_lost'].sum())} of "
          f"{int(got['hit_off'][-1])} positions lost, {pc.contested(exp, b.hb)} listed / contested points, {int(moved.sum())} medoids moved")
    assert (O.rule, O.min_keep) == ("score", 5)
    assert (got["ow_lost"] > 0).sum() >= 3 and got["ow_lost"].sum() >= 300 and (status > 0).all() and moved.any()
    assert got["hit_idx"].tobytes() == base["hit_idx"].tobytes() and got["hit_xyz"].tobytes() == base["hit_xyz"].tobytes()
    # a second pass after poisoning every ow_* buffer and the workspace; the stage alone on the resident raw lists; a captured graph
    _poison_owner(eng)
    _same_bytes(_run(eng), got)
    _poison_owner(eng, results=False)
    eng.b.ow_ws.fill_(0xFF)
    eng.stage_point_owner(torch.cuda.current_stream().cuda_stream)
    _same_bytes(_sync_download(eng), got)
    g = eng.capture_graph(masks="rle")
    _poison_owner(eng)
    g.replay()
    _same_bytes(_sync_download(eng), got)
    small = eng.download(full=False)
    assert all(np.array_equal(small[k], got[k]) for k in ("ow_off", "ow_status", "ow_lost")) and "ow_xyz" not in small and "ow_owner" not in small
    # the cloud materialised: the same bytes
    kept = _engine(b, owner=O, keep_cloud=True)
    cloud = _run(kept, b.hb)
    assert kept.b.points is not None and "points" in cloud
    _same_bytes({k: v for k, v in cloud.items() if k != "points"}, got)


@pytest.mark.parametrize("name", ["nusc", "waymo"])
def test_rule_smallest(oracle, name):
    b = pc.batch(name)
    small = po.PointOwner("smallest")
    exp = pc.expected_of(oracle, name, small)
    eng = _engine(b, owner=small)
    got = _run(eng, b.hb)
    _check_pass(b.hb, got, exp)
    _check_owner(eng, got, exp)
    assert not np.array_equal(exp["ow_owner"], pc.expected_of(oracle, name)["ow_owner"])       # the rules disagree on these batches


@pytest.mark.parametrize("name", ["nusc", "waymo"])
def test_with_the_ground_strip(oracle, name):
    """The strip's host statement reads the exclusive lists; medoid_pos is a position in the stripped exclusive ones."""
    b = pc.batch(name)
    exp = pc.expected_of(oracle, name, strip=S)
    eng = _engine(b, owner=O, strip=S)
    got = _run(eng, b.hb)
    _check_pass(b.hb, got, exp)
    _check_owner(eng, got, exp)
    _check_strip(eng, got, exp)
    from tests import ground_strip_pass_cases as gpc
    assert not np.array_equal(exp["gs_off"], gpc.expected_of(oracle, name)["gs_off"])           # not what the strip makes of the raw lists
    assert list(eng.b.timed) == ["owner", "strip"]
    assert set(got) == set(_run(_engine(b, strip=S), b.hb)) | set(pc.OW_KEYS)


@pytest.mark.parametrize("name,strip", [("nusc", None), ("waymo", None), ("nusc", S)])
def test_with_the_clustering(oracle, name, strip):
    """The clustering sees the exclusive lists (the stripped exclusive ones behind a strip)."""
    b = pc.batch(name)
    exp = pc.expected_of(oracle, name, strip=strip, cluster=C)
    eng = _engine(b, owner=O, cluster=C, strip=strip)
    got = _run(eng, b.hb)
    _check_pass(b.hb, got, exp)
    _check_owner(eng, got, exp)
    if strip is not None:
        _check_strip(eng, got, exp)
    unowned = oc.expected(oracle, b.frames, b.lanes, b.frame_lane, b.hb, cluster=C, base=pc.plain(oracle, name))
    assert not np.array_equal(exp["cl_off"], unowned["cl_off"])
    import torch
    eng.b.cl_off.fill_(-3), eng.b.cl_idx.fill_(-3)
    eng.stage_cluster(torch.cuda.current_stream().cuda_stream)                 # the stage alone reads the same lists
    again = _sync_download(eng)
    assert np.array_equal(again["cl_off"], exp["cl_off"]) and np.array_equal(again["cl_idx"], exp["cl_idx"])


@pytest.mark.parametrize("name", ["nusc", "waymo"])
def test_with_the_vertical_stage(oracle, name):
    """The vertical stage reads the exclusive lists: its host statement on them and on the composed pass's boxes, to the bit."""
    b = pc.batch(name)
    exp = pc.expected_of(oracle, name)
    xyz, off = pc.read_lists(exp)
    vert = bv.box_vertical_host(xyz, off, len(xyz), exp["box"], exp["flags"], b.classes.prior_wlh, V.q_bot, V.q_top, V.min_points, V.lo, V.hi)
    eng = _engine(b, owner=O, vertical=V)
    got = _run(eng, b.hb)
    _check_owner(eng, got, exp)
    for k in ("vert_src", "vert_status"):
        assert np.array_equal(got[k], vert[k]), k
    assert np.array_equal(_bits(got["vert_z"]), _bits(vert["vert_z"])) and np.array_equal(_bits(got["vert_h"]), _bits(vert["vert_h"]))
    judged = vert["vert_src"] > 0
    assert judged.sum() >= 5 and np.allclose(got["box"][:, 2], vert["box"][:, 2], rtol=0, atol=1e-4)
    assert np.array_equal(_bits(got["box"][judged, 2]), _bits(vert["box"][judged, 2]))
    base = pc.plain(oracle, name)
    raw4 = np.zeros((len(base["hit_idx"]), 4), np.float32)
    raw4[:, :3] = oc.hit_xyz_of(b.hb, base)[:, :3]
    raw = bv.box_vertical_host(raw4, base["hit_off"], len(raw4), exp["box"], exp["flags"], b.classes.prior_wlh, V.q_bot, V.q_top, V.min_points, V.lo, V.hi)
    assert not np.array_equal(_bits(raw["vert_z"]), _bits(vert["vert_z"]))      # the raw lists would give other order statistics


@pytest.mark.parametrize("name,cluster", [("nusc", None), ("waymo", None), ("nusc", C)])
def test_with_the_yaw_fit(oracle, name, cluster):
    """The fit sees the exclusive lists (the clustered exclusive ones behind a clustering)."""
    b = pc.batch(name)
    front = pc.expected_of(oracle, name, cluster=cluster)
    as_lists = front if cluster is not None else dict(front, cl_off=front["ow_off"], cl_xyz=front["ow_xyz"])       # (what yaw_fit_pass_cases.fitted fits)
    exp = yc.fitted(oracle, b, as_lists, Y)
    if cluster is None:
        exp = {k: v for k, v in exp.items() if k not in ("cl_off", "cl_xyz")}
        raw_fit = yc.fitted(oracle, b, pc.plain(oracle, name), Y)
        assert not np.array_equal(exp["fit_rect"], raw_fit["fit_rect"])                # the ownership changes what is fitted
    eng = _engine(b, owner=O, yaw=Y, cluster=cluster)
    got = _run(eng, b.hb)
    _check_fitted(b, got, exp, front)
    _check_owner(eng, got, exp)


def test_with_every_other_stage_on(oracle):
    """Strip, clustering, yaw fit, placement, rotated NMS, velocity, tracks, size, vertical and ground stage on the moving scenes of
    tests/box_size_pass_cases.py: the ownership's outputs are the host statement's on the oracle's lists, the strip's the host
    statement's on the exclusive lists, the clustering's on the stripped ones, the fit's on the clustered ones, the vertical stage's
    status and order statistics too -- each stage reads the lists the header says it reads."""
    from cm3d_amd import boxground as bg
    from cm3d_amd import nms as nmsmod
    from cm3d_amd import tracks as T
    b = sp.batch()
    kw = dict(strip=S, cluster=C, yaw=sp.Y, place=sp.P, nms=nmsmod.RotatedNms(class_agnostic=True), velocity=vc.settings()[0],
              tracks=T.Tracks(2, "mean", 2), size=sp.S, vertical=V, ground=bg.BoxGround())
    front = oc._frozen(oc.oracle_batch(oracle, b.frames, b.lanes, b.frame_lane, b.hb))
    exp = pc.expected(oracle, b, front, strip=S, cluster=C)
    eng = _engine(b, owner=O, **kw)
    got = _run(eng, b.hb)
    _check_owner(eng, got, exp)
    _check_strip(eng, got, exp)
    print(f"moving scenes: {int((exp['ow_lost'] > 0).sum())} masks lose {int(exp['ow_lost'].sum())} positions")
    for key in ("cl_off", "cl_status", "cl_idx", "medoid_pos"):
        assert np.array_equal(got[key], exp[key]), key
    assert got["cl_xyz"].tobytes() == np.ascontiguousarray(exp["cl_xyz"], np.float32).tobytes()
    assert np.array_equal(got["centroid"].view(np.uint32), exp["centroid"].view(np.uint32))
    fit_k, fit_rect, fit_status = bevfit.bev_fit_lists(exp["cl_off"], exp["cl_xyz"], sp.Y.angles, sp.Y.d0, sp.Y.min_points, sp.Y.min_length)
    assert np.array_equal(got["fit_k"], fit_k) and np.array_equal(got["fit_status"], fit_status) and np.array_equal(_bits(got["fit_rect"]), _bits(fit_rect))
    xyz, off = pc.read_lists(exp)
    vert = bv.box_vertical_host(xyz, off, len(xyz), got["box"], got["flags"], b.classes.prior_wlh, V.q_bot, V.q_top, V.min_points, V.lo, V.hi)
    assert np.array_equal(got["vert_status"], vert["vert_status"]) and np.array_equal(_bits(got["vert_z"]), _bits(vert["vert_z"]))
    base = _run(_engine(b, **kw), b.hb)
    assert set(got) == set(base) | set(pc.OW_KEYS) and got["hit_idx"].tobytes() == base["hit_idx"].tobytes()
    assert list(eng.b.timed)[:3] == ["owner", "strip", "cluster"]


@pytest.mark.parametrize("name", ["nusc", "waymo"])
def test_virtual_points_read_the_exclusive_lists(oracle, name):
    """The re-projection, the nearest return and src_idx are the exclusive lists': the host statement on ow_off and the re-projection
    of ow_xyz, and frame_records' src_idx out of ow_idx."""
    from cm3d_amd import lifting
    b = pc.batch(name)
    vset = vp.VirtualPoints(per_mask=24, seed=5, kept_only=False)
    eng = _engine(b, owner=O, virtual=vset)
    got = _run(eng, b.hb)
    exp = pc.expected_of(oracle, name)
    _check_owner(eng, got, exp)
    off, xyz, hb, e = got["ow_off"], got["ow_xyz"], b.hb, eng.b
    uvd = got["hit_uvd"]
    assert uvd.shape == (int(off[-1]), 4)
    cams = np.asarray(hb.cams, np.float32).reshape(e.F, hb.n_cams, -1)
    for m in range(e.M):
        rows = np.zeros((off[m + 1] - off[m], 4), np.float32)
        rows[:, :3] = xyz[off[m]:off[m + 1], :3]
        want = oracle.project_points(rows, cams[hb.mask_frame[m], hb.mask_cam[m]])
        assert np.array_equal(uvd[off[m]:off[m + 1], :3].view(np.uint32), np.ascontiguousarray(want, np.float32).view(np.uint32)), m
    host = vp.virtual_points_host(e.packed.cpu().numpy(), e.bbox.cpu().numpy(), e.W, e.H, cams, hb.mask_off, hb.mask_frame, hb.mask_cam,
                                  got["flags"], uvd, off, len(uvd), vset.per_mask, vset.seed, vset.max_px, vset.kept_only, hb.frame_seed)
    assert np.array_equal(got["vp_count"], host["vp_count"]) and np.array_equal(got["vp_status"], host["vp_status"])
    K, lost = vset.per_mask, np.flatnonzero(exp["ow_lost"] > 0)
    for m in range(e.M):
        n = int(host["vp_count"][m])
        assert np.array_equal(got["vp_src"][m * K:m * K + n], host["vp_src"][m * K:m * K + n]), m
        assert (got["vp_src"][m * K:m * K + n] < off[m + 1] - off[m]).all()
    assert host["vp_count"][lost].sum() > 0
    frames = lifting.virtual_point_frames(eng)
    for f, rec in enumerate(frames):
        if rec is None:
            continue
        for j in range(len(rec["src_idx"])):
            m = int(hb.mask_off[f]) + int(rec["mask"][j])
            assert rec["src_idx"][j] in exp["ow_idx"][off[m]:off[m + 1]]
    assert any(r is not None for r in frames)


def test_pipeline_rerun_with_two_different_batches_in_flight_and_the_timer_pair(oracle):
    import torch
    from cm3d_amd import lifting
    # (the engines of one pipeline share a class table: the second batch is the nuScenes batch's frames 2 and 3)
    b0, b1 = pc.batch("nusc"), bgc.pass_batch("nusc", first=2)
    exp0 = pc.expected_of(oracle, "nusc", cluster=C)
    exp1 = pc.expected(oracle, b1, oc._frozen(oc.oracle_batch(oracle, b1.frames, b1.lanes, b1.frame_lane, b1.hb)), cluster=C)
    assert not np.array_equal(exp0["ow_off"], exp1["ow_off"])
    pipe = lifting.LiftPipeline("cuda:0", depth=2, classes=b0.classes, owner=O, cluster=C)
    ev = []
    slots = [pipe.submit(b0.hb, "rle", stage_events=ev), pipe.submit(b1.hb, "rle")]
    assert len(ev) == 9 and not pipe.engines[0].b.plain_pass          # the plain pass's five events, the ownership's pair, the clustering's pair
    assert list(pipe.engines[0].b.timed) == ["owner", "cluster"] and all(e.owner == O for e in pipe.engines)
    before = pipe.native_passes
    for s in slots:
        pipe.rerun(s)
    pipe.rerun(slots[0])
    assert pipe.native_passes == before + 3                           # `rerun` took its Python branch: cm3d_pipe_submit knows the plain pass only
    for s, exp in zip(slots, (exp0, exp1)):
        got = pipe.collect(s, full=False)[1]
        torch.cuda.synchronize()
        for k in ("ow_off", "ow_status", "ow_lost", "cl_off", "medoid_pos"):
            assert np.array_equal(got[k], exp[k]), (s, k)
        full = pipe.engines[s].download(full=True)
        assert np.array_equal(full["ow_owner"], exp["ow_owner"]) and np.array_equal(full["ow_idx"], exp["ow_idx"])
    assert ev[5].elapsed_time(ev[6]) >= 0.0 and ev[6].elapsed_time(ev[7]) >= 0.0 and ev[7].elapsed_time(ev[8]) >= 0.0


@pytest.mark.parametrize("name", ["nusc", "waymo"])
def test_without_the_option_nothing_changes(name):
    from cm3d_amd import lifting
    b = pc.batch(name)
    without, off = _engine(b), _engine(b, owner=None)
    _same_bytes(_run(without, b.hb), _run(off, b.hb))
    assert off.owner is None and off.b.plain_pass and not any(hasattr(off.b, k) for k in OW_BUFFERS) and "owner" not in off.b.timed
    stripped = _engine(b, strip=S)
    got = _run(stripped, b.hb)
    assert not any(hasattr(stripped.b, k) for k in OW_BUFFERS) and list(stripped.b.timed) == ["strip"]
    assert set(got) == set(_run(without)) | set(GS_KEYS)             # exactly the keys it downloaded before
    on = _engine(b, owner=O)
    on.upload(b.hb)
    assert all(hasattr(on.b, k) for k in OW_BUFFERS) and not on.b.plain_pass and on.b.points is None
    with pytest.raises(ValueError, match="KITTI"):
        lifting.LiftEngine("cuda:0", classes=b.classes, obb=True, owner=O)


# ------------------------------------------------------------------------------------------------ the entry points
def _host_rows(hb, got, owner, P):
    """The painted cloud of every frame by the host statement of the ownership on the downloaded raw lists and flags."""
    res = po.point_owner_host(got["hit_idx"], got["hit_off"], hb.mask_off, hb.score, P, owner.rule, owner.min_keep)
    assert np.array_equal(res["ow_owner"], got["ow_owner"])
    return [po.label_rows(f, got["hit_idx"], got["hit_xyz"], got["hit_off"], hb.mask_off, res["ow_owner"], hb.mask_cam, hb.class_id, hb.score,
                          got["flags"], P) for f in range(hb.n_frames)]


def _check_label_files(directory, stems, rows):
    """Every frame with a listed point has its file, equal to the host rows array by array; no other file exists."""
    written = 0
    for stem, want in zip(stems, rows):
        path = os.path.join(directory, f"{stem}.npz")
        if not len(want["idx"]):
            assert not os.path.exists(path), stem
            continue
        z = np.load(path, allow_pickle=False)
        assert tuple(z.files) == po.LABEL_FIELDS
        for k in po.LABEL_FIELDS:
            assert z[k].dtype == want[k].dtype and z[k].shape == want[k].shape and z[k].tobytes() == want[k].tobytes(), (stem, k)
        written += 1
    assert written and sorted(os.listdir(directory)) == sorted(f"{s}.npz" for s, w in zip(stems, rows) if len(w["idx"]))
    return written


def test_nuscenes_entry_point(tmp_path):
    """src/nuscenes/2d_to_3d.py --point-owner score on scenes written to disk, both host routes: the file is the text writer's for the
    records of an engine with the option on the batch packed from the same files; --point-owner off writes the bytes of no flag; with
    --point-labels every frame's file holds the host statement's rows."""
    from cm3d_amd import lifting
    from cm3d_amd.pipeline_nuscenes import META
    dataroot, mask_dir, names = sp.write_dataset(tmp_path)
    env = dict(os.environ, CM3D_VER_NAME="v1.0-synth", CM3D_INPUT_PATH=dataroot, CM3D_INPUT_DIR=mask_dir)
    runs = {"none": (), "off": ("--point-owner", "off"),
            "native": ("--point-owner", "score", "--point-labels", str(tmp_path / "labels_native")),
            "python": ("--point-owner", "score", "--point-labels", str(tmp_path / "labels_python"), "--reader-threads", "-1")}
    out = {}
    for key, flags in runs.items():
        r = subprocess.run([sys.executable, "2d_to_3d.py", "--ratio", str(sp.config().ratio), *flags], cwd=os.path.join(ROOT, "src", "nuscenes"),
                           env=dict(env, CM3D_OUTPUT_DIR=str(tmp_path / key)), capture_output=True, text=True, timeout=300)
        assert r.returncode == 0, r.stderr[-2000:]
        out[key] = open(tmp_path / key / "pseudolabels_minival.json", "rb").read()
        assert ("owner :" in r.stdout) == (key in ("native", "python"))                   # the timers' bucket
    assert out["off"] == out["none"] and out["native"] == out["python"]
    r = subprocess.run([sys.executable, "2d_to_3d.py", "--point-owner-min-keep", "3"], cwd=os.path.join(ROOT, "src", "nuscenes"), env=env,
                       capture_output=True, text=True, timeout=300)
    assert r.returncode == 2 and "--point-owner-min-keep needs --point-owner" in r.stderr
    hb = sp.dataset_batch(dataroot, mask_dir, names)
    classes = lifting.ClassTable.nuscenes()
    ids = np.stack([np.arange(hb.n_frames), np.zeros(hb.n_frames)], 1)
    text = {}
    for key, kw in (("none", {}), ("native", dict(owner=po.PointOwner()))):
        eng = lifting.LiftEngine("cuda:0", classes=classes, **kw)
        got = _run(eng, hb)
        rec = lifting.kept_box_records(eng.b, ids).cpu().numpy()
        text[key], n = lifting.nuscenes_results_json(rec, hb.tokens, classes, dict(META))
        assert n == len(rec)
    print(f"dataset: {int((got['ow_lost'] > 0).sum())} masks lose {int(got['ow_lost'].sum())} positions")
    assert out["native"] == text["native"].encode() and out["none"] == text["none"].encode()
    assert (out["native"] != out["none"]) == (text["native"] != text["none"])
    rows = _host_rows(hb, got, po.PointOwner(), eng.b.max_pts)
    assert max(int(r["claims"].max()) for r in rows if len(r["idx"])) >= 2                # the scenes do contest points
    for route in ("native", "python"):
        _check_label_files(str(tmp_path / f"labels_{route}"), hb.tokens, rows)


def test_waymo_entry_point(tmp_path):
    """src/waymo/2d_to_3d.py --point-owner smallest: the file is objects_from_results' for an engine with the option; --point-owner off
    writes the bytes of no flag; the painted cloud of every frame is the host statement's, in DIR/<scene>/<frame file's stem>.npz."""
    from tests.test_gpu_entrypoint import _write_waymo_scene
    from cm3d_amd import lifting, pipeline_waymo as pw, waymo as wm
    scene = "segment-synthetic-0"
    _write_waymo_scene(tmp_path, scene, 0, 3)
    args = ["--frames-dir", str(tmp_path / "frames"), "--mask-dir", str(tmp_path / "masks")]
    own = ["--point-owner", "smallest", "--point-owner-min-keep", "1", "--point-labels", str(tmp_path / "labels")]
    blobs = {}
    for key, extra in (("plain", []), ("off", ["--point-owner", "off"]), ("own", own)):
        p = subprocess.run([sys.executable, "2d_to_3d.py", *args, "--output", str(tmp_path / f"{key}.bin"), *extra],
                           cwd=os.path.join(ROOT, "src", "waymo"), capture_output=True, text=True, timeout=300)
        assert p.returncode == 0, p.stderr[-2000:]
        blobs[key] = open(tmp_path / f"{key}.bin", "rb").read()
    p = subprocess.run([sys.executable, "2d_to_3d.py", *args, "--output", str(tmp_path / "bad.bin"), "--point-labels", str(tmp_path / "x")],
                       cwd=os.path.join(ROOT, "src", "waymo"), capture_output=True, text=True, timeout=300)
    assert p.returncode == 2 and "--point-labels needs --point-owner" in p.stderr and not os.path.exists(tmp_path / "x")
    assert blobs["off"] == blobs["plain"]
    frames, lanes = pw.load_scene(str(tmp_path / "frames"), str(tmp_path / "masks"), scene)
    classes = lifting.ClassTable.waymo()
    hb = lifting.pack_frames(frames, [lanes], [0] * len(frames), classes)
    meta = [(f.context_name, f.timestamp_micros) for f in frames]
    enc, small = {}, po.PointOwner("smallest", 1)
    for key, kw in (("plain", {}), ("own", dict(owner=small))):
        eng = lifting.LiftEngine("cuda:0", classes=classes, **kw)
        got = _run(eng, hb)
        enc[key] = wm.encode_objects(wm.objects_from_results(hb, got, classes, meta))
    assert blobs["own"] == enc["own"] and blobs["plain"] == enc["plain"]
    assert (blobs["own"] != blobs["plain"]) == (enc["own"] != enc["plain"]) and got["ow_status"].size > 0
    stems = [f"{int(f.token.rsplit(':', 1)[1])}_frame" for f in frames]
    _check_label_files(str(tmp_path / "labels" / scene), stems, _host_rows(hb, got, small, eng.b.max_pts))
