"""GPU: LiftEngine(virtual=VirtualPoints(...)) on the two-frame nuScenes and Waymo batches of tests/yaw_fit_pass_cases.py -- alone, with
the clustering and the ground strip on, through LiftPipeline with two batches in flight and a rerun -- and both entry points on scenes
written to disk.

The expectation is virtualpoints.virtual_points_host on the engine's own masks, lists and flags, with the re-projection held against
the oracle's project_points; every other downloaded array is the bytes of the same engine without the option."""
import os
import subprocess
import sys

import numpy as np
import pytest

from cm3d_amd import cluster as clustermod
from cm3d_amd import groundstrip as gsmod
from cm3d_amd import virtualpoints as vp
from tests import yaw_fit_pass_cases as yc
from tests.test_gpu_optin_passes import _run

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
V = vp.VirtualPoints(per_mask=24, seed=5)
WIDTH = {"vp_xyz": 3, "vp_pix": 2, "vp_src": 1, "vp_depth": 1, "vp_d2": 1}


def _engine(b, **kw):
    from cm3d_amd import lifting
    return lifting.LiftEngine("cuda:0", classes=b.classes, **kw)


def _bits(a):
    a = np.ascontiguousarray(a)
    return a.view({4: np.uint32, 8: np.uint64}[a.dtype.itemsize])


def _lists(eng, got):
    if eng.cluster is not None:
        return got["cl_off"], got["cl_xyz"]
    if eng.strip is not None:
        return got["gs_off"], got["gs_xyz"]
    return got["hit_off"], got["hit_xyz"]


def _host(eng, got, uvd):
    """The host statement on what the engine holds: its masks, its flags, the lists the medoid saw and their re-projection `uvd`."""
    b, v = eng.b, eng.virtual
    hb = b.hb
    cams = np.asarray(hb.cams, np.float32).reshape(b.F, hb.n_cams, -1)
    return vp.virtual_points_host(b.packed.cpu().numpy(), b.bbox.cpu().numpy(), b.W, b.H, cams, hb.mask_off, hb.mask_frame, hb.mask_cam,
                                  got["flags"], uvd, _lists(eng, got)[0], len(uvd), v.per_mask, v.seed, v.max_px, v.kept_only, hb.frame_seed)


def _same_points(got, exp, K):
    assert np.array_equal(got["vp_count"], exp["vp_count"]) and np.array_equal(got["vp_status"], exp["vp_status"])
    for k, w in WIDTH.items():
        g, e = got[k].reshape(-1, w), exp[k].reshape(-1, w)
        assert got[k].dtype == exp[k].dtype and g.shape == e.shape, k
        for m in range(len(exp["vp_count"])):
            n = int(exp["vp_count"][m])
            assert np.array_equal(_bits(g[m * K:m * K + n]), _bits(e[m * K:m * K + n])), (k, m)


def _check(oracle, eng, got, base):
    """got: the engine with the option; base: the same engine without."""
    b = eng.b
    hb = b.hb
    assert set(got) == set(base) | set(vp.RESULTS) | {"hit_uvd"}
    for k in base:
        assert got[k].dtype == base[k].dtype and got[k].tobytes() == base[k].tobytes(), k
    off, xyz = _lists(eng, got)
    uvd = got["hit_uvd"]
    assert uvd.dtype == np.float32 and uvd.shape == (int(off[-1]), 4)
    cams = np.asarray(hb.cams, np.float32).reshape(b.F, hb.n_cams, -1)
    for m in range(b.M):                                                    # step 1: the oracle's chain through the mask's own camera
        rows = np.zeros((off[m + 1] - off[m], 4), np.float32)
        rows[:, :3] = xyz[off[m]:off[m + 1], :3]
        exp = oracle.project_points(rows, cams[hb.mask_frame[m], hb.mask_cam[m]])
        assert np.array_equal(_bits(uvd[off[m]:off[m + 1], :3]), _bits(exp)) and not uvd[off[m]:off[m + 1], 3].any(), m
    exp = _host(eng, got, uvd)
    _same_points(got, exp, eng.virtual.per_mask)
    kept = (got["flags"] & 3) == 3
    empty = (np.diff(off) == 0) | (b.bbox.cpu().numpy()[:, 0] > b.bbox.cpu().numpy()[:, 2])
    if eng.virtual.kept_only:
        assert np.array_equal(exp["vp_status"] == 1, ~kept) and exp["vp_count"][kept].sum() > eng.virtual.per_mask
    else:
        assert set(exp["vp_status"]) <= {0, 2} and np.array_equal(exp["vp_status"] == 2, empty)
    print(f"{b.M} masks, {int(kept.sum())} kept, {int(exp['vp_count'].sum())} points, statuses {np.bincount(exp['vp_status'], minlength=5).tolist()}")
    return exp


@pytest.mark.parametrize("name", ["nusc", "waymo"])
def test_the_engine_equals_the_host_statement_on_its_own_lists(oracle, name):
    import torch
    b = yc.batch(name)
    base = _run(_engine(b), b.hb)
    eng = _engine(b, virtual=V)
    got = _run(eng, b.hb)
    exp = _check(oracle, eng, got, base)
    # a second pass rewrites the same bytes; the stage alone on what the pass left does too
    for k in vp.RESULTS:
        getattr(eng.b, k).fill_(-3)
    again = _run(eng)
    _same_points(again, exp, V.per_mask)
    eng.b.vp_count.fill_(-3)
    eng.stage_virtual(torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    _same_points(eng.download(full=False), exp, V.per_mask)
    assert not eng.b.plain_pass


def test_with_the_clustering_and_the_ground_strip_on(oracle):
    b = yc.batch("nusc")
    kw = dict(cluster=clustermod.DepthCluster(1.0, 20), strip=gsmod.GroundStrip())
    eng = _engine(b, virtual=vp.VirtualPoints(per_mask=24, seed=5, max_px=6.0, kept_only=False), **kw)
    got = _run(eng, b.hb)
    exp = _check(oracle, eng, got, _run(_engine(b, **kw), b.hb))
    assert not np.array_equal(got["cl_off"], got["hit_off"])                 # the lists the stage read are not the raw ones
    assert (exp["vp_count"] < 24).any()                                     # the pixel limit dropped samples


def test_two_batches_in_flight_and_a_rerun(oracle):
    import torch
    from cm3d_amd import lifting
    first, second = yc.batch("nusc"), yc.batch("nusc", first=2, n_frames=2)
    first.hb.frame_seed, second.hb.frame_seed = np.array([0, 1], np.uint32), np.array([2, 3], np.uint32)
    try:
        alone = []
        for b in (first, second):
            eng = _engine(b, virtual=V)
            alone.append(_run(eng, b.hb))                                   # one at a time
        pipe = lifting.LiftPipeline("cuda:0", depth=2, classes=first.classes, virtual=V)
        ev = []
        slots = [pipe.submit(first.hb, "rle", stage_events=ev), pipe.submit(second.hb, "rle")]
        assert len(ev) == 7 and not pipe.engines[0].b.plain_pass             # the plain pass's five events, then the stage's pair
        before = pipe.native_passes
        pipe.rerun(slots[0])
        assert pipe.native_passes == before + 1
        for s, exp in zip(slots, alone):
            got = pipe.collect(s, full=False)[1]
            torch.cuda.synchronize()
            _same_points(got, exp, V.per_mask)
        assert ev[5].elapsed_time(ev[6]) >= 0.0
        assert not np.array_equal(alone[0]["vp_pix"], alone[1]["vp_pix"])
    finally:
        first.hb.frame_seed = second.hb.frame_seed = None


def test_without_the_option_nothing_is_there():
    b = yc.batch("nusc")
    off = _engine(b, virtual=None)
    off.upload(b.hb)
    assert off.virtual is None and off.b.plain_pass and not any(hasattr(off.b, k) for k in vp.RESULTS + ("hit_uvd", "frame_seed"))
    from cm3d_amd import lifting
    kitti = lifting.LiftEngine("cuda:0", classes=b.classes, obb=True, virtual=V)          # a KITTI engine is not refused
    assert kitti.virtual is V


def _load(path):
    z = np.load(path)
    return {k: z[k] for k in z.files}


def _same_files(out_dir, names, frames):
    """The files of DIR against lifting.virtual_point_frames of the same frames: one file per frame with a point, no other."""
    want = {f"{n}.npz" for n, rec in zip(names, frames) if rec is not None}
    assert want and set(os.listdir(out_dir)) == want
    n = 0
    for name, rec in zip(names, frames):
        if rec is None:
            continue
        got = _load(os.path.join(out_dir, f"{name}.npz"))
        assert set(got) == {k for k, _ in vp.FILE_FIELDS}
        for k, dtype in vp.FILE_FIELDS:
            assert got[k].dtype == dtype and got[k].tobytes() == np.ascontiguousarray(rec[k], dtype).tobytes(), (name, k)
        n += len(got["depth"])
    return n


def test_nuscenes_entry_point_writes_the_engines_points_and_the_same_json(tmp_path):
    from cm3d_amd import lifting, nusc_io, synthetic as syn
    cfg = syn.config("tiny")
    dataroot, mask_dir, names = nusc_io.write_synthetic_dataset(str(tmp_path), cfg, n_scenes=2, frames_per_scene=3)
    env = dict(os.environ, CM3D_VER_NAME="v1.0-synth", CM3D_INPUT_PATH=dataroot, CM3D_INPUT_DIR=mask_dir)
    flags = ["--virtual-points-per-mask", "16", "--virtual-points-seed", "3"]
    runs = {"plain": ("2d_to_3d.py", []), "native": ("2d_to_3d.py", ["--virtual-points", str(tmp_path / "vp_native")] + flags),
            "workers": ("2d_to_3d_new.py", ["--workers", "2", "--scenes-per-batch", "1", "--virtual-points", str(tmp_path / "vp_workers")] + flags)}
    for key, (script, extra) in runs.items():
        r = subprocess.run([sys.executable, script, "--ratio", str(cfg.ratio), "--output-dir", str(tmp_path / key)] + extra,
                           cwd=os.path.join(ROOT, "src", "nuscenes"), env=env, capture_output=True, text=True, timeout=600)
        assert r.returncode == 0, r.stderr[-2000:]
    plain = open(tmp_path / "plain" / "pseudolabels_minival.json", "rb").read()
    assert open(tmp_path / "native" / "pseudolabels_minival.json", "rb").read() == plain
    assert open(tmp_path / "workers" / "pseudolabels_minival.json", "rb").read() == plain
    # the engine on the same files, scene by scene, every frame with its ordinal in the job as its seed word
    tables = nusc_io.NuscTables("v1.0-synth", dataroot)
    import json
    classes = lifting.ClassTable.nuscenes(json.load(open(os.path.join(ROOT, "src", "nuscenes", "cfg", "shape_priors_chatgpt.json"))))
    eng = lifting.LiftEngine("cuda:0", classes=classes, virtual=vp.VirtualPoints(16, 3))
    tokens, frames = [], []
    for name in names:
        scene = tables.scene_by_name(name)
        fr = nusc_io.frames_of_scene(tables, scene, mask_dir, n_sweeps=3, ratio=cfg.ratio)
        hb = lifting.pack_frames(fr, [nusc_io.load_lane_points(dataroot, tables.location(scene))], [0] * len(fr), classes)
        hb.frame_seed = np.arange(len(tokens), len(tokens) + len(fr), dtype=np.uint32)
        _run(eng, hb)
        frames += lifting.virtual_point_frames(eng)
        tokens += [f.token for f in fr]
    n = _same_files(tmp_path / "vp_native", tokens, frames)
    assert n == _same_files(tmp_path / "vp_workers", tokens, frames) and n > 100
    print(f"{len(tokens)} frames, {n} virtual points")


def test_waymo_entry_point_writes_the_engines_points(tmp_path):
    from cm3d_amd import lifting, pipeline_waymo as pw
    from tests.test_gpu_entrypoint import _write_waymo_scene
    scene = "segment-synthetic-0"
    _write_waymo_scene(tmp_path, scene, 0, 2)
    outs = {}
    for key, extra in (("plain", []), ("vp", ["--virtual-points", str(tmp_path / "vp"), "--virtual-points-per-mask", "16"])):
        out = tmp_path / key / "pred.bin"
        r = subprocess.run([sys.executable, "2d_to_3d.py", "--frames-dir", str(tmp_path / "frames"), "--mask-dir", str(tmp_path / "masks"),
                            "--output", str(out)] + extra, cwd=os.path.join(ROOT, "src", "waymo"), capture_output=True, text=True, timeout=600)
        assert r.returncode == 0, r.stderr[-2000:]
        outs[key] = open(out, "rb").read()
    assert outs["plain"] == outs["vp"]
    frames, lanes = pw.load_scene(str(tmp_path / "frames"), str(tmp_path / "masks"), scene)
    import json
    classes = lifting.ClassTable.waymo(json.load(open(os.path.join(ROOT, "src", "waymo", "cfg", "shape_priors_chatgpt.json"))))
    hb = lifting.pack_frames(frames, [lanes], [0] * len(frames), classes)
    hb.frame_seed = np.arange(len(frames), dtype=np.uint32)                 # scene 0: scene_index * 65536 + the frame's number
    eng = lifting.LiftEngine("cuda:0", classes=classes, virtual=vp.VirtualPoints(16))
    _run(eng, hb)
    assert _same_files(tmp_path / "vp" / scene, [f"{k}_frame" for k in range(len(frames))], lifting.virtual_point_frames(eng)) > 20
