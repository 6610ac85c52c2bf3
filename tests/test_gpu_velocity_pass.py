"""GPU: the velocity stage behind the pass (LiftEngine(velocity=...), cm3d_box_velocity behind cm3d_lift_pass_opt) on the moving
scenes of tests/velocity_pass_cases.py, and the nuScenes entry point with --velocity track on the same scenes written to disk.

(a) the device's outputs equal velocity.track_velocity_host applied to the device's own downloaded box / flags, to the bit;
(b) against the expectation composed on the CPU from the oracle's pass alone, matches and vel_src are exact and vel lies within
    BOX_TOL * 2 / dt: a velocity is a difference of two centres, each within test_gpu_parity's BOX_TOL of the oracle's, over a span of
    at least dt.  The builder (velocity_pass_cases.assert_robust) asserts that BOX_TOL cannot change a decision.
"""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

from tests import velocity_pass_cases as pc

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
VEL_KEYS = ("next_match", "prev_match", "vel_src", "vel")
VEL_TOL = pc.BOX_TOL * 2 / pc.DT


def _run(eng, hb, graph=False):
    import torch
    eng.upload(hb)
    eng.run(masks="rle")
    torch.cuda.synchronize()
    if graph:
        first = eng.download()
        for k in VEL_KEYS:                                   # poison: the replay has to write them again
            getattr(eng.b, k).fill_(-3)
        g = eng.capture_graph(masks="rle")
        g.replay()
        torch.cuda.synchronize()
        return first, eng.download()
    return eng.download()


def _assert_statement(hb, got):
    """(a): the device against the host statement on the device's own boxes."""
    host = pc.host_velocity(hb, got["box"], got["flags"])
    for k in ("next_match", "prev_match", "vel_src"):
        assert np.array_equal(got[k], host[k]), k
    assert got["vel"].tobytes() == host["vel"].tobytes()
    assert host["status"] == 0
    return host


def _assert_composed(got, exp_vel):
    """(b): matches and vel_src exact, velocities within VEL_TOL of the CPU composition."""
    for k in ("next_match", "prev_match", "vel_src"):
        assert np.array_equal(got[k], exp_vel[k]), k
    err = np.abs(got["vel"] - exp_vel["vel"]).max()
    print(f"max |vel - composed| = {err:.3e} (bound {VEL_TOL:.1e})")
    assert err <= VEL_TOL


@pytest.fixture(scope="module")
def plain():
    from cm3d_amd import lifting
    return _run(lifting.LiftEngine("cuda:0"), pc.batch().hb)


@pytest.fixture(scope="module")
def tracked():
    from cm3d_amd import lifting
    return _run(lifting.LiftEngine("cuda:0", velocity=pc.settings()[0]), pc.batch().hb)


def test_engine_equals_host_statement_and_cpu_composition(tracked):
    b = pc.batch()
    exp, exp_vel = pc.expected()
    assert np.array_equal(tracked["flags"], exp["flags"]) and np.allclose(tracked["box"], exp["box"], rtol=0, atol=pc.BOX_TOL)
    _assert_statement(b.hb, tracked)
    _assert_composed(tracked, exp_vel)
    moving = pc.check_known_velocities(b.hb, tracked["flags"], tracked["medoid_pos"], tracked, VEL_TOL)
    assert moving.sum() >= 12


def test_without_the_option_every_buffer_is_what_it_was(plain, tracked):
    from cm3d_amd import lifting
    assert not set(VEL_KEYS) & set(plain) and set(plain) | set(VEL_KEYS) == set(tracked)
    for k, v in plain.items():
        assert v.tobytes() == tracked[k].tobytes(), k
    eng = lifting.LiftEngine("cuda:0", velocity=None)
    eng.upload(pc.batch().hb)
    assert eng.velocity is None and not hasattr(eng.b, "vel") and not hasattr(eng.b, "vel_ws")


def test_option_needs_the_frame_links():
    import dataclasses
    from cm3d_amd import lifting
    hb = dataclasses.replace(pc.batch().hb, frame_next=None, frame_time=None)
    with pytest.raises(ValueError, match="frame_next and frame_time"):
        lifting.LiftEngine("cuda:0", velocity=pc.settings()[0]).upload(hb)


def test_behind_the_rotated_nms(plain):
    """The stage sees the kept set the rotated NMS leaves: composed on the CPU from the oracle's boxes and nms.rotated_nms_host."""
    from cm3d_amd import lifting, nms as nmsmod
    from tests import optin_pass_cases as oc
    b = pc.batch()
    exp, _ = pc.expected()
    r = nmsmod.RotatedNms(measure="cover", class_agnostic=True, thr=0.0)
    keep = oc.rotated_keep(exp["box"], exp["flags"], b.hb, r)
    flags = (exp["flags"] & 1) | (keep << 1)
    assert (flags != exp["flags"]).any()                                  # the NMS decides something else than the circle NMS
    pc.assert_robust(b.hb, exp["box"], flags)
    got = _run(lifting.LiftEngine("cuda:0", nms=r, velocity=pc.settings()[0]), b.hb)
    assert np.array_equal(got["flags"], flags)
    _assert_statement(b.hb, got)
    _assert_composed(got, pc.host_velocity(b.hb, exp["box"], flags))


def test_behind_all_four_options_at_once():
    """Clustering, lane filter, yaw fit and rotated NMS on: the pass's buffers are those of the same engine without the stage, the
    stage equals the host statement on the box rows and flags that pass left, and the CPU composition of all five holds."""
    from cm3d_amd import lifting
    b, kw = pc.batch(), pc.all_four_options()
    box, flags, exp_vel = pc.expected_all_four()
    base = _run(lifting.LiftEngine("cuda:0", **kw), b.hb)
    got = _run(lifting.LiftEngine("cuda:0", velocity=pc.settings()[0], **kw), b.hb)
    for k, v in base.items():
        assert v.tobytes() == got[k].tobytes(), k
    assert {"cl_off", "medoid_pos_kept", "yaw_src"} <= set(got)
    assert np.array_equal(got["flags"], flags)
    keep = (flags & 3) == 3
    assert np.allclose(got["box"][keep][:, :2], box[keep][:, :2], rtol=0, atol=pc.BOX_TOL)
    _assert_statement(b.hb, got)
    _assert_composed(got, exp_vel)
    assert (exp_vel["vel_src"] > 0).sum() >= 12


def test_captured_graph_gives_the_same_bytes(tracked):
    from cm3d_amd import lifting
    first, replayed = _run(lifting.LiftEngine("cuda:0", velocity=pc.settings()[0]), pc.batch().hb, graph=True)
    for k in VEL_KEYS + ("box", "flags"):
        assert first[k].tobytes() == tracked[k].tobytes() == replayed[k].tobytes(), k


def test_pipeline_rerun_and_kept_velocities(tracked):
    """LiftPipeline with the option: `rerun` takes its Python branch (the stage runs again), and kept_box_velocities are the rows of
    kept_box_records' masks in its order."""
    import torch
    from cm3d_amd import lifting
    hb = pc.batch().hb
    pipe = lifting.LiftPipeline("cuda:0", depth=1, velocity=pc.settings()[0])
    slot = pipe.submit(hb, "rle")
    pipe.check_status(slot)
    before = pipe.native_passes
    pipe.engines[slot].b.vel.fill_(float("nan"))
    pipe.rerun(slot)
    ids = np.stack([np.arange(hb.n_frames), np.zeros(hb.n_frames)], 1)
    rec = pipe.collect_records(slot, ids).cpu().numpy()
    vel = lifting.kept_box_velocities(pipe.engines[slot].b).cpu().numpy()
    torch.cuda.synchronize()
    keep = (tracked["flags"] & 3) == 3
    assert pipe.native_passes == before + 1 and rec.shape[0] == keep.sum()
    assert vel.tobytes() == tracked["vel"][keep].tobytes() and np.array_equal(rec[:, :2], tracked["box"][keep][:, :2])


# ------------------------------------------------------------------------------------------------ the entry point
def _write_dataset(tmp_path, monkeypatch):
    """The two moving scenes in the reference's on-disk formats (velocity_pass_cases.write_dataset), the one-yaw lane table for both
    map locations."""
    return pc.write_dataset(tmp_path, n_scenes=2)


def _entry_point(dataroot, mask_dir, out_dir, *flags):
    env = dict(os.environ, CM3D_VER_NAME="v1.0-synth", CM3D_INPUT_PATH=dataroot, CM3D_INPUT_DIR=mask_dir, CM3D_OUTPUT_DIR=str(out_dir))
    r = subprocess.run([sys.executable, "2d_to_3d.py", "--ratio", str(pc.config().ratio), *flags], cwd=os.path.join(ROOT, "src", "nuscenes"),
                       env=env, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-2000:]
    return open(os.path.join(out_dir, "pseudolabels_minival.json"), "rb").read()


def test_entry_point_writes_the_velocities_on_both_host_routes(tmp_path, monkeypatch):
    """--velocity track through the native reader and through the Python reader: identical files, which hold the velocities an engine
    computes on the batch packed from the same files -- the moving scene's stable boxes at VELOCITY[0] within VEL_TOL."""
    from cm3d_amd import lifting, nusc_io
    dataroot, mask_dir, names = _write_dataset(tmp_path, monkeypatch)
    flags = ("--velocity", "track", "--velocity-max-speed", ",".join(f"{n}={pc.MAX_SPEED}" for n in sorted(_class_names())))
    native = _entry_point(dataroot, mask_dir, tmp_path / "native", *flags)
    python = _entry_point(dataroot, mask_dir, tmp_path / "python", "--reader-threads", "-1", *flags)
    assert native == python
    tables = nusc_io.NuscTables("v1.0-synth", dataroot, annotations=False)
    frames = [f for n in names for f in nusc_io.frames_of_scene(tables, tables.scene_by_name(n), mask_dir, n_sweeps=3, ratio=pc.config().ratio)]
    hb = lifting.pack_frames(frames, [pc.lane_table()], [0] * len(frames))
    assert hb.frame_next.tolist() == [1, 2, -1, 4, 5, -1] and hb.frame_time.tolist() == [0.0, 0.5, 1.0, 0.0, 0.5, 1.0]
    got = _run(lifting.LiftEngine("cuda:0", velocity=pc.settings()[0]), hb)
    _assert_statement(hb, got)
    results = json.loads(native)["results"]
    assert list(results) == hb.tokens
    boxes = [b for bs in results.values() for b in bs]
    keep = (got["flags"] & 3) == 3
    assert len(boxes) == keep.sum() and all(type(v) is float for b in boxes for v in b["velocity"])
    written = np.array([b["velocity"] for b in boxes], np.float64)
    assert np.array([b["translation"][:2] for b in boxes]).tobytes() == np.ascontiguousarray(got["box"][keep][:, :2]).tobytes()
    assert written.tobytes() == got["vel"][keep].tobytes()                  # repr round-trips: what the stage computed, to the bit
    moving = pc.check_known_velocities(hb, got["flags"], got["medoid_pos"], got, VEL_TOL)[keep]
    scene0 = (hb.mask_frame < pc.FRAMES_PER_SCENE)[keep]
    assert (moving & scene0).sum() >= 6 and np.abs(written[moving & scene0] - pc.VELOCITY[0]).max() <= VEL_TOL


def test_entry_point_velocity_none_writes_the_bytes_of_no_flag(tmp_path, monkeypatch):
    dataroot, mask_dir, _ = _write_dataset(tmp_path, monkeypatch)
    assert _entry_point(dataroot, mask_dir, tmp_path / "a") == _entry_point(dataroot, mask_dir, tmp_path / "b", "--velocity", "none")
    assert b'"velocity": [0, 0]' in open(tmp_path / "a" / "pseudolabels_minival.json", "rb").read()


def _class_names():
    from cm3d_amd import lifting
    return lifting.ClassTable.nuscenes().names
