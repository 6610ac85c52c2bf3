"""GPU: a multi-batch job through the nuScenes entry point with EVERY opt-in stage on -- depth clustering, lane and drivable-area filter,
yaw fit, rotated NMS, velocity -- on five scenes of three moving frames (tests/velocity_pass_cases.py), every scene with its own map
location: its own lane table (one yaw per scene) and its own drivable square, so ten entries go through the engines' cache of eight.

However the job is cut into batches (five of one scene through the depth-2 pipeline and five streamed parts; one batch; three
batches from the Python reader, the last of one scene; two ranks and one gather), it writes the same bytes -- those of lone
five-option engines scene by scene.  No tolerance: the kernels are deterministic by their own statement."""
import contextlib
import io
import json
import os
import subprocess
import sys

import numpy as np
import pytest

from tests import velocity_pass_cases as pc

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PRIORS = os.path.join(ROOT, "src", "nuscenes", "cfg", "shape_priors_chatgpt.json")
N_SCENES = 5
LANE_YAWS = (pc.LANE_YAW, 0.9, -0.6, 1.7, 2.4)           # one per map location: another scene's lanes show in every pushed box
ROAD_HALF = (60.0, 45.0, 30.0, 75.0, 50.0)                # half side of each location's drivable square
VEL_TOL = pc.BOX_TOL * 2 / pc.DT                          # tests/test_gpu_velocity_pass.py


def _flags():
    from cm3d_amd import lifting
    speeds = ",".join(f"{n}={pc.MAX_SPEED}" for n in sorted(lifting.ClassTable.nuscenes().names))
    # the values of velocity_pass_cases.all_four_options() and settings(), with the drivable-area test
    return ["--depth-cluster", "1", "--depth-cluster-min-points", "3", "--lane-max-dist", "2.5", "--drivable-filter", "--yaw", "fit",
            "--yaw-fit-min-points", "5", "--nms", "rotated", "--nms-overlap", "cover", "--nms-class-agnostic", "--nms-thr", "0",
            "--velocity", "track", "--velocity-max-speed", speeds]


@pytest.fixture(scope="module")
def dataset(tmp_path_factory):
    root = tmp_path_factory.mktemp("optin_job")
    dataroot, mask_dir, names = pc.write_dataset(root, n_scenes=N_SCENES, lane_yaws=LANE_YAWS, road_half=ROAD_HALF)
    return root, dataroot, mask_dir, names


def _argv(dataset, out, *extra):
    root, dataroot, mask_dir, names = dataset
    return ["--version", "v1.0-synth", "--dataroot", dataroot, "--mask-dir", mask_dir, "--output-dir", str(root / out), "--priors", PRIORS,
            "--scenes", ",".join(names), "--ratio", str(pc.config().ratio), *extra]


def _job(dataset, out, *extra):
    """pipeline_nuscenes.main in this process (one rank): (the file's bytes, what it printed)."""
    from cm3d_amd import pipeline_nuscenes as pn
    text = io.StringIO()
    with contextlib.redirect_stdout(text):
        assert pn.main(_argv(dataset, out, *extra)) == 0
    return open(dataset[0] / out / pn.OUTPUT_NAME, "rb").read(), text.getvalue()


@pytest.fixture(scope="module")
def streamed(dataset):
    """Run 1: the native reader, one scene per batch -- five batches through depth 2, five streamed parts."""
    return _job(dataset, "native1", "--reader-threads", "4", "--scenes-per-batch", "1", *_flags())


def _buckets(stdout):
    out = {}
    for line in stdout.splitlines():
        key, sep, v = line.partition(":")
        if sep:
            with contextlib.suppress(ValueError):
                out[key.strip()] = float(v)
    return out


def _lone_scenes(dataset):
    """Every scene by itself through a lone five-option engine, its frames packed from the written files: (HostBatch, download)."""
    import torch
    from cm3d_amd import eval_detection, lifting, nusc_io
    from tests import inflight_cases as ic
    _, dataroot, mask_dir, names = dataset
    tables = nusc_io.NuscTables("v1.0-synth", dataroot, annotations=False)
    classes = lifting.ClassTable.nuscenes(json.load(open(PRIORS)))
    out = []
    for s, name in enumerate(names):
        scene = tables.scene_by_name(name)
        frames = nusc_io.frames_of_scene(tables, scene, mask_dir, n_sweeps=3, ratio=pc.config().ratio)
        hb = lifting.pack_frames(frames, [pc.lane_table(LANE_YAWS[s])], [0] * len(frames), classes)
        hb.polygons = [eval_detection.load_drivable_polygons(dataroot, tables.location(scene))]
        assert hb.frame_next.tolist() == [1, 2, -1] and hb.frame_time.tolist() == [0.0, 0.5, 1.0]
        eng = lifting.LiftEngine("cuda:0", classes=classes, **ic.five_options(True))
        eng.upload(hb)
        eng.run(masks="rle")
        torch.cuda.synchronize()
        out.append((hb, eng.download(full=True), classes))
    return out


def test_one_rank_jobs_write_the_lone_engines_bytes_however_they_are_batched(dataset, streamed):
    from cm3d_amd import lifting
    native1, stdout = streamed
    native5, _ = _job(dataset, "native5", "--reader-threads", "4", "--scenes-per-batch", "5", *_flags())
    python2, _ = _job(dataset, "python2", "--reader-threads", "-1", "--scenes-per-batch", "2", *_flags())
    plain, _ = _job(dataset, "plain", "--reader-threads", "4", "--scenes-per-batch", "1")
    assert native1 == native5, "five batches in flight against one batch"
    assert native1 == python2, "the native reader against the Python reader in batches of 2, 2 and 1 scenes"
    assert native1 != plain and b'"velocity": [0, 0]' in plain and b'"velocity": [0, 0]' not in native1
    # ... and they are what lone engines give scene by scene
    results = json.loads(native1)["results"]
    lone = _lone_scenes(dataset)
    assert list(results) == [t for hb, _, _ in lone for t in hb.tokens] and len(results) == N_SCENES * pc.FRAMES_PER_SCENE
    moving_scenes = dropped_by_road = 0
    for s, (hb, got, classes) in enumerate(lone):
        keep = (got["flags"] & 3) == 3
        boxes = [b for t in hb.tokens for b in results[t]]
        assert len(boxes) == keep.sum() >= 3, s
        written = np.array([b["velocity"] for b in boxes], np.float64)
        assert np.array([b["translation"][:2] for b in boxes]).tobytes() == np.ascontiguousarray(got["box"][keep][:, :2]).tobytes(), s
        assert written.tobytes() == got["vel"][keep].tobytes(), s
        want = lifting.box_records(hb, got, classes)
        vels = iter(got["vel"][keep].tolist())
        for t in hb.tokens:
            for b in want[t]:
                b["velocity"] = next(vels)
        assert {t: results[t] for t in hb.tokens} == want, s
        moving_scenes += int((np.abs(written) > 0).any())
        has = got["medoid_pos"] >= 0
        dropped_by_road += int((has & (got["on_road"] == 0) & (got["medoid_pos_kept"] < 0)).sum())
        if s == 0:
            # scene 0 moves at VELOCITY[0]: every kept, matched box whose discrete decisions -- medoid, source of the yaw, fitted
            # direction -- are the same in all three frames is the same physical box moved by exactly D per frame
            per = lambda a: np.asarray(a).reshape(pc.FRAMES_PER_SCENE, -1)
            same = (per(got["medoid_pos"]) >= 0).all(0)
            for key in ("medoid_pos", "yaw_src", "fit_k"):
                same &= (per(got[key]) == per(got[key])[0]).all(0)
            stable = np.tile(same, pc.FRAMES_PER_SCENE) & keep & (got["vel_src"] > 0)
            err = np.abs(got["vel"][stable] - pc.VELOCITY[0]).max()
            print(f"scene 0: {int(stable.sum())} stable boxes, max |vel - VELOCITY[0]| = {err:.3e} (bound {VEL_TOL:.1e})")
            assert stable.sum() >= 6 and err <= VEL_TOL
    assert moving_scenes >= 3 and dropped_by_road >= 1
    # the job's timer: every opt-in stage's bucket was filled from the eleven events of a pass
    t = _buckets(stdout)
    print({k: t.get(k) for k in ("medoid", "cluster", "yawfit", "drivable")})
    assert t["cluster"] > 0 and t["yawfit"] > 0 and t["drivable"] > 0 and t["medoid"] >= 0


def test_two_ranks_gather_the_velocities_beside_the_records(dataset, streamed):
    """Two ranks (gloo, both on the one device) shard the five scenes, one scene per batch; rank 0 gathers records and velocity rows
    and writes the bytes of the one-rank job."""
    root, dataroot, mask_dir, names = dataset
    env = dict(os.environ, CM3D_DIST_BACKEND="gloo", CM3D_SINGLE_DEVICE="1")
    r = subprocess.run([sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", "2", "--master-addr", "127.0.0.1",
                        "--master-port", "29723", "2d_to_3d.py", *_argv(dataset, "two", "--reader-threads", "4", "--scenes-per-batch", "1", *_flags())],
                       cwd=os.path.join(ROOT, "src", "nuscenes"), env=env, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-3000:]
    two = open(root / "two" / "pseudolabels_minival.json", "rb").read()
    assert two == streamed[0]
