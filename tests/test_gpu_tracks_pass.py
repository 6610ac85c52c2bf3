"""GPU: the track stage behind the velocity stage (LiftEngine(velocity=..., tracks=...), cm3d_box_tracks behind cm3d_box_velocity) on
the moving scenes of tests/velocity_pass_cases.py, and the nuScenes entry point with the three track flags on the same scenes written
to disk with one mask that shows in a single frame.

(a) the device's outputs equal tracks.box_tracks_host applied to the arrays the same engine WITHOUT the stage leaves on the device
    (box, flags, next_match, prev_match: the stage's inputs), to the bit;
(b) against the composition on the CPU -- the oracle's pass, velocity.track_velocity_host, tracks.box_tracks_host -- ids, positions,
    lengths, flags and the rewritten scores are exact, and vel_smooth lies within the bound below.

The decisions of the stage read the boxes only through the matches (velocity_pass_cases.assert_robust: BOX_TOL cannot change one), the
flags and the scores (no arithmetic before the stage: the same bits on both sides); times come from the host.  So BOX_TOL cannot flip
an id, a position, a length, a flag or which scores are averaged; `composed` asserts the part of that which is a property of the data:
every link spans DT, far from the `>` of the rule, and every window has den > 0 by a wide margin.

The bound of vel_smooth is derived, not measured: vx = sum_j c_j x_j with c_j = (n t_j - St) / den, which depend on the frame times
alone, and x_j = box[j][0] - box[i][0], each centre within BOX_TOL of the oracle's, so |vx - composed| <= 2 BOX_TOL sum_j |c_j| (plus
float64 rounding, ~1e-12 here, which the bound's slack of BOX_TOL itself covers many times over).
"""
import functools
import json
import os
import pickle
import subprocess
import sys

from types import SimpleNamespace

import numpy as np
import pytest

from cm3d_amd import tracks as T
from tests import velocity_pass_cases as pc

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SETTINGS = (2, "mean", 2)                           # min_length, score, smooth_window of the engine under test
TRACK_KEYS = ("track_id", "track_pos", "track_len", "track_stat", "vel_smooth")
INT_KEYS = ("track_id", "track_pos", "track_len", "flags")


def _tracks(st=SETTINGS):
    return T.Tracks(*st)


@functools.lru_cache(maxsize=None)
def batch():
    """velocity_pass_cases' two moving scenes with the scores of frame k of a scene scaled by (8 - k) / 8: the order of the scores
    inside a frame, and with it the NMS, is what it was, but a track's mean and greatest score are no longer every member's own."""
    from cm3d_amd import lifting
    frames = pc.scene_frames(pc.config())
    for i, fr in enumerate(frames):
        fr.scores = [float(s) * (8 - i % pc.FRAMES_PER_SCENE) / 8.0 for s in fr.scores]
    lanes, frame_lane = [pc.lane_table()], [0] * len(frames)
    hb = lifting.pack_frames(frames, lanes, frame_lane)
    assert hb.frame_next.tolist() == [1, 2, -1, 4, 5, -1] and hb.frame_time.tolist() == [0.0, 0.5, 1.0, 60.0, 60.5, 61.0]
    return SimpleNamespace(frames=frames, lanes=lanes, frame_lane=frame_lane, hb=hb)


@functools.lru_cache(maxsize=None)
def expected():
    """The oracle's pass over `batch()` and the velocity stage's host statement on it (as velocity_pass_cases.expected, with its
    builder conditions): a dict of the oracle's arrays plus next_match / prev_match."""
    from oracle import oracle as orc
    from tests.helpers import oracle_batch
    b = batch()
    exp = oracle_batch(orc, b.frames, b.lanes, b.frame_lane, b.hb)
    pc.assert_robust(b.hb, exp["box"], exp["flags"])
    vel = pc.host_velocity(b.hb, exp["box"], exp["flags"])
    pc.check_known_velocities(b.hb, exp["flags"], exp["medoid_pos"], vel, 1e-9)
    return dict(exp, next_match=vel["next_match"], prev_match=vel["prev_match"])


@functools.lru_cache(maxsize=None)
def expected_all_four():
    """The same with clustering, lane filter, yaw fit and rotated NMS composed on the CPU (as velocity_pass_cases.expected_all_four)."""
    from oracle import oracle as orc
    from tests import optin_pass_cases as oc, yaw_fit_pass_cases as yc
    b, o = batch(), pc.all_four_options()
    exp = oc.expected(orc, b.frames, b.lanes, b.frame_lane, b.hb, cluster=o["cluster"], filters=o["filters"], base=expected())
    fit = yc.fitted(orc, b, exp, o["yaw"])
    flags = (fit["flags"] & 1) | (oc.rotated_keep(fit["box"], fit["flags"], b.hb, o["nms"]) << 1)
    pc.assert_robust(b.hb, fit["box"], flags)
    vel = pc.host_velocity(b.hb, fit["box"], flags)
    box = fit["box"].copy()
    box[:, 9] = flags                                # cm3d_box_rotated_nms writes the flags it decides into column 9 as well
    return dict(box=box, flags=flags, next_match=vel["next_match"], prev_match=vel["prev_match"])


def _run(eng, hb):
    import torch
    eng.upload(hb)
    eng.run(masks="rle")
    torch.cuda.synchronize()
    return eng.download()


def host_tracks(hb, src, st=SETTINGS):
    """tracks.box_tracks_host on the arrays of `src` (box, flags, next_match, prev_match: an engine's download or a CPU composition)."""
    return T.box_tracks_host(src["box"], src["flags"], hb.mask_frame, src["next_match"], src["prev_match"], hb.frame_time, *st)


def smooth_bound(hb, tr, W):
    """Per mask: 2 BOX_TOL sum_j |c_j| over its window, c_j = (n t_j - St) / den from the frame times (0 where vel_smooth is zeros by
    the rule).  Asserts den > 0 with margin for every window of two or more."""
    M = len(tr["track_id"])
    t = np.asarray(hb.frame_time, np.float64)[hb.mask_frame]
    bound = np.zeros(M)
    for h in np.unique(tr["track_id"][tr["track_id"] >= 0]):
        mem = np.flatnonzero(tr["track_id"] == h)
        mem = mem[np.argsort(tr["track_pos"][mem])]
        L = len(mem)
        assert tr["track_pos"][mem].tolist() == list(range(L)) and (np.diff(t[mem]) >= pc.DT - 1e-9).all()
        for p, i in enumerate(mem):
            win = mem[max(0, p - W):min(L - 1, p + W) + 1]
            n = len(win)
            if n < 2:
                continue
            tj = t[win] - t[i]
            den = n * (tj * tj).sum() - tj.sum() ** 2
            assert den >= 0.99 * pc.DT * pc.DT                    # (two members DT apart: den = DT^2; more members, more) far from 0
            bound[i] = 2 * pc.BOX_TOL * np.abs((n * tj - tj.sum()) / den).sum()
    return bound


def composed(hb, base, st=SETTINGS):
    """The CPU composition on `base` (box, flags and the matches of the velocity stage's host statement on them); status 0."""
    tr = host_tracks(hb, base, st)
    assert tr["status"] == 0
    return tr


def full_stable_tracks(hb, medoid_pos, tr):
    """Masks of full-length tracks (one box in every frame of the scene) all of whose members are stable masks; asserts every scene
    has one."""
    stable = pc.stable_masks(hb, medoid_pos)
    ok = np.zeros(len(stable), bool)
    for h in np.unique(tr["track_id"][tr["track_id"] >= 0]):
        mem = tr["track_id"] == h
        if mem.sum() == pc.FRAMES_PER_SCENE and stable[mem].all():
            ok |= mem
    scene = np.repeat(np.arange(2), pc.FRAMES_PER_SCENE)[hb.mask_frame]
    assert ok[scene == 0].any() and ok[scene == 1].any(), "a scene without a full-length track of stable masks"
    return ok, scene


@pytest.fixture(scope="module")
def cpu():
    """(oracle arrays + host matches, composed tracks) of the plain pass; the builder's asserts: in each scene at least one
    full-length track of stable masks, whose smoothed velocity is the scene's to 1e-9."""
    base = expected()
    hb = batch().hb
    tr = composed(hb, base)
    ok, scene = full_stable_tracks(hb, base["medoid_pos"], tr)
    assert np.abs(tr["vel_smooth"][ok] - pc.VELOCITY[scene[ok]]).max() <= 1e-9
    return base, tr


@pytest.fixture(scope="module")
def velocity_only():
    from cm3d_amd import lifting
    return _run(lifting.LiftEngine("cuda:0", velocity=pc.settings()[0]), batch().hb)


@pytest.fixture(scope="module")
def tracked():
    from cm3d_amd import lifting
    return _run(lifting.LiftEngine("cuda:0", velocity=pc.settings()[0], tracks=_tracks()), batch().hb)


def _assert_statement(hb, got, before, st=SETTINGS):
    """(a): the device against the host statement on the stage's own inputs."""
    host = host_tracks(hb, before, st)
    for k in INT_KEYS:
        assert np.array_equal(got[k], host[k]), k
    for k in ("track_stat", "box") + (("vel_smooth",) if st[2] else ()):
        assert got[k].tobytes() == host[k].tobytes(), k
    assert host["status"] == 0
    for k in ("vel", "vel_src", "next_match", "prev_match"):          # the velocity stage's outputs are never written
        assert got[k].tobytes() == before[k].tobytes(), k
    return host


def _assert_composed(hb, got, tr, W=SETTINGS[2]):
    """(b): integers and rewritten scores exact, vel_smooth within the derived bound."""
    for k in INT_KEYS:
        assert np.array_equal(got[k], tr[k]), k
    assert np.array_equal(got["box"][:, 7], tr["box"][:, 7]) and np.array_equal(got["box"][:, 9], tr["box"][:, 9])
    bound = smooth_bound(hb, tr, W)
    err = np.abs(got["vel_smooth"] - tr["vel_smooth"]).max(1)
    print(f"max |vel_smooth - composed| = {err.max():.3e} (bound {bound[bound > 0].min():.3e} .. {bound.max():.3e})")
    assert (err <= bound).all() and (bound > 0).sum() >= 12
    return bound


def test_engine_equals_host_statement_and_cpu_composition(velocity_only, tracked, cpu):
    hb = batch().hb
    base, tr = cpu
    assert (tr["track_len"] == pc.FRAMES_PER_SCENE).sum() >= 12 and (tr["box"][:, 7] != base["box"][:, 7]).any()
    _assert_statement(hb, tracked, velocity_only)
    bound = _assert_composed(hb, tracked, tr)
    # the known answer: the stable masks of full-length tracks move at their scene's velocity
    ok, scene = full_stable_tracks(hb, tracked["medoid_pos"], tracked)
    err = np.abs(tracked["vel_smooth"][ok] - pc.VELOCITY[scene[ok]]).max(1)
    print(f"max |vel_smooth - known| = {err.max():.3e} on {ok.sum()} masks")
    assert (err <= bound[ok]).all() and ok.sum() >= 6


def test_a_filter_that_no_track_passes_drops_every_box(velocity_only):
    """min_length above every track's length: each kept box loses bit 1 and only that; max scores; W = 1."""
    from cm3d_amd import lifting
    hb, st = batch().hb, (pc.FRAMES_PER_SCENE + 1, "max", 1)
    got = _run(lifting.LiftEngine("cuda:0", velocity=pc.settings()[0], tracks=_tracks(st)), hb)
    _assert_statement(hb, got, velocity_only, st)
    kept = (velocity_only["flags"] & 3) == 3
    assert kept.sum() >= 12 and np.array_equal(got["flags"], np.where(kept, velocity_only["flags"] & ~2, velocity_only["flags"]))
    assert np.array_equal(got["box"][kept, 9], got["flags"][kept].astype(np.float64))


def test_without_the_option_and_at_its_defaults_nothing_changes(velocity_only, tracked):
    """tracks=None and Tracks() leave every buffer of the velocity engine byte-identical and allocate nothing; with the stage on, what
    it does not own is what it was."""
    from cm3d_amd import lifting
    for tr in (None, T.Tracks(), T.Tracks(1, "own", 0)):
        eng = lifting.LiftEngine("cuda:0", velocity=pc.settings()[0], tracks=tr)
        got = _run(eng, batch().hb)
        assert eng.tracks is None and not any(hasattr(eng.b, k) for k in TRACK_KEYS + ("track_ws", "track_status"))
        assert set(got) == set(velocity_only)
        for k, v in velocity_only.items():
            assert v.tobytes() == got[k].tobytes(), k
    assert set(tracked) == set(velocity_only) | set(TRACK_KEYS)
    for k, v in velocity_only.items():
        if k not in ("box", "flags"):
            assert v.tobytes() == tracked[k].tobytes(), k
    cols = [c for c in range(velocity_only["box"].shape[1]) if c not in (7, 9)]
    assert tracked["box"][:, cols].tobytes() == velocity_only["box"][:, cols].tobytes()


def test_option_needs_the_velocity_stage():
    from cm3d_amd import lifting
    with pytest.raises(ValueError, match="velocity"):
        lifting.LiftEngine("cuda:0", tracks=_tracks())
    lifting.LiftEngine("cuda:0", tracks=T.Tracks())              # at the defaults there is no stage to need it


def test_check_status_raises_on_each_bit(tracked):
    from cm3d_amd import lifting
    from cm3d_amd._lib import Cm3dError
    eng = lifting.LiftEngine("cuda:0", velocity=pc.settings()[0], tracks=_tracks())
    _run(eng, batch().hb)
    for bit in (1, 2, 4):
        eng.b.track_status.fill_(bit)
        with pytest.raises(Cm3dError, match="tracks"):
            eng.check_status()
    eng.b.track_status.zero_()
    eng.check_status()


def test_captured_graph_gives_the_same_bytes(tracked):
    import torch
    from cm3d_amd import lifting
    eng = lifting.LiftEngine("cuda:0", velocity=pc.settings()[0], tracks=_tracks())
    first = _run(eng, batch().hb)
    for k in TRACK_KEYS:                                         # poison: the replay has to write them again
        getattr(eng.b, k).fill_(-3)
    g = eng.capture_graph(masks="rle")
    g.replay()
    torch.cuda.synchronize()
    replayed = eng.download()
    for k in TRACK_KEYS + ("box", "flags", "vel", "next_match"):
        assert first[k].tobytes() == tracked[k].tobytes() == replayed[k].tobytes(), k


def test_pipeline_rerun_and_kept_velocities(tracked):
    """LiftPipeline with the option: `rerun` takes its Python branch (the pass writes box and flags anew, both stages run again), and
    kept_box_velocities are the vel_smooth rows of kept_box_records' masks in its order."""
    import torch
    from cm3d_amd import lifting
    hb = batch().hb
    pipe = lifting.LiftPipeline("cuda:0", depth=1, velocity=pc.settings()[0], tracks=_tracks())
    slot = pipe.submit(hb, "rle")
    pipe.check_status(slot)
    before = pipe.native_passes
    pipe.engines[slot].b.vel_smooth.fill_(float("nan"))
    pipe.engines[slot].b.track_len.fill_(-9)
    pipe.rerun(slot)
    ids = np.stack([np.arange(hb.n_frames), np.zeros(hb.n_frames)], 1)
    rec = pipe.collect_records(slot, ids).cpu().numpy()
    vel = lifting.kept_box_velocities(pipe.engines[slot].b).cpu().numpy()
    again = pipe.collect(slot, full=False)[1]
    torch.cuda.synchronize()
    keep = (tracked["flags"] & 3) == 3
    assert pipe.native_passes == before + 1 and rec.shape[0] == keep.sum()
    assert vel.tobytes() == tracked["vel_smooth"][keep].tobytes() and np.array_equal(rec[:, 7], tracked["box"][keep][:, 7])
    for k in TRACK_KEYS + ("box", "flags"):
        assert again[k].tobytes() == tracked[k].tobytes(), k


def test_behind_all_five_other_options():
    """Clustering, lane filter, yaw fit, rotated NMS and the velocity stage on: the buffers of the pass are those of the same engine
    without the stage, the stage equals the host statement on what that engine left, and the CPU composition of all six holds."""
    from cm3d_amd import lifting
    b, kw = batch(), pc.all_four_options()
    base = _run(lifting.LiftEngine("cuda:0", velocity=pc.settings()[0], **kw), b.hb)
    got = _run(lifting.LiftEngine("cuda:0", velocity=pc.settings()[0], tracks=_tracks(), **kw), b.hb)
    for k, v in base.items():
        if k not in ("box", "flags"):
            assert v.tobytes() == got[k].tobytes(), k
    assert {"cl_off", "medoid_pos_kept", "yaw_src", "vel"} <= set(got)
    _assert_statement(b.hb, got, base)
    tr = composed(b.hb, expected_all_four())
    _assert_composed(b.hb, got, tr)
    assert (tr["track_len"] >= 2).sum() >= 12


# ------------------------------------------------------------------------------------------------ the entry point
ONE_OFF = (0, 2)                 # (scene, mask) of the dataset's mask that is left in frame 0 of its scene only


def write_one_off_dataset(root):
    """velocity_pass_cases.write_dataset, then mask ONE_OFF[1] of scene ONE_OFF[0] taken out of every frame but the first: its box
    shows once, every other box of the job keeps its partners.  Returns (dataroot, mask_dir, names)."""
    dataroot, mask_dir, names = pc.write_dataset(root, n_scenes=2)
    s, j = ONE_OFF
    for f in range(1, pc.FRAMES_PER_SCENE):
        p_masks, p_data = (os.path.join(mask_dir, names[s], f"{f}_{n}") for n in ("masks.pkl", "data.json"))
        with open(p_masks, "rb") as fh:
            rles = pickle.load(fh)
        with open(p_data) as fh:
            data = json.load(fh)
        del rles[j]
        for key in ("labels", "detection_scores", "cam_nums"):
            del data[key][j]
        with open(p_masks, "wb") as fh:
            pickle.dump(rles, fh)
        with open(p_data, "w") as fh:
            json.dump(data, fh)
    return dataroot, mask_dir, names


def one_off_batch(dataroot, mask_dir, names):
    """The batch packed from the dataset's files, and the index of the one-off mask in it."""
    from cm3d_amd import lifting, nusc_io
    tables = nusc_io.NuscTables("v1.0-synth", dataroot, annotations=False)
    frames = [f for n in names for f in nusc_io.frames_of_scene(tables, tables.scene_by_name(n), mask_dir, n_sweeps=3, ratio=pc.config().ratio)]
    hb = lifting.pack_frames(frames, [pc.lane_table()], [0] * len(frames))
    return frames, hb, int(hb.mask_off[ONE_OFF[0] * pc.FRAMES_PER_SCENE]) + ONE_OFF[1]


def _entry_point(dataroot, mask_dir, out_dir, *flags, ok=True):
    env = dict(os.environ, CM3D_VER_NAME="v1.0-synth", CM3D_INPUT_PATH=dataroot, CM3D_INPUT_DIR=mask_dir, CM3D_OUTPUT_DIR=str(out_dir))
    r = subprocess.run([sys.executable, "2d_to_3d.py", "--ratio", str(pc.config().ratio), *flags], cwd=os.path.join(ROOT, "src", "nuscenes"),
                       env=env, capture_output=True, text=True, timeout=300)
    if not ok:
        return r
    assert r.returncode == 0, r.stderr[-2000:]
    return open(os.path.join(out_dir, "pseudolabels_minival.json"), "rb").read()


@pytest.fixture(scope="module")
def outputs(tmp_path_factory):
    """The entry point's files for the flag sets of the tests below, one run each, on one dataset."""
    from cm3d_amd import lifting
    root = tmp_path_factory.mktemp("one_off")
    dataroot, mask_dir, names = write_one_off_dataset(root)
    vel = ("--velocity", "track", "--velocity-max-speed", ",".join(f"{n}={pc.MAX_SPEED}" for n in sorted(lifting.ClassTable.nuscenes().names)))
    runs = {"velocity": vel, "min2": vel + ("--track-min-length", "2"), "min2_python": vel + ("--track-min-length", "2", "--reader-threads", "-1"),
            "defaults": vel + ("--track-min-length", "1", "--track-score", "own", "--velocity-smooth", "0")}
    out = {k: _entry_point(dataroot, mask_dir, root / k, *flags) for k, flags in runs.items()}
    out["dataset"] = (dataroot, mask_dir, names)
    return out


def test_entry_point_min_length_drops_exactly_the_one_off_box(outputs):
    """--track-min-length 2: the file lacks the one box whose mask shows in a single frame, is otherwise the bytes of the run
    without the flag, and is the same through the native and the Python reader."""
    from cm3d_amd import lifting
    a, b = outputs["velocity"], outputs["min2"]
    assert b == outputs["min2_python"]
    frames, hb, one = one_off_batch(*outputs["dataset"])
    before = _run(lifting.LiftEngine("cuda:0", velocity=pc.settings()[0]), hb)
    got = _run(lifting.LiftEngine("cuda:0", velocity=pc.settings()[0], tracks=T.Tracks(min_length=2)), hb)
    _assert_statement(hb, got, before, (2, "own", 0))
    kept = (before["flags"] & 3) == 3
    # the builder's condition: the one-off box is kept and alone, every other kept box has a partner
    assert kept[one] and got["track_len"][one] == 1 and (got["track_len"][kept & (np.arange(len(kept)) != one)] >= 2).all()
    assert np.flatnonzero(got["flags"] != before["flags"]).tolist() == [one]
    ra, rb = json.loads(a)["results"], json.loads(b)["results"]
    assert list(ra) == list(rb) == hb.tokens
    token = hb.tokens[hb.mask_frame[one]]
    gone = [x for x in ra[token] if x not in rb[token]]
    assert len(gone) == 1 and gone[0]["translation"][:2] == before["box"][one, :2].tolist()
    assert sum(len(v) for v in ra.values()) == kept.sum() == sum(len(v) for v in rb.values()) + 1
    assert all(rb[t] == [x for x in ra[t] if x is not gone[0]] for t in ra)
    # bytes: the file without the flag minus one contiguous span is the file with it
    k = next((i for i, (x, y) in enumerate(zip(a, b)) if x != y), len(b))
    assert len(a) > len(b) and a[:k] + a[k + len(a) - len(b):] == b


def test_entry_point_flags_at_their_defaults_write_the_bytes_of_velocity_track(outputs):
    assert outputs["defaults"] == outputs["velocity"]


def test_entry_point_flag_without_velocity_track_is_an_error(outputs):
    dataroot, mask_dir, _ = outputs["dataset"]
    r = _entry_point(dataroot, mask_dir, os.path.join(dataroot, "unused"), "--track-min-length", "2", ok=False)
    assert r.returncode == 2 and "--velocity track" in r.stderr
