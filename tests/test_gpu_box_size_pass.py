"""GPU: the size stage behind the track stage (LiftEngine(yaw, place, velocity, tracks, size), cm3d_box_size behind cm3d_box_tracks) on
the batch of tests/box_size_pass_cases.py -- velocity_pass_cases' two moving scenes with yaw_fit_pass_cases' car of two faces in every
frame --, and the nuScenes entry point with --size track on the same scenes written to disk.

(i)  the stage's outputs equal boxsize.box_size_host applied to the arrays the same engine WITHOUT `size` leaves on the device (box,
     flags, fit_rect, place_src, the matches and the track arrays: the stage's inputs), to the bit;
(ii) against the composition on the CPU that takes nothing from the device (box_size_pass_cases.composed), size_src, size_obs and flags
     are exact; sizes, ratios and the centres of the sized boxes are functions of fit_rect and the sensor, which are exact
     (test_gpu_box_place_pass holds placed centres to the bit for the same reason): to the bit; every other centre lies within
     velocity_pass_cases.BOX_TOL (test_gpu_parity's tolerance), and size_vel within the bound test_gpu_tracks_pass derives for
     vel_smooth from that tolerance -- 2 BOX_TOL sum_j |c_j| over the window, which for the two-neighbour form is 2 BOX_TOL / span.
No tolerance is new here."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

from cm3d_amd import boxsize as bs
from cm3d_amd import nms as nmsmod
from cm3d_amd import tracks as T
from tests import box_size_cases as sc
from tests import box_size_pass_cases as sp
from tests import velocity_pass_cases as pc
from tests.test_gpu_tracks_pass import smooth_bound

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TR = (2, "mean", 2)


def _engine(size=sp.S, tracks=None, **kw):
    from cm3d_amd import lifting
    kw.setdefault("yaw", sp.Y)
    return lifting.LiftEngine("cuda:0", classes=sp.batch().classes, place=sp.P, velocity=pc.settings()[0], tracks=tracks, size=size, **kw)


def _run(eng, hb=None):
    import torch
    if hb is not None:
        eng.upload(hb)
    eng.run(masks="rle")
    torch.cuda.synchronize()
    return eng.download()


def _track_arrays(hb, base, st):
    """The track arrays in front of the size stage: the base engine's own where it ran the track stage, else the host statement's on
    the base engine's matches (integers: the device's to the bit, tests/test_gpu_tracks.py)."""
    if "track_id" in base:
        return base
    return T.box_tracks_host(base["box"], base["flags"], hb.mask_frame, base["next_match"], base["prev_match"], hb.frame_time, *st)


def _assert_statement(got, base, st=(1, "own", 0), s=sp.S):
    """(i): the device against the host statement on the stage's own inputs; what the stage never writes is the base engine's."""
    b = sp.batch()
    tr = _track_arrays(b.hb, base, st)
    host = sp.host_size(b.hb, b.classes, dict(base, box=tr["box"], flags=tr["flags"]), tr, sp.P, pc.settings()[0], st[2], s)
    assert host["status"] == 0
    sc.assert_same(dict(got, status=0), host, "statement")
    assert got["box"][:, 2:].tobytes() == tr["box"][:, 2:].tobytes()
    for k, v in base.items():
        if k not in ("box", "flags"):
            assert got[k].tobytes() == v.tobytes(), k
    return host


def _assert_composed(got, before, out, W=0):
    """(ii): against the composition on the CPU."""
    hb = sp.batch().hb
    for k in ("size_src", "size_obs", "flags"):
        assert np.array_equal(got[k], out[k]), k
    for k in ("track_id", "track_pos", "track_len", "place_src"):
        assert np.array_equal(got[k], before[k]), k
    assert got["size_wlh"].tobytes() == out["size_wlh"].tobytes() and got["size_ratio"].tobytes() == out["size_ratio"].tobytes()
    on = out["size_src"] > 0
    placed = before["place_src"] > 0
    assert on.sum() >= 6 and got["box"][placed, :2].tobytes() == out["box"][placed, :2].tobytes()
    assert np.abs(got["box"][:, :2] - out["box"][:, :2]).max() <= pc.BOX_TOL
    assert np.abs(got["size_placed"] - before["box"][:, :2]).max() <= pc.BOX_TOL
    if W:
        bound = smooth_bound(hb, before, W)
    else:                                            # the two-neighbour form: two centres over a span of DT or 2 DT
        bound = np.where((before["next_match"] >= 0) | (before["prev_match"] >= 0), 2 * pc.BOX_TOL / pc.DT, 0.0)
    err = np.abs(got["size_vel"] - out["size_vel"]).max(1)
    print(f"{int(on.sum())} boxes sized ({np.bincount(out['size_src'], minlength=4).tolist()} by size_src); max |size_vel - composed| = "
          f"{err.max():.3e} (bound {bound.max():.3e})")
    assert (err <= bound).all()


@pytest.fixture(scope="module")
def base():
    return _run(_engine(size=None), sp.batch().hb)


@pytest.fixture(scope="module")
def sized():
    return _run(_engine(), sp.batch().hb)


def test_engine_equals_host_statement_and_cpu_composition(oracle, base, sized):
    b = sp.batch()
    assert set(sized) == set(base) | set(sp.SIZE_KEYS) | {"track_id", "track_pos", "track_len", "track_stat"}
    _assert_statement(sized, base)
    before, out = sp.composed(oracle)
    _assert_composed(sized, before, out)
    # the cars of two faces: three boxes a track, both dimensions pooled from three observations, sized by their own extents
    for m in b.l_masks:
        assert sized["size_src"][m] == 3 and sized["size_obs"][m].tolist() == [3, 3] and sized["track_len"][m] == 3
        assert np.abs(sized["size_wlh"][m, :2] - [sp.yc.CAR_W, sp.yc.CAR_L]).max() < 0.05
        assert np.array_equal(sized["size_wlh"][m, 2], b.classes.prior_wlh[b.hb.class_id[m], 2])
    moved = np.hypot(*(sized["box"][:, :2] - base["box"][:, :2]).T)
    assert moved[sized["size_src"] > 0].max() > 0.01 and not moved[sized["size_src"] == 0].any()
    print(f"centres moved by up to {moved.max():.3f} m")
    # the scene's velocity: the car is the same points in every frame, its sized centres move by exactly k D
    scene = np.repeat(np.arange(2), pc.FRAMES_PER_SCENE)[b.hb.mask_frame]
    assert np.abs(sized["size_vel"][b.l_masks] - pc.VELOCITY[scene[b.l_masks]]).max() <= 2 * pc.BOX_TOL / pc.DT


def test_with_a_track_stage_that_filters_scores_and_smooths(oracle):
    base = _run(_engine(size=None, tracks=T.Tracks(*TR)), sp.batch().hb)
    got = _run(_engine(tracks=T.Tracks(*TR)), sp.batch().hb)
    _assert_statement(got, base, TR)
    before, out = sp.composed(oracle, tracks=TR)
    _assert_composed(got, before, out, W=TR[2])
    assert got["vel_smooth"].tobytes() == base["vel_smooth"].tobytes()           # (the track stage's own output is never written)


def test_behind_the_clustered_the_filtered_pass_and_the_rotated_nms(oracle):
    from tests import optin_pass_cases as oc
    from tests.helpers import oracle_batch
    b, o = sp.batch(), pc.all_four_options()
    plain = oracle_batch(oracle, b.frames, b.lanes, b.frame_lane, b.hb)
    for kw in (dict(cluster=o["cluster"]), dict(filters=o["filters"]), dict(nms=o["nms"]),
               dict(cluster=o["cluster"], filters=o["filters"], nms=o["nms"])):
        base = _run(_engine(size=None, **kw), b.hb)
        got = _run(_engine(**kw), b.hb)
        _assert_statement(got, base)
        front = oc.expected(oracle, b.frames, b.lanes, b.frame_lane, b.hb, cluster=kw.get("cluster"), filters=kw.get("filters"), base=plain)
        before, out = sp.composed(oracle, front=front, nms=kw.get("nms"))
        _assert_composed(got, before, out)


def test_identity_against_the_device_velocity_and_tracks(base):
    """lo = hi = 1: nothing is observed; box is the bytes of the engine without the stage, size_vel the velocity stage's `vel`, and
    with a smoothing window the track stage's `vel_smooth`."""
    one = bs.BoxSize(lo=1.0, hi=1.0)
    got = _run(_engine(size=one), sp.batch().hb)
    assert got["box"].tobytes() == base["box"].tobytes() and not got["size_src"].any() and not got["size_obs"].any()
    assert got["size_vel"].tobytes() == base["vel"].tobytes() and np.abs(base["vel"]).max() > 1.0
    for W in (1, 3):
        t = T.Tracks(1, "own", W)
        smoothed = _run(_engine(size=None, tracks=t), sp.batch().hb)
        got = _run(_engine(size=one, tracks=t), sp.batch().hb)
        assert got["box"].tobytes() == smoothed["box"].tobytes() and got["size_vel"].tobytes() == smoothed["vel_smooth"].tobytes()


def test_captured_graph_and_second_pass_give_the_same_bytes(sized):
    import torch
    eng = _engine()
    first = _run(eng, sp.batch().hb)

    def poison():
        for k in sp.SIZE_KEYS:
            getattr(eng.b, k).fill_(-3)
        eng.b.box.fill_(-3.0)
    poison()
    again = _run(eng)
    g = eng.capture_graph(masks="rle")
    poison()
    g.replay()
    torch.cuda.synchronize()
    replayed = eng.download()
    for k in sized:
        assert first[k].tobytes() == sized[k].tobytes() == again[k].tobytes() == replayed[k].tobytes(), k
    assert all(np.array_equal(eng.download(full=False)[k], sized[k]) for k in sp.SIZE_KEYS)


def test_pipeline_rerun_with_batches_in_flight_and_the_kept_rows(sized):
    """LiftPipeline with the option, two slots busy: `rerun` takes its Python branch; kept_box_sizes and kept_box_velocities are the
    size_wlh and size_vel rows of kept_box_records' masks in its order."""
    import torch
    from cm3d_amd import lifting
    hb = sp.batch().hb
    pipe = lifting.LiftPipeline("cuda:0", depth=2, classes=sp.batch().classes, yaw=sp.Y, place=sp.P, velocity=pc.settings()[0], size=sp.S)
    slots = [pipe.submit(hb, "rle"), pipe.submit(hb, "rle")]
    assert not pipe.engines[0].b.plain_pass
    before = pipe.native_passes
    for s in slots:
        pipe.rerun(s)
    pipe.rerun(slots[0])
    assert pipe.native_passes == before + 3
    ids = np.stack([np.arange(hb.n_frames), np.zeros(hb.n_frames)], 1)
    keep = (sized["flags"] & 3) == 3
    for s in slots:
        rec = pipe.collect_records(s, ids).cpu().numpy()
        b = pipe.engines[s].b
        sizes, vel = lifting.kept_box_sizes(b).cpu().numpy(), lifting.kept_box_velocities(b).cpu().numpy()
        again = pipe.collect(s, full=False)[1]
        torch.cuda.synchronize()
        assert rec.shape[0] == keep.sum() and rec[:, :2].tobytes() == sized["box"][keep, :2].tobytes()
        assert sizes.tobytes() == sized["size_wlh"][keep].tobytes() and vel.tobytes() == sized["size_vel"][keep].tobytes()
        for k in sp.SIZE_KEYS + ("box", "flags"):
            assert again[k].tobytes() == sized[k].tobytes(), k


def test_without_the_option_nothing_changes_and_the_option_needs_its_stages(base):
    from cm3d_amd import lifting
    from cm3d_amd._lib import Cm3dError
    b = sp.batch()
    without = lifting.LiftEngine("cuda:0", classes=b.classes, yaw=sp.Y, place=sp.P, velocity=pc.settings()[0])
    got = _run(without, b.hb)
    assert set(got) == set(base) and without.size is None and without.tracks is None
    for k, v in base.items():
        assert v.tobytes() == got[k].tobytes(), k
    assert not any(hasattr(without.b, k) for k in sp.SIZE_KEYS + ("size_ws", "size_status", "track_id"))
    for kw in (dict(place=sp.P, velocity=pc.settings()[0]), dict(yaw=sp.Y, velocity=pc.settings()[0]), dict(yaw=sp.Y, place=sp.P)):
        with pytest.raises(ValueError, match="size=BoxSize"):
            lifting.LiftEngine("cuda:0", classes=b.classes, size=sp.S, **kw)
    eng = _engine()
    _run(eng, b.hb)
    assert eng.tracks == T.Tracks() and hasattr(eng.b, "track_id")
    for bit in (1, 2):
        eng.b.size_status.fill_(bit)
        with pytest.raises(Cm3dError, match="size"):
            eng.check_status()
    eng.b.size_status.zero_()
    eng.check_status()


# ------------------------------------------------------------------------------------------------ the entry point
def _entry_point(dataroot, mask_dir, out_dir, *flags):
    env = dict(os.environ, CM3D_VER_NAME="v1.0-synth", CM3D_INPUT_PATH=dataroot, CM3D_INPUT_DIR=mask_dir, CM3D_OUTPUT_DIR=str(out_dir))
    r = subprocess.run([sys.executable, "2d_to_3d.py", "--ratio", str(sp.config().ratio), *flags], cwd=os.path.join(ROOT, "src", "nuscenes"),
                       env=env, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-2000:]
    return open(os.path.join(out_dir, "pseudolabels_minival.json"), "rb").read()


def test_entry_point_writes_the_sizes_and_velocities_of_the_engine(tmp_path):
    """src/nuscenes/2d_to_3d.py --yaw fit --place fit --velocity track --size track on the scenes written to disk, both host routes:
    the file is the text writer's for the records, velocities and sizes of an engine with the option on the batch packed from the same
    files; --size prior writes the bytes of no flag."""
    from cm3d_amd import lifting
    from cm3d_amd.pipeline_nuscenes import META
    dataroot, mask_dir, names = sp.write_dataset(tmp_path)
    classes = lifting.ClassTable.nuscenes()
    full = ("--yaw", "fit", "--place", "fit", "--velocity", "track", "--velocity-max-speed", ",".join(f"{n}={pc.MAX_SPEED}" for n in sorted(classes.names)))
    runs = {"none": full, "prior": full + ("--size", "prior"), "native": full + ("--size", "track"),
            "python": full + ("--size", "track", "--reader-threads", "-1")}
    out = {k: _entry_point(dataroot, mask_dir, tmp_path / k, *flags) for k, flags in runs.items()}
    assert out["prior"] == out["none"] and out["native"] != out["none"] and out["native"] == out["python"]
    hb = sp.dataset_batch(dataroot, mask_dir, names)
    ids = np.stack([np.arange(hb.n_frames), np.zeros(hb.n_frames)], 1)
    eng = lifting.LiftEngine("cuda:0", classes=classes, yaw=sp.Y, place=sp.P, velocity=pc.settings()[0], size=bs.BoxSize())
    got = _run(eng, hb)
    rec = lifting.kept_box_records(eng.b, ids).cpu().numpy()
    sizes, vel = lifting.kept_box_sizes(eng.b).cpu().numpy(), lifting.kept_box_velocities(eng.b).cpu().numpy()
    assert (got["size_src"] > 0).sum() >= 6 and (sizes != classes.prior_wlh[rec[:, 8].astype(int)]).any()
    text, n = lifting.nuscenes_results_json(rec, hb.tokens, classes, dict(META), vel=vel, size=sizes)
    assert out["native"] == text.encode() and n == len(rec)
    # the cars of two faces (the last mask of every frame) carry their own extents into the file
    res = json.loads(out["native"])["results"]
    for f, m in enumerate(int(x) - 1 for x in hb.mask_off[1:]):
        assert got["flags"][m] & 3 == 3 and got["size_src"][m] == 3
        mine = [bx for bx in res[hb.tokens[f]] if bx["translation"][:2] == got["box"][m, :2].tolist()]
        assert len(mine) == 1 and mine[0]["size"] == got["size_wlh"][m].tolist() and mine[0]["velocity"] == got["size_vel"][m].tolist()
        assert abs(mine[0]["size"][0] - sp.yc.CAR_W) < 0.05 and abs(mine[0]["size"][1] - sp.yc.CAR_L) < 0.05
