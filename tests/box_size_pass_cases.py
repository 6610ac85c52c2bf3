"""The batch and the CPU composition of tests/test_gpu_box_size_pass.py.  No GPU here: the oracle's pass, yaw_fit_pass_cases.fitted,
boxplace.box_place_host, velocity.track_velocity_host, tracks.box_tracks_host, boxsize.box_size_host, one after the other.

The batch: velocity_pass_cases' two moving scenes (three keyframes 0.5 s apart each; scene 0 moves at (2, -1) m/s, scene 1 stands) at
the image size of yaw_fit_pass_cases, with that module's car of two faces added to every frame as the last mask.  The car is built
relative to the frame's camera, so it moves with its scene and is one track of three boxes whose rectangle has the extents of
CAR_L x CAR_W, not of the class prior."""
import copy
import functools
import os
from types import SimpleNamespace

import numpy as np

from cm3d_amd import bevfit, boxplace, boxsize
from cm3d_amd import synthetic as syn
from cm3d_amd import tracks as T
from tests import velocity_pass_cases as pc
from tests import yaw_fit_pass_cases as yc

Y = bevfit.YawFit()
P = boxplace.BoxPlace()
S = boxsize.BoxSize()
SIZE_KEYS = ("size_wlh", "size_src", "size_ratio", "size_obs", "size_placed", "size_vel")


def config():
    return syn.config("tiny", n_points=9000, n_masks=8, duplicate_prob=0.25, width=512, height=288, ratio=0.32, max_area=12000.0)


def _own_lists(fr):
    """moved_frame shares the base frame's lists between the frames of a scene; add_l_vehicle edits them in place."""
    fr = copy.copy(fr)                             # (keeps timestamp and next_token, which moved_frame sets beside the fields)
    fr.sweeps_raw, fr.rles, fr.labels = [np.array(r) for r in fr.sweeps_raw], list(fr.rles), list(fr.labels)
    fr.scores, fr.cam_nums = list(fr.scores), list(fr.cam_nums)
    return fr


def scene_frames():
    frames = [_own_lists(f) for f in pc.scene_frames(config())]
    for f in frames:
        yc.add_l_vehicle(f, pc.LANE_YAW)
    return frames


@functools.lru_cache(maxsize=None)
def batch():
    from cm3d_amd import lifting
    frames = scene_frames()
    lanes, frame_lane = [pc.lane_table()], [0] * len(frames)
    classes = lifting.ClassTable.nuscenes()
    hb = lifting.pack_frames(frames, lanes, frame_lane, classes)
    assert hb.frame_next.tolist() == [1, 2, -1, 4, 5, -1] and hb.frame_time.tolist() == [0.0, 0.5, 1.0, 60.0, 60.5, 61.0]
    return SimpleNamespace(name="size", frames=frames, lanes=lanes, frame_lane=frame_lane, hb=hb, classes=classes,
                           l_masks=[int(m) - 1 for m in hb.mask_off[1:]])


def host_size(hb, classes, src, tr, place, v, smooth_window=0, s=S):
    """boxsize.box_size_host on the arrays of `src` (box, flags, fit_rect, place_src, next_match, prev_match) and `tr` (the track arrays)."""
    return boxsize.box_size_host(src["box"], src["flags"], hb.mask_frame, src["fit_rect"], src["place_src"], classes.prior_wlh, hb.ego_xyz,
                                 src["next_match"], src["prev_match"], tr["track_id"], tr["track_pos"], tr["track_len"], hb.frame_time,
                                 thin=place.thin, max_dt=v.max_dt, smooth_window=smooth_window, q=s.q, min_obs=s.min_obs, lo=s.lo, hi=s.hi)


def composed(orc, front=None, nms=None, tracks=(1, "own", 0), s=S, y=Y, p=P, b=None):
    """The whole chain on the CPU, nothing from the device: `front` (the expectation of the pass in front of the fit; the oracle's plain
    pass when None), the yaw fit, the placement with its circle NMS, the rotated NMS when given, the velocity stage, the track stage with
    `tracks` = (min_length, score, smooth_window), the size stage.  b: a batch built like batch() (frames, lanes, frame_lane, hb,
    classes); batch() itself when None.  Returns (the arrays in front of the size stage, its outputs)."""
    from tests import optin_pass_cases as oc
    from tests.helpers import oracle_batch
    if b is None:
        b = batch()
    hb = b.hb
    if front is None:
        front = oracle_batch(orc, b.frames, b.lanes, b.frame_lane, hb)
    fit = yc.fitted(orc, b, front, y)
    planes = (int(np.diff(hb.mask_off).max()) + 31) // 32
    pl = boxplace.box_place_host(fit["box"], fit["flags"], hb.mask_off, fit["fit_rect"], fit["yaw_src"], b.classes.prior_wlh, b.classes.nms_group,
                                 b.classes.nms_thr, hb.ego_xyz, p.thin, min(32 * planes, 1024))
    box, flags = pl["box"], pl["flags"]
    if nms is not None:
        flags = (flags & 1) | (oc.rotated_keep(box, flags, hb, nms) << 1)
        box = box.copy()
        box[:, 9] = flags
    pc.assert_robust(hb, box, flags)
    vel = pc.host_velocity(hb, box, flags)
    tr = T.box_tracks_host(box, flags, hb.mask_frame, vel["next_match"], vel["prev_match"], hb.frame_time, *tracks)
    assert vel["status"] == 0 and tr["status"] == 0
    before = dict(fit, box=tr["box"], flags=tr["flags"], place_src=pl["place_src"], next_match=vel["next_match"], prev_match=vel["prev_match"],
                  vel=vel["vel"], **{k: tr[k] for k in ("track_id", "track_pos", "track_len", "vel_smooth")})
    out = host_size(hb, b.classes, before, tr, p, pc.settings()[0], tracks[2], s)
    assert out["status"] == 0
    return before, out


def write_dataset(root):
    """The batch's two scenes in the reference's on-disk formats (velocity_pass_cases.write_dataset with this module's image size and
    the car added to every frame before it is written).  Returns (dataroot, mask_dir, scene names)."""
    real_moved, real_config = pc.moved_frame, pc.config

    def moved_with_car(base, s, k, *a, **kw):
        fr = _own_lists(real_moved(base, s, k, *a, **kw))
        yc.add_l_vehicle(fr, pc.LANE_YAW)
        return fr
    pc.moved_frame, pc.config = moved_with_car, config
    try:
        return pc.write_dataset(root, n_scenes=2)
    finally:
        pc.moved_frame, pc.config = real_moved, real_config


def dataset_batch(dataroot, mask_dir, names):
    """The batch packed from the dataset's files, as the entry point's Python reader packs it."""
    from cm3d_amd import lifting, nusc_io
    tables = nusc_io.NuscTables("v1.0-synth", dataroot, annotations=False)
    frames = [f for n in names for f in nusc_io.frames_of_scene(tables, tables.scene_by_name(n), mask_dir, n_sweeps=3, ratio=config().ratio)]
    return lifting.pack_frames(frames, [pc.lane_table()], [0] * len(frames))
