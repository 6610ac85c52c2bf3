"""The batch of the velocity stage's pass tests: two scenes of three keyframes whose world moves rigidly at a known velocity, and
the CPU expectation composed from the oracle's pass.  Numpy, the oracle and the host statements of cm3d_amd only.

A scene is ONE synthetic frame (cm3d_amd.synthetic.make_frame) shown three times, 0.5 s apart, with the ego pose -- the sweeps', the
cameras' and the key frame's -- moved by k * D in the global frame; the sensor-frame data stay what they are, so every object of
the scene moves by exactly D per frame.  The poses are rebased to EGO0 first: every global coordinate of the batch then lies in one
float32 binade per axis, D is a multiple of that binade's ulp, and a float32 sum a + (t + k D) is the sum a + t moved by k D.  The
points in every mask and their float32 coordinates in frame k are therefore those of frame 0 moved by k D, to the bit, and so is the
centroid wherever the medoid is the same point of the list (stable_masks: the medoid's sums are not translation invariant).
The lane table has ONE yaw: the push of a vehicle's box along its lane does not depend on which lane point is nearest, and the boxes
move by k D as well (to float64 rounding).  Scene 0 moves at VELOCITY[0], scene 1 stands still.

The builder asserts what the tolerance of the parity tests (BOX_TOL) may not touch: no candidate pair lies within 2 BOX_TOL of its
gate, and no box has more than one candidate within gate + 2 BOX_TOL in the neighbouring frame -- so moving any centre by BOX_TOL
changes neither a weight-positive decision nor the assignment.  If that assert fails the inputs are wrong, not the tolerance.
"""
import dataclasses
import functools
from types import SimpleNamespace

import numpy as np

from cm3d_amd import synthetic as syn
from cm3d_amd import velocity as velmod

BOX_TOL = 1e-4                                  # tests/test_gpu_parity.py
DT = 0.5
EGO0 = np.array([768.0, 1536.0])                # x in [512, 1024): ulp 2^-14; y in [1024, 2048): ulp 2^-13; the cloud reaches ~100 m
VELOCITY = np.array([[2.0, -1.0], [0.0, 0.0]])  # m/s of the two scenes: D = (1, -0.5) m per frame, dyadic
FRAMES_PER_SCENE = 3
LANE_YAW = 0.3
MAX_SPEED = 6.0                                 # gate 3 m: |D| = 1.12 m lies well inside, the objects lie further apart
T0_US = 1533151603547590                        # a nuScenes-sized timestamp


def moved_frame(base, s, k, vel=VELOCITY):
    """Frame k of scene s: `base` with every ego translation rebased to EGO0 and moved by k * DT * vel[s % len(vel)] (x, y only)."""
    delta = (EGO0 - np.asarray(base.sweep_xf[0][21:23], np.float64)).astype(np.float32)      # the rebase: one float32 vector
    v = np.asarray(vel[s % len(vel)], np.float64)          # scenes beyond the table take its rows in turn: even ones move, odd ones stand
    step = (k * DT * v).astype(np.float32)
    assert np.array_equal(step.astype(np.float64), k * DT * v)
    xf, cams = np.array(base.sweep_xf, np.float32), np.array(base.cams, np.float32)
    xf[:, 21:23] = (xf[:, 21:23] + delta) + step
    cams[:, 0:2] = (cams[:, 0:2] - delta) - step
    # exact: rebased + k D in float32 equals the float64 sum
    assert np.array_equal(xf[:, 21:23].astype(np.float64), (np.array(base.sweep_xf, np.float32)[:, 21:23] + delta).astype(np.float64) + step)
    assert np.array_equal(cams[:, 0:2].astype(np.float64), (np.array(base.cams, np.float32)[:, 0:2] - delta).astype(np.float64) - step)
    ego = np.array(base.ego_xyz, np.float64)
    ego[:2] = xf[0, 21:23].astype(np.float64)              # the key frame's pose: what its sweep record holds
    fr = dataclasses.replace(base, token=f"{base.token}-s{s}k{k}", sweep_xf=xf, cams=cams, ego_xyz=ego)
    fr.timestamp = T0_US + s * 60_000_000 + k * int(DT * 1e6)
    return fr


def lane_table(yaw=LANE_YAW):
    """Lane points on a 4 m grid around EGO0, all with the yaw `yaw`."""
    g = np.arange(-140.0, 141.0, 4.0)
    X, Y = np.meshgrid(EGO0[0] + g, EGO0[1] + g)
    return np.stack([X.ravel(), Y.ravel(), np.full(X.size, yaw)], 1)


def scene_frames(cfg, n_scenes=2, frames_per_scene=FRAMES_PER_SCENE, first_scene=0):
    """The frames of scenes first_scene .. first_scene + n_scenes - 1: scene s is synthetic frame 1000 s shown frames_per_scene times,
    moving at VELOCITY[s % 2]."""
    frames = []
    for s in range(first_scene, first_scene + n_scenes):
        base = syn.make_frame(cfg, 1000 * s)
        fs = [moved_frame(base, s, k) for k in range(frames_per_scene)]
        for k, fr in enumerate(fs):
            fr.next_token = fs[k + 1].token if k + 1 < len(fs) else ""
        frames.extend(fs)
    return frames


def config():
    return syn.config("tiny", n_masks=8, duplicate_prob=0.25)


def write_dataset(root, n_scenes=2, frames_per_scene=FRAMES_PER_SCENE, lane_yaws=None, road_half=None):
    """The moving scenes in the reference's on-disk formats: nusc_io.write_synthetic_dataset with moved_frame for its frames (timestamps
    500000 * f, as the writer sets them) and a one-yaw lane table for every map location -- lane_yaws[s], LANE_YAW for all when None.
    road_half: None, or one half side per scene: the location's drivable area becomes that square around EGO0 (the writer's is a 160 m
    square with a hole for every scene).  Returns (dataroot, mask_dir, scene names)."""
    import json
    import os
    from cm3d_amd import nusc_io
    real = syn.make_frame
    syn.make_frame = lambda cfg, index: moved_frame(real(cfg, 1000 * (index // 1000)), index // 1000, index % 1000)
    try:
        dataroot, mask_dir, names = nusc_io.write_synthetic_dataset(str(root), config(), n_scenes=n_scenes, frames_per_scene=frames_per_scene)
    finally:
        syn.make_frame = real
    for s in range(n_scenes):
        np.save(os.path.join(dataroot, "lanes", f"synthtown-{s}.npy"), lane_table(LANE_YAW if lane_yaws is None else lane_yaws[s]))
        if road_half is not None:
            h = float(road_half[s])
            ring = [(EGO0[0] - h, EGO0[1] - h), (EGO0[0] + h, EGO0[1] - h), (EGO0[0] + h, EGO0[1] + h), (EGO0[0] - h, EGO0[1] + h)]
            nodes = [{"token": f"node-{s}-ext-{i}", "x": float(x), "y": float(y)} for i, (x, y) in enumerate(ring)]
            polygon = {"token": f"poly-{s}", "exterior_node_tokens": [n["token"] for n in nodes], "holes": []}
            with open(os.path.join(dataroot, "maps", "expansion", f"synthtown-{s}.json"), "w") as fh:
                json.dump({"node": nodes, "polygon": [polygon], "drivable_area": [{"token": f"da-{s}", "polygon_tokens": [polygon["token"]]}]}, fh)
    return dataroot, mask_dir, names


@functools.lru_cache(maxsize=None)
def batch():
    """frames, lanes, frame_lane, hb (lifting.pack_frames: frame_next and frame_time from the frames' timestamp / next_token)."""
    from cm3d_amd import lifting
    frames = scene_frames(config())
    lanes, frame_lane = [lane_table()], [0] * len(frames)
    hb = lifting.pack_frames(frames, lanes, frame_lane)
    assert hb.frame_next.tolist() == [1, 2, -1, 4, 5, -1] and hb.frame_time.tolist() == [0.0, 0.5, 1.0, 60.0, 60.5, 61.0]
    return SimpleNamespace(frames=frames, lanes=lanes, frame_lane=frame_lane, hb=hb)


def settings(classes=None):
    """The engine's switch and what it hands to the kernel: (Velocity, track_group, max_speed per group)."""
    from cm3d_amd import lifting
    classes = classes or lifting.ClassTable.nuscenes()
    v = velmod.Velocity(max_speed=MAX_SPEED, max_dt=1.5)
    return v, np.asarray(classes.nms_group, np.int32), v.speed_by_group(classes)


def host_velocity(hb, box, flags):
    """velocity.track_velocity_host on box rows and flags of the batch, with the settings above."""
    v, group, speed = settings()
    return velmod.track_velocity_host(box, flags, hb.mask_off, hb.class_id, hb.frame_next, hb.frame_time, group, speed, v.max_dt,
                                      want_weights=True)


def assert_robust(hb, box, flags, tol=BOX_TOL):
    """The builder condition on box rows of the batch: moving any centre by `tol` changes no weight-positive decision and no
    assignment."""
    v, group, speed = settings()
    link, dt, _, _ = velmod.link_table(hb.mask_off, hb.frame_next, hb.frame_time, v.max_dt)
    kept = (np.asarray(flags) & 3) == 3
    grp = group[hb.class_id]
    n_pos = 0
    for f in np.flatnonzero(link):
        n = int(hb.frame_next[f])
        a, b = np.arange(hb.mask_off[f], hb.mask_off[f + 1]), np.arange(hb.mask_off[n], hb.mask_off[n + 1])
        cand = kept[a][:, None] & kept[b][None, :] & (grp[a][:, None] == grp[b][None, :])
        dist = np.hypot(box[b][None, :, 0] - box[a][:, None, 0], box[b][None, :, 1] - box[a][:, None, 1])
        gate = (speed[grp[a]] * dt[f])[:, None]
        assert not (cand & (np.abs(dist - gate) <= 2 * tol)).any(), "a candidate pair on its gate"
        near = cand & (dist <= gate + 2 * tol)
        assert (near.sum(0) <= 1).all() and (near.sum(1) <= 1).all(), "a box with two candidates: the assignment is not forced"
        n_pos += int(near.sum())
    assert n_pos >= 8, "too few associated boxes for the case to mean anything"


@functools.lru_cache(maxsize=None)
def expected():
    """The oracle's pass over the batch (tests.helpers.oracle_batch) and the velocity stage composed on it by the host statement:
    (oracle arrays, velocity dict).  Asserts the builder condition and the known velocities."""
    from oracle import oracle as orc
    from tests.helpers import oracle_batch
    b = batch()
    exp = oracle_batch(orc, b.frames, b.lanes, b.frame_lane, b.hb)
    assert_robust(b.hb, exp["box"], exp["flags"])
    vel = host_velocity(b.hb, exp["box"], exp["flags"])
    check_known_velocities(b.hb, exp["flags"], exp["medoid_pos"], vel, 1e-9)
    return exp, vel


def stable_masks(hb, medoid_pos):
    """Masks whose medoid is the same list position in every frame of their scene (mask j of frame k is mask j of frame 0): the same
    physical point, moved by exactly k D.  The medoid's Gram-form sums are not translation invariant, so a near-tie between two points
    of a list can fall differently from frame to frame; such a mask has moved by something else and is left out of the known answers."""
    per = np.asarray(medoid_pos).reshape(2, FRAMES_PER_SCENE, -1)
    assert np.array_equal(np.diff(hb.mask_off), np.full(2 * FRAMES_PER_SCENE, per.shape[2]))
    same = (per == per[:, :1]).all(1) & (per[:, 0] >= 0)
    return np.repeat(same[:, None, :], FRAMES_PER_SCENE, 1).reshape(-1)


def check_known_velocities(hb, flags, medoid_pos, vel, tol):
    """Every kept box of a stable mask with a match moves at its scene's velocity; every frame holds such boxes, scene 0 through every
    kind of difference."""
    kept = (np.asarray(flags) & 3) == 3
    scene = np.repeat(np.arange(2), FRAMES_PER_SCENE)[hb.mask_frame]
    moving = kept & (vel["vel_src"] > 0) & stable_masks(hb, medoid_pos)
    assert np.abs(vel["vel"][moving] - VELOCITY[scene[moving]]).max() <= tol
    for f in range(2 * FRAMES_PER_SCENE):
        assert (moving & (hb.mask_frame == f)).sum() >= 2, f
    assert set(vel["vel_src"][moving & (scene == 0)].tolist()) == {1, 2, 3}
    return moving


def all_four_options():
    """The other four opt-in stages of the tests, as LiftEngine keywords."""
    from cm3d_amd import nms as nmsmod
    from cm3d_amd.bevfit import YawFit
    from cm3d_amd.cluster import DepthCluster
    from cm3d_amd.drivable import Stage2Filters
    return dict(cluster=DepthCluster(1.0, 3), filters=Stage2Filters(lane_max_dist=2.5), yaw=YawFit(min_points=5),
                nms=nmsmod.RotatedNms(measure="cover", class_agnostic=True, thr=0.0))


@functools.lru_cache(maxsize=None)
def expected_all_four():
    """The pass with all four options composed on the CPU -- optin_pass_cases.expected (clustering, filter), yaw_fit_pass_cases.fitted,
    optin_pass_cases.rotated_keep -- and the velocity stage on its box rows and final flags: (box, flags, velocity dict).  Asserts
    the builder condition for that kept set."""
    from oracle import oracle as orc
    from tests import optin_pass_cases as oc, yaw_fit_pass_cases as yc
    b, o = batch(), all_four_options()
    exp = oc.expected(orc, b.frames, b.lanes, b.frame_lane, b.hb, cluster=o["cluster"], filters=o["filters"], base=expected()[0])
    fit = yc.fitted(orc, b, exp, o["yaw"])
    flags = (fit["flags"] & 1) | (oc.rotated_keep(fit["box"], fit["flags"], b.hb, o["nms"]) << 1)
    assert (flags != expected()[0]["flags"]).any() and (fit["yaw_src"] > 0).any()       # the options decide something
    assert_robust(b.hb, fit["box"], flags)
    return fit["box"], flags, host_velocity(b.hb, fit["box"], flags)
