"""Batches and the CPU composition for the tests that keep passes with ALL TEN opt-in stages in flight
(tests/test_gpu_all_stages_in_flight.py): cluster, filters, yaw fit, placement, rotated NMS inside the native pass call, and vertical,
ground, velocity, tracks and size as separate library calls behind it.  Several DIFFERENT batches for one set of engine options, so that
a slot of a LiftPipeline that reads anything of its neighbour's -- lists, frame links, frame times, matches, a workspace, the raw rows
of a frame -- differs from the lone engine on its own batch.  Numpy, the oracle and the host statements of cm3d_amd only.

nuScenes, "ten": four batches built the way box_size_pass_cases.batch() is built -- velocity_pass_cases.scene_frames at
box_size_pass_cases.config()'s image size (moving scenes, frame links, the synthetic sweeps' own ground), yaw_fit_pass_cases.add_l_vehicle
as the last mask of every frame, a lane table of one yaw per batch.  Batch 0 is box_size_pass_cases.batch() itself.

Waymo layout: three batches like box_ground_cases.pass_batch("waymo") (rows on the vehicle removed, ground sheet, L vehicle) at the
frame indices and counts of inflight_cases.WAYMO_RECIPES; no velocity, tracks or size there, the boxes are in the vehicle frame.

tests/test_inflight_all_cases_host.py asserts on the CPU that the batches hold what they are for."""
import dataclasses
import functools
from types import SimpleNamespace

import numpy as np

from cm3d_amd import boxground, boxplace, boxvertical
from cm3d_amd import tracks as T
from tests import box_ground_cases as gc
from tests import box_size_pass_cases as sp
from tests import inflight_cases as ic
from tests import velocity_pass_cases as pc
from tests import yaw_fit_pass_cases as yc

# (first scene, scenes, frames per scene, n_masks of the config -- the L vehicle adds one mask per frame --, lane yaw)
RECIPES = ((0, 2, 3, 8, pc.LANE_YAW), (2, 1, 3, 7, 0.9), (2, 2, 2, 9, -0.6), (0, 1, 4, 10, 1.7))
TR = (2, "mean", 2)                                 # min_length, score, smooth_window of the track stage
G, V = boxground.BoxGround(), boxvertical.BoxVertical()

# the per-mask arrays every stage leaves, by the names of LiftEngine.download (what composed() returns under `stages`)
STAGE_KEYS = dict(cluster=("cl_count", "cl_status"), filters=("medoid_pos_kept",), yaw=("yaw_src", "fit_status", "fit_k", "fit_rect"),
                  place=("place_src", "place_pushed"), nms=("flags",), velocity=("next_match", "prev_match", "vel"),
                  tracks=("track_id", "track_pos", "track_len", "vel_smooth"), size=sp.SIZE_KEYS, vertical=boxvertical.RESULTS,
                  ground=boxground.RESULTS)


def _nusc_batch(k):
    from cm3d_amd import lifting
    first, n_scenes, per_scene, n_masks, yaw = RECIPES[k]
    if k == 0:
        b = sp.batch()
        assert (first, n_scenes, per_scene, n_masks, yaw) == (0, 2, pc.FRAMES_PER_SCENE, sp.config().n_masks, pc.LANE_YAW)
        return b
    cfg = dataclasses.replace(sp.config(), n_masks=n_masks)
    frames = [sp._own_lists(f) for f in pc.scene_frames(cfg, n_scenes, per_scene, first)]
    for f in frames:
        yc.add_l_vehicle(f, yaw)
    lanes, frame_lane = [pc.lane_table(yaw)], [0] * len(frames)
    classes = lifting.ClassTable.nuscenes()
    hb = lifting.pack_frames(frames, lanes, frame_lane, classes)
    return SimpleNamespace(name=f"ten{k}", frames=frames, lanes=lanes, frame_lane=frame_lane, hb=hb, classes=classes,
                           l_masks=[int(m) - 1 for m in hb.mask_off[1:]])


@functools.lru_cache(maxsize=None)
def nusc_batches():
    """The four nuScenes batches (name, frames, lanes, frame_lane, hb, classes, l_masks)."""
    return tuple(_nusc_batch(k) for k in range(len(RECIPES)))


def ten_options():
    """LiftEngine keywords of the nuScenes set: all ten opt-in stages."""
    return dict(pc.all_four_options(), place=sp.P, velocity=pc.settings()[0], tracks=T.Tracks(*TR), size=sp.S, vertical=V, ground=G)


@functools.lru_cache(maxsize=None)
def waymo_batches():
    return tuple(gc.pass_batch("waymo", first, n) for first, n in ic.WAYMO_RECIPES)


def waymo_options():
    """inflight_cases.waymo_options() -- cluster, lane filter, yaw fit, rotated NMS on the Waymo class table -- plus placement, vertical
    and ground."""
    return dict(ic.waymo_options(), place=sp.P, vertical=V, ground=G)


def _place_bound(hb):
    return min(32 * ((int(np.diff(hb.mask_off).max()) + 31) // 32), 1024)          # the engine's launch bound: 32 masks per plane of hit words


def composed(orc, b):
    """The whole ten-stage chain of a nuScenes batch on the CPU, nothing from the device, in the stage order of LiftEngine.run:
    optin_pass_cases.expected with cluster and filters on; box_size_pass_cases.composed on it (yaw fit, placement, rotated NMS,
    velocity, tracks, size); box_ground_cases.pass_expected on the centres the placement left -- vertical and ground stand in front of
    velocity, tracks and size and write column 2 only, which none of those reads.  Returns a dict: plain (oracle_batch), front, before
    and size (box_size_pass_cases.composed's pair), circle_flags and rotated_flags (what the placement's circle NMS left, and what the
    rotated NMS made of it, in front of the track stage), vert, ground, box (the final rows: the size stage's with column 2 from the ground stage), stages ({stage: {key: array}}, STAGE_KEYS)."""
    from tests import optin_pass_cases as oc
    from tests.helpers import oracle_batch
    o, hb = ten_options(), b.hb
    plain = oracle_batch(orc, b.frames, b.lanes, b.frame_lane, hb)
    front = oc.expected(orc, b.frames, b.lanes, b.frame_lane, hb, cluster=o["cluster"], filters=o["filters"], base=plain)
    before, out = sp.composed(orc, front=front, nms=o["nms"], tracks=TR, y=o["yaw"], b=b)
    vert, ground = gc.pass_expected(b, front, before["box"], before["flags"], G, V)
    fit = yc.fitted(orc, b, front, o["yaw"])          # (once more, for what box_size_pass_cases.composed does not hand back)
    pl = boxplace.box_place_host(fit["box"], fit["flags"], hb.mask_off, fit["fit_rect"], fit["yaw_src"], b.classes.prior_wlh,
                                 b.classes.nms_group, b.classes.nms_thr, hb.ego_xyz, sp.P.thin, _place_bound(hb))
    assert np.array_equal(pl["place_src"], before["place_src"])
    rotated_flags = (pl["flags"] & 1) | (oc.rotated_keep(pl["box"], pl["flags"], hb, o["nms"]) << 1)
    box = out["box"].copy()
    box[:, 2] = ground["box"][:, 2]
    have = dict(before, **{k: out[k] for k in sp.SIZE_KEYS}, **{k: vert[k] for k in boxvertical.RESULTS},
                **{k: ground[k] for k in boxground.RESULTS}, cl_count=np.diff(front["cl_off"]), place_pushed=pl["place_pushed"],
                flags=out["flags"])
    stages = {s: {k: np.ascontiguousarray(have[k]) for k in keys} for s, keys in STAGE_KEYS.items()}
    return dict(plain=plain, front=front, before=before, size=out, circle_flags=pl["flags"], rotated_flags=rotated_flags, vert=vert,
                ground=ground, box=box, stages=stages)


def composed_waymo(orc, b):
    """The Waymo chain on the CPU up to what the three added stages see: optin_pass_cases.expected (cluster, lane filter),
    yaw_fit_pass_cases.fitted, boxplace.box_place_host (the sensor is the origin of the vehicle frame), then the vertical and the ground
    stage's host statements on the placed centres (they read bit 0 of the flags only, which the rotated NMS leaves).  Returns a dict:
    front, fit, place, vert, ground."""
    from tests import optin_pass_cases as oc
    from tests.helpers import oracle_batch
    o, hb = waymo_options(), b.hb
    plain = oracle_batch(orc, b.frames, b.lanes, b.frame_lane, hb)
    front = oc.expected(orc, b.frames, b.lanes, b.frame_lane, hb, cluster=o["cluster"], filters=o["filters"], base=plain)
    fit = yc.fitted(orc, b, front, o["yaw"])
    pl = boxplace.box_place_host(fit["box"], fit["flags"], hb.mask_off, fit["fit_rect"], fit["yaw_src"], b.classes.prior_wlh,
                                 b.classes.nms_group, b.classes.nms_thr, None, sp.P.thin, _place_bound(hb))
    vert, ground = gc.pass_expected(b, front, pl["box"], pl["flags"], G, V)
    return dict(front=front, fit=fit, place=pl, vert=vert, ground=ground)
