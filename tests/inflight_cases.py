"""Batches for the tests that keep passes with opt-in stages in flight (tests/test_gpu_optin_in_flight.py): several DIFFERENT batches
for one set of engine options, so that a slot of a LiftPipeline that reads anything of its neighbour's -- lists, lane tables, polygon
tables, frame links -- differs from the lone engine on its own batch.  Numpy, the oracle and the host statements of cm3d_amd only.

nuScenes: the moving scenes of tests/velocity_pass_cases.py (moved_frame).  The batches differ in frame count, in masks per frame
(so no two have equal mask_off), in the scenes they show and in the lane table: every batch's lanes have ONE yaw of their own, and that
yaw is in every pushed box.  Batch 0 is velocity_pass_cases.batch() itself, whose five-option result test_gpu_velocity_pass pins to the CPU
composition.  Two small extra batches bring the number of table sets to six: with the drivable filter on, a table set takes two entries
of the engines' shared cache of eight.

Waymo layout: batches made like yaw_fit_pass_cases.batch("waymo") at other frame indices and frame counts.

tests/test_inflight_cases_host.py asserts on the CPU that the batches hold what they are for."""
import dataclasses
import functools
from types import SimpleNamespace

import numpy as np

from cm3d_amd import synthetic as syn
from tests import velocity_pass_cases as pc
from tests import yaw_fit_pass_cases as yc

# (first scene, scenes, frames per scene, masks per frame, lane yaw, half side of the drivable square); the first four are THE batches
RECIPES = ((0, 2, 3, 8, pc.LANE_YAW, 60.0), (2, 1, 3, 8, 0.9, 45.0), (2, 2, 2, 9, -0.6, 30.0), (0, 1, 4, 10, 1.7, 75.0),
           (0, 1, 2, 6, 2.4, 50.0), (1, 1, 2, 5, -1.3, 40.0))
N_MAIN = 4
WAYMO_RECIPES = ((2, 2), (4, 3), (7, 1))          # (first frame, frames)
WAYMO_LANE_MAX_DIST = 1.5                         # parallel lanes 6 m apart: a medoid lies up to 3 m from one


def _nusc_batch(k):
    from cm3d_amd import lifting
    first, n_scenes, per_scene, n_masks, yaw, _ = RECIPES[k]
    if k == 0:
        b = pc.batch()
        assert (first, n_scenes, per_scene, n_masks, yaw) == (0, 2, pc.FRAMES_PER_SCENE, pc.config().n_masks, pc.LANE_YAW)
        return SimpleNamespace(frames=b.frames, lanes=b.lanes, frame_lane=b.frame_lane, hb=b.hb)
    cfg = syn.config("tiny", n_masks=n_masks, duplicate_prob=0.25)          # velocity_pass_cases.config() with another mask count
    frames = pc.scene_frames(cfg, n_scenes, per_scene, first)
    lanes, frame_lane = [pc.lane_table(yaw)], [0] * len(frames)
    return SimpleNamespace(frames=frames, lanes=lanes, frame_lane=frame_lane, hb=lifting.pack_frames(frames, lanes, frame_lane))


@functools.lru_cache(maxsize=None)
def nusc_batches():
    """All six nuScenes batches (frames, lanes, frame_lane, hb); the first N_MAIN are the ones the walks use, the last two only add
    table sets."""
    return tuple(_nusc_batch(k) for k in range(len(RECIPES)))


def road_table(k):
    """Batch k's drivable area: one polygon table ([(exterior, holes)]), a square of its own size around EGO0 with the synthetic map's
    24 m hole to the north-east (nusc_io.write_synthetic_dataset)."""
    h, (cx, cy) = RECIPES[k][5], pc.EGO0
    rect = lambda x0, y0, x1, y1: np.array([(x0, y0), (x1, y0), (x1, y1), (x0, y1)], np.float64)
    return [(rect(cx - h, cy - h, cx + h, cy + h), [rect(cx + 20, cy + 20, cx + 44, cy + 44)])]


@functools.lru_cache(maxsize=None)
def drivable_batches():
    """The same six batches, each HostBatch a copy that carries its own polygon table (HostBatch.polygons)."""
    return tuple(SimpleNamespace(frames=b.frames, lanes=b.lanes, frame_lane=b.frame_lane, polygons=[road_table(k)],
                                 hb=dataclasses.replace(b.hb, polygons=[road_table(k)], polygon_key=None))
                 for k, b in enumerate(nusc_batches()))


def five_options(drivable=False):
    """LiftEngine keywords of the nuScenes sets: velocity_pass_cases.all_four_options() plus the velocity stage; drivable: the lane
    filter's Stage2Filters with the drivable-area test on as well."""
    kw = dict(pc.all_four_options(), velocity=pc.settings()[0])
    if drivable:
        kw["filters"] = dataclasses.replace(kw["filters"], drivable=True)
    return kw


@functools.lru_cache(maxsize=None)
def waymo_batches():
    return tuple(yc.batch("waymo", first, n) for first, n in WAYMO_RECIPES)


def waymo_options():
    """Cluster, lane filter, yaw fit and rotated NMS on the Waymo class table; no velocity (its boxes are in the vehicle frame), no
    drivable area."""
    from cm3d_amd import lifting
    from cm3d_amd.drivable import Stage2Filters
    kw = pc.all_four_options()
    return dict(kw, classes=lifting.ClassTable.waymo(), filters=Stage2Filters(lane_max_dist=WAYMO_LANE_MAX_DIST))


def composed(orc, b, drivable_tables=None):
    """The five-option pass of a nuScenes batch composed on the CPU: optin_pass_cases.expected (clustering, filters),
    yaw_fit_pass_cases.fitted, optin_pass_cases.rotated_keep, velocity_pass_cases.host_velocity.  Returns a dict: plain (oracle_batch),
    front (the pass in front of the fit), fit, flags (final), vel."""
    from tests import optin_pass_cases as oc
    from tests.helpers import oracle_batch
    o = five_options(drivable_tables is not None)
    plain = oracle_batch(orc, b.frames, b.lanes, b.frame_lane, b.hb)
    front = oc.expected(orc, b.frames, b.lanes, b.frame_lane, b.hb, cluster=o["cluster"], filters=o["filters"], tables=drivable_tables, base=plain)
    fit = yc.fitted(orc, b, front, o["yaw"])
    flags = (fit["flags"] & 1) | (oc.rotated_keep(fit["box"], fit["flags"], b.hb, o["nms"]) << 1)
    return dict(plain=plain, front=front, fit=fit, flags=flags, vel=pc.host_velocity(b.hb, fit["box"], flags))
