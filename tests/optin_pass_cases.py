"""Batches and the composed CPU expectation of the opt-in passes (the clustered pass, the filtered pass, both, and what the rotated-box
NMS then sees).  Numpy, the oracle and the host statements of cm3d_amd only; nothing here touches the device.

expected() states a pass on the CPU in the pass's own order: the plain pass by the oracle (tests.helpers.oracle_batch), the depth
clustering of its lists by cluster.cluster_lists, the medoid of every clustered list by oracle.medoid, stage 2 by oracle.stage2_frame on
those medoids, the filters by drivable.filter_rule and stage 2 again on the masks they keep.  Three batch recipes reach what the tiny
frames of the other modules do not (tests/test_optin_pass_cases_host.py asserts that each holds what it is for):

mid    lists of up to 472 points whose clusters end in every range of the medoid stage below 448 -- a raw list above MD_BATCH_LONG
       whose cluster is below it;
deep   lists of thousands of points: a list above the clustering's LDS limit that loses points, clustered lists far above 448;
many   70 and 130 masks in a frame: 5 hit-word planes, so a rotated-NMS bound of 160 -- strictly between its register route and 1024.
"""
from types import SimpleNamespace

import numpy as np

from cm3d_amd import cluster as clustermod
from cm3d_amd import drivable
from cm3d_amd import nms as nmsmod
from cm3d_amd import synthetic as syn
from tests.helpers import oracle_batch

BATCH_NAMES = ("mid", "deep", "many")
CLUSTER_KEYS = ("cl_off", "cl_tile_off", "cl_status", "cl_idx", "cl_xyz")
MD_BATCH_LONG = 448            # csrc/medoid.hip: a batch with a longer list takes the two-pass medoid route


def _recipe(name):
    """(frames, DepthCluster) of a batch."""
    if name == "mid":
        cfg = syn.config("tiny", n_points=30000, n_sweeps=5, n_masks=14, width=512, height=288, ratio=0.32)
        return [syn.make_frame(cfg, 0), syn.make_frame(cfg, 1)], clustermod.DepthCluster(1.0, 20)
    if name == "deep":
        cfg = syn.config("tiny", n_points=60000, n_sweeps=4, n_masks=5, width=512, height=288, ratio=0.32, min_area=30000.0,
                         max_area=120000.0, empty_mask_prob=0.0, duplicate_prob=0.0, seed=1)
        return [syn.make_frame(cfg, 0)], clustermod.DepthCluster(0.3, 20)
    if name == "many":
        return ([syn.make_frame(syn.config("tiny", n_masks=70, seed=979), 0),
                 syn.make_frame(syn.config("tiny", n_masks=130, n_points=6000, duplicate_prob=0.5, seed=3), 1)], clustermod.DepthCluster(0.6, 6))
    raise KeyError(name)


_BATCHES, _PLAIN, _CLUSTERED = {}, {}, {}


def batch(name):
    """The batch `name`, built once per process: frames, lanes, frame_lane, hb (lifting.pack_frames), cluster (its DepthCluster)."""
    if name not in _BATCHES:
        from cm3d_amd import lifting
        frames, c = _recipe(name)
        lanes = [syn.make_lane_table(frames[0].ego_xyz[:2], 1500, seed=2)]
        frame_lane = [0] * len(frames)
        _BATCHES[name] = SimpleNamespace(name=name, frames=frames, lanes=lanes, frame_lane=frame_lane,
                                         hb=lifting.pack_frames(frames, lanes, frame_lane), cluster=c)
    return _BATCHES[name]


def _cluster_key(c):
    return None if c is None else (c.eps, c.min_points, c.pick)


def _frozen(d):
    for v in d.values():
        if isinstance(v, np.ndarray):
            v.setflags(write=False)
    return d


def plain(orc, name):
    """oracle_batch of the batch `name`, computed once per process (read-only arrays)."""
    if name not in _PLAIN:
        b = batch(name)
        _PLAIN[name] = _frozen(oracle_batch(orc, b.frames, b.lanes, b.frame_lane, b.hb))
    return _PLAIN[name]


def expected_of(orc, name, cluster=None, filters=None, tables=None):
    """expected() of the batch `name`; the plain pass and every clustered expectation are computed once per process."""
    b = batch(name)
    key = (name, _cluster_key(cluster))
    if key not in _CLUSTERED:
        _CLUSTERED[key] = _frozen(expected(orc, b.frames, b.lanes, b.frame_lane, b.hb, cluster=cluster, base=plain(orc, name)))
    exp = _CLUSTERED[key]
    if filters is None:
        return exp
    return _frozen(_filtered(orc, b.frames, b.lanes, b.frame_lane, b.hb, exp, filters, tables))


# ------------------------------------------------------------------------------------------------ the composition
def hit_xyz_of(hb, exp):
    """Coordinates of every listed point from the oracle's cloud (tests.test_gpu_parity._expected_hit_xyz)."""
    from tests.test_gpu_parity import _expected_hit_xyz
    return _expected_hit_xyz(hb, exp)


def stage2_records(orc, frames, lanes, frame_lane, hb, centroid, med):
    """Stage 2 and the circle NMS of every frame on `centroid` (M, 3) float32 and `med` (M,), in oracle_batch's record layout:
    lane_idx, lane_dist, box (M, 10), flags."""
    lane_idx, lane_dist, box, flags = [], [], [], []
    centroid, med = np.asarray(centroid, np.float32), np.asarray(med, np.int32)
    for fi, fr in enumerate(frames):
        m0, m1 = int(hb.mask_off[fi]), int(hb.mask_off[fi + 1])
        if hb.pose_rt is not None:
            s2 = orc.stage2_frame_waymo(centroid[m0:m1], med[m0:m1], hb.class_id[m0:m1], hb.score[m0:m1], lanes[frame_lane[fi]],
                                        hb.pose_rt[fi], hb.pose_inv[fi])
            s2["rotation"] = np.zeros((m1 - m0, 4))
            s2["rotation"][:, 0] = s2["heading"]
            s2["rotation"][~s2["valid"], 0] = 1.0
        else:
            s2 = orc.stage2_frame(centroid[m0:m1], med[m0:m1], hb.class_id[m0:m1], hb.score[m0:m1], lanes[frame_lane[fi]], fr.ego_xyz)
        b = np.zeros((m1 - m0, 10))
        b[:, 0:3] = np.where(s2["valid"][:, None], s2["translation"], 0.0)
        b[:, 3] = np.where(s2["valid"], s2["rotation"][:, 0], 1.0)
        b[:, 4] = np.where(s2["valid"], s2["rotation"][:, 3], 0.0)
        b[:, 5] = s2["yaw"]
        b[:, 6] = np.where(s2["valid"], s2["lane_dist"], 0.0)
        b[:, 7], b[:, 8] = hb.score[m0:m1], hb.class_id[m0:m1]
        b[:, 9] = s2["valid"].astype(np.int32) | (s2["keep"].astype(np.int32) << 1)
        lane_idx.append(s2["lane_idx"]); lane_dist.append(s2["lane_dist"])
        box.append(b)
        flags.append(s2["valid"].astype(np.int32) | (s2["keep"].astype(np.int32) << 1))
    return dict(lane_idx=np.concatenate(lane_idx), lane_dist=np.concatenate(lane_dist), box=np.concatenate(box, 0), flags=np.concatenate(flags))


def expected_filtered(orc, hb, plain, lanes, frame_lane, frames, tables, filters):
    """The host restatement: on_road by the host test on the plain pass's medoids, medoid_pos_kept by the rule, box / flags by the
    oracle's stage 2 with med = -1 for the dropped masks (tests/helpers.oracle_batch's record layout)."""
    from cm3d_amd.lifting import ClassTable
    cls = ClassTable.nuscenes()
    has = plain["medoid_pos"] >= 0
    cg = plain["centroid"]
    on_road = None
    if filters.drivable:
        on_road = drivable.points_on_road(tables, cg[:, :2].astype(np.float64), np.asarray(frame_lane)[hb.mask_frame]) * has.astype(np.uint8)
    kept = drivable.filter_rule(plain["medoid_pos"], hb.class_id, plain["lane_dist"], on_road, cls.is_vehicle, cls.needs_road,
                                filters.lane_max_dist, filters.vehicle_lane_max_dist)
    s2 = stage2_records(orc, frames, lanes, frame_lane, hb, cg, kept)
    return dict(on_road=on_road if on_road is not None else np.zeros(hb.n_masks, np.uint8), medoid_pos_kept=kept,
                box=s2["box"], flags=s2["flags"])


def _clustered(orc, frames, lanes, frame_lane, hb, base, c):
    """Steps 2 to 4: the clustering of the oracle's lists, the medoid of every clustered list, stage 2 on those medoids."""
    hit_xyz = hit_xyz_of(hb, base)
    cl_off, cl_tile_off, keep, status = clustermod.cluster_lists(base["hit_off"], hit_xyz, hb.mask_frame, hb.ego_xyz, c.eps, c.min_points, c.pick)
    cl_idx = base["hit_idx"][keep]
    pts = base["points"]
    M = hb.n_masks
    med = np.full(M, -1, np.int32)
    cen = np.full((M, 3), np.nan, np.float32)
    for m in range(M):
        o, e = int(cl_off[m]), int(cl_off[m + 1])
        if e > o:
            rows = int(base["pt_off"][int(hb.mask_frame[m])]) + cl_idx[o:e]
            med[m] = orc.medoid(pts, rows)
            cen[m] = pts[rows[med[m]], :3]
    out = dict(base, cl_off=cl_off, cl_tile_off=cl_tile_off, cl_status=status, cl_idx=cl_idx, cl_xyz=hit_xyz[keep], medoid_pos=med,
               centroid=np.where(np.isnan(cen), np.float32(0), cen).astype(np.float32))
    out.update(stage2_records(orc, frames, lanes, frame_lane, hb, cen, med))
    return out


def _filtered(orc, frames, lanes, frame_lane, hb, exp, filters, tables):
    """Step 5 on an expectation without filters."""
    return dict(exp, **expected_filtered(orc, hb, exp, lanes, frame_lane, frames, tables, filters))


def expected(orc, frames, lanes, frame_lane, hb, cluster=None, filters=None, tables=None, base=None):
    """Arrays shaped like LiftEngine.download(full=True) (plus `cl_tile_off`, which the engine keeps in eng.b) of a pass of an engine
    with these options.  base: oracle_batch of the same arguments, where the caller has it already.
    1. oracle_batch: raw lists, cloud, plain medoids and boxes;
    2. cluster: cluster.cluster_lists on the oracle's hit_off, the listed points' coordinates and hb.ego_xyz -> cl_*;
    3. per mask oracle.medoid over (frame base + the mask's cl_idx) -> medoid_pos (a position in the clustered list), centroid;
    4. per frame oracle.stage2_frame (Waymo layout: stage2_frame_waymo) on those -> lane_idx, lane_dist, box, flags;
    5. filters: drivable.filter_rule on those values (on_road: drivable.points_on_road) -> medoid_pos_kept; stage 2 again with
       med = -1 for the dropped masks -> box, flags."""
    out = dict(base if base is not None else oracle_batch(orc, frames, lanes, frame_lane, hb))
    if cluster is not None:
        out = _clustered(orc, frames, lanes, frame_lane, hb, out, cluster)
    if filters is not None:
        out = _filtered(orc, frames, lanes, frame_lane, hb, out, filters, tables)
    return out


# ------------------------------------------------------------------------------------------------ what the tests derive from it
def lane_filters(exp):
    """The filters of the tests, from an expectation without filters: the median of lane_dist over the masks with a box, and 0.75 of
    it for the pushed classes."""
    thr = float(np.median(exp["lane_dist"][exp["medoid_pos"] >= 0]))
    return drivable.Stage2Filters(lane_max_dist=thr, vehicle_lane_max_dist=0.75 * thr)


def rotated_keep(box, flags, hb, r, classes=None):
    """nms.rotated_nms_host on the records of box rows (nuScenes layout), the boxes with flags & 1 taking part: keep (M,) int32."""
    if classes is None:
        from cm3d_amd.lifting import ClassTable
        classes = ClassTable.nuscenes()
    box = np.asarray(box, np.float64)
    cls = box[:, 8].astype(int)
    return nmsmod.rotated_nms_host(nmsmod.records_from_boxes(box, classes.prior_wlh, False), box[:, 7], classes.nms_group[cls], hb.mask_off,
                                   r.thr_by_group(classes), r.measure, r.class_agnostic, take=(np.asarray(flags) & 1) == 1)


def obb_expected(exp, max_gap_excluded):
    """kitti.obb_canonical on the clustered lists of an expectation: (yaw (M,), status (M,), pinned (M,) bool).  A list of at most 3
    points is skipped (status 1, yaw NaN), one without a hull has status 2 and yaw 0; `pinned` marks the fitted lists whose relative
    eigenvalue gap is at least `max_gap_excluded` (below it a 1e-9 comparison cannot pin the eigenvectors)."""
    import warnings
    from cm3d_amd import kitti as kt
    from tests.test_gpu_obb import _eig_gap
    off = exp["cl_off"]
    M = off.size - 1
    yaw, st, pinned = np.zeros(M), np.zeros(M, np.int32), np.zeros(M, bool)
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        for m in range(M):
            c = exp["cl_xyz"][off[m]:off[m + 1], :3]
            if len(c) <= 3:
                yaw[m], st[m] = np.nan, kt.OBB_SKIPPED
                continue
            try:
                yaw[m], _, vidx = kt.obb_canonical(c)
            except Exception:
                st[m] = kt.OBB_NO_HULL
                continue
            pinned[m] = _eig_gap(c, vidx) >= max_gap_excluded
    return yaw, st, pinned
