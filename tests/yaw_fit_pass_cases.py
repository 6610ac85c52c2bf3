"""Batches and the composed CPU expectation of the yaw-fitted pass (LiftEngine(yaw=YawFit(...)), alone and behind the clustered and the
filtered pass).  Numpy, the oracle and the host statements of cm3d_amd only; nothing here touches the device.

The batches are tests/optin_pass_cases.py's kind -- synthetic frames, a few dozen masks -- with two changes: the lane tables are
parallel lanes of ONE direction (parallel_lanes), so that "across the lane" means something, and every frame carries one more mask, a
car whose points are two faces of a rectangle that stands 100 degrees off that direction (add_l_vehicle): the lane's yaw is wrong for
it by more than any tolerance, and the fit is right within its grid.

fitted() states the pass on the CPU in the pass's own order, from an expectation of the pass in front of it (optin_pass_cases.expected):
bevfit.bev_fit_lists on the oracle's lists (the clustered ones where the expectation has them), bevfit.yaw_select_host on the oracle's
lane results (with medoid_pos_kept where the expectation has it), per mask oracle.box_assemble / box_assemble_waymo with the selected
yaw, the oracle's circle NMS per frame."""
from types import SimpleNamespace

import numpy as np

from cm3d_amd import bevfit
from cm3d_amd import geometry as geo
from cm3d_amd import rle as rlemod
from cm3d_amd import synthetic as syn
from tests import optin_pass_cases as oc

LANE_YAW = {"nusc": 0.35, "waymo": -1.1}
OFF_LANE = np.pi / 2 + 0.17            # the L vehicle's heading relative to the lanes
CAR_L, CAR_W = 4.4, 1.8


def parallel_lanes(centre_xy, yaw, extent=120.0, spacing=6.0, step=0.5):
    """(x, y, yaw) rows of parallel straight lanes of direction `yaw` around centre_xy."""
    s = np.arange(-extent, extent, step)
    rows = []
    for off in np.arange(-extent, extent, spacing):
        x, y = s * np.cos(yaw) - off * np.sin(yaw), s * np.sin(yaw) + off * np.cos(yaw)
        rows.append(np.stack([x + centre_xy[0], y + centre_xy[1], np.full_like(s, yaw)], 1))
    return np.concatenate(rows, 0)


# ------------------------------------------------------------------------------------------------ the L vehicle
def _sweep_to_frame(xf, p):
    xf = np.asarray(xf, np.float64)
    return (p @ xf[0:9].reshape(3, 3).T + xf[9:12]) @ xf[12:21].reshape(3, 3).T + xf[21:24]


def _frame_to_sweep(xf, p):
    xf = np.asarray(xf, np.float64)
    return ((p - xf[21:24]) @ xf[12:21].reshape(3, 3) - xf[9:12]) @ xf[0:9].reshape(3, 3)


def _project(rec, p):
    """Pixel coordinates and depth of points of the kernels' frame through a camera record, in float64."""
    for s in range(int(rec[54])):
        tp, R, tq = geo.cam_stage(rec, s)
        p = (p + tp) @ R.T + tq
    uvw = p @ geo.cam_K(rec).T
    with np.errstate(divide="ignore", invalid="ignore"):
        return uvw[:, 0] / uvw[:, 2], uvw[:, 1] / uvw[:, 2], p[:, 2]


def _unproject_camera_point(rec, pc):
    p = np.asarray(pc, np.float64).reshape(1, 3)
    for s in reversed(range(int(rec[54]))):
        tp, R, tq = geo.cam_stage(rec, s)
        p = (p - tq) @ R - tp
    return p[0]


def add_l_vehicle(fr, lane_yaw, to_lane=None, cam=0, depth=12.0):
    """Adds to the frame (in place) a car seen by camera `cam`, `depth` metres in front of it: the two faces of a CAR_L x CAR_W rectangle
    that look at the camera, as rows of sweep 0 (noise-free up to float32), a mask around their projection labelled "car", and takes out
    of every sweep the rows that would fall into that mask beside them.  The car's heading in the lanes' frame is lane_yaw + OFF_LANE;
    to_lane: 4x4 from the frame of the kernels (nuScenes: global, None; Waymo: vehicle) to the lanes' frame.  Returns the heading in the
    lanes' frame, as the transformed long face has it."""
    T = np.eye(4) if to_lane is None else np.asarray(to_lane, np.float64).reshape(4, 4)
    rec = np.asarray(fr.cams[cam], np.float64)
    centre = _unproject_camera_point(rec, [0.4, 0.3, depth])
    eye = _unproject_camera_point(rec, [0.0, 0.0, 0.0])
    h = lane_yaw + OFF_LANE - np.arctan2(T[1, 0], T[0, 0])
    ch, sh = np.cos(h), np.sin(h)
    vu, vw = (eye[0] - centre[0]) * ch + (eye[1] - centre[1]) * sh, -(eye[0] - centre[0]) * sh + (eye[1] - centre[1]) * ch
    nl, ns, nz = 48, 20, 5
    u = np.concatenate([np.linspace(-CAR_L / 2, CAR_L / 2, nl), np.full(ns, np.sign(vu) * CAR_L / 2)])
    w = np.concatenate([np.full(nl, np.sign(vw) * CAR_W / 2), np.linspace(-CAR_W / 2, CAR_W / 2, ns)])
    xy = np.stack([centre[0] + u * ch - w * sh, centre[1] + u * sh + w * ch], 1)
    pts = np.concatenate([np.concatenate([xy, np.full((len(xy), 1), centre[2] + dz)], 1) for dz in np.linspace(-0.45, 0.35, nz)], 0)
    px, py, pz = _project(rec, pts)
    assert (pz > 2.5).all() and px.min() > 8 and px.max() < fr.width - 8 and py.min() > 8 and py.max() < fr.height - 8
    cx, cy = 0.5 * (px.min() + px.max()), 0.5 * (py.min() + py.max())
    ax, ay = 0.75 * (px.max() - px.min()) + 3.0, 0.75 * (py.max() - py.min()) + 3.0
    for s in range(len(fr.sweeps_raw)):
        raw = np.asarray(fr.sweeps_raw[s])
        qx, qy, qz = _project(rec, _sweep_to_frame(fr.sweep_xf[s], raw[:, :3].astype(np.float64)))
        with np.errstate(invalid="ignore"):
            inside = (qz > 0.1) & (np.abs(qx - cx) <= ax + 3) & (np.abs(qy - cy) <= ay + 3)
        fr.sweeps_raw[s] = np.ascontiguousarray(raw[~inside])
    rows = np.zeros((len(pts), fr.sweeps_raw[0].shape[1]), np.float32)
    rows[:, :3] = _frame_to_sweep(fr.sweep_xf[0], pts)
    rows[:, 3] = 1.0
    fr.sweeps_raw[0] = np.ascontiguousarray(np.concatenate([fr.sweeps_raw[0], rows], 0))
    fr.rles.append({"size": [fr.width, fr.height], "counts": rlemod.counts_to_string(syn._ellipse_rle(cx, cy, ax, ay, fr.width, fr.height))})
    fr.labels.append("car")
    fr.scores.append(0.93)
    fr.cam_nums.append(int(cam))
    d = (T[:3, :3] @ np.array([ch, sh, 0.0]))
    return float(np.arctan2(d[1], d[0]))


_BATCHES, _PLAIN, _EXP = {}, {}, {}


def batch(name, first=0, n_frames=2):
    """`nusc` or `waymo`: synthetic frames first .. first + n_frames - 1 (two frames from 0 unless told otherwise), a lane table of
    parallel lanes per frame, an L vehicle as the last mask of every frame.  Fields as optin_pass_cases.batch, plus classes, l_masks
    (the L vehicles' mask numbers) and l_heading (their headings in the lanes' frame)."""
    key = name if (first, n_frames) == (0, 2) else (name, first, n_frames)         # plain(), expected_of() know the default batch by its name
    if key in _BATCHES:
        return _BATCHES[key]
    from cm3d_amd import lifting
    ids = range(first, first + n_frames)
    if name == "nusc":
        cfg = syn.config("tiny", n_points=9000, n_masks=20, width=512, height=288, ratio=0.32, max_area=12000.0)
        frames = [syn.make_frame(cfg, i) for i in ids]
        classes = lifting.ClassTable.nuscenes()
        lanes = [parallel_lanes(f.ego_xyz[:2], LANE_YAW[name]) for f in frames]
        heading = [add_l_vehicle(f, LANE_YAW[name]) for f in frames]
    elif name == "waymo":
        cfg = syn.config("tiny", n_cams=5, n_points=9000, n_masks=17, width=512, height=288, ratio=0.32, max_area=12000.0)
        frames = [syn.make_waymo_frame(cfg, i) for i in ids]
        classes = lifting.ClassTable.waymo()
        poses = [np.asarray(f.pose, np.float64).reshape(4, 4) for f in frames]
        lanes = [parallel_lanes(P[:2, 3], LANE_YAW[name]) for P in poses]
        heading = [add_l_vehicle(f, LANE_YAW[name], P) for f, P in zip(frames, poses)]
    else:
        raise KeyError(name)
    frame_lane = list(range(n_frames))
    hb = lifting.pack_frames(frames, lanes, frame_lane, classes)
    _BATCHES[key] = SimpleNamespace(name=name, frames=frames, lanes=lanes, frame_lane=frame_lane, hb=hb, classes=classes,
                                    l_masks=[int(m) - 1 for m in hb.mask_off[1:]], l_heading=heading)
    return _BATCHES[key]


def plain(orc, name):
    if name not in _PLAIN:
        b = batch(name)
        _PLAIN[name] = oc._frozen(oc.oracle_batch(orc, b.frames, b.lanes, b.frame_lane, b.hb))
    return _PLAIN[name]


def expected_of(orc, name, cluster=None, filters=None):
    """optin_pass_cases.expected of the batch (the pass in front of the fit), once per process."""
    key = (name, oc._cluster_key(cluster), None if filters is None else (filters.lane_max_dist, filters.vehicle_lane_max_dist))
    if key not in _EXP:
        b = batch(name)
        _EXP[key] = oc._frozen(oc.expected(orc, b.frames, b.lanes, b.frame_lane, b.hb, cluster=cluster, filters=filters, base=plain(orc, name)))
    return _EXP[key]


# ------------------------------------------------------------------------------------------------ the composition
def fitted(orc, b, exp, y):
    """exp (an expectation of the pass in front) with fit_k, fit_rect, fit_status, yaw_src and the box and flags of the yaw-fitted pass."""
    hb = b.hb
    M = hb.n_masks
    if "cl_off" in exp:
        off, xyz = exp["cl_off"], exp["cl_xyz"]
    else:
        off, xyz = exp["hit_off"], oc.hit_xyz_of(hb, exp)
    fit_k, fit_rect, fit_status = bevfit.bev_fit_lists(off, xyz, y.angles, y.d0, y.min_points, y.min_length)
    med = np.asarray(exp["medoid_pos_kept"] if "medoid_pos_kept" in exp else exp["medoid_pos"], np.int32)
    lane32 = [np.asarray(t, np.float64).astype(np.float32).reshape(-1, 3) for t in b.lanes]
    lane_yaw = np.zeros(M, np.float32)
    for m in np.flatnonzero(med >= 0):
        lane_yaw[m] = lane32[b.frame_lane[int(hb.mask_frame[m])]][int(exp["lane_idx"][m]), 2]
    waymo = hb.pose_rt is not None
    yaw, src = bevfit.yaw_select_host(fit_rect, fit_status, med, hb.class_id, orc.IS_VEHICLE.astype(np.int32), exp["lane_dist"], lane_yaw,
                                      y.lane_min_dist, hb.pose_rt if waymo else None, hb.mask_frame)
    box, flags = np.zeros((M, 10)), np.zeros(M, np.int32)
    box[:, 3] = 1.0
    for fi in range(hb.n_frames):
        m0, m1 = int(hb.mask_off[fi]), int(hb.mask_off[fi + 1])
        vi = m0 + np.flatnonzero(med[m0:m1] >= 0)
        for m in vi:
            cls = int(hb.class_id[m])
            if waymo:
                cg = orc.centroid_transform(exp["centroid"][m], hb.pose_rt[fi])
                t, head = orc.box_assemble_waymo(cg, hb.pose_inv[fi], orc.PRIORS_WLH[cls], yaw[m], orc.IS_VEHICLE[cls])
                box[m, 0:3], box[m, 3], box[m, 4] = t, head, 0.0
            else:
                t, q = orc.box_assemble(exp["centroid"][m], orc.PRIORS_WLH[cls], yaw[m], b.frames[fi].ego_xyz, orc.IS_VEHICLE[cls])
                box[m, 0:3], box[m, 3], box[m, 4] = t, q[0], q[3]
            box[m, 6] = exp["lane_dist"][m]
        keep = np.zeros(0, bool)
        if vi.size:
            lab = orc.WAYMO_NMS_GROUP[hb.class_id[vi]] if waymo else np.asarray(hb.class_id[vi], np.int32)
            keep = orc.circle_nms(box[vi, 0], box[vi, 1], np.asarray(hb.score, np.float64)[vi], lab, orc.WAYMO_NMS_THR if waymo else orc.NMS_THR)
        flags[vi] = 1 | (keep.astype(np.int32) << 1)
    box[:, 5] = yaw
    box[:, 7], box[:, 8], box[:, 9] = hb.score, hb.class_id, flags
    return dict(exp, fit_k=fit_k, fit_rect=fit_rect, fit_status=fit_status, yaw_src=src, yaw=yaw, box=box, flags=flags)
