"""GPU: the two stage-2 launches at their seams.  k_lane_nn_grid: the first ring batch (the 5 x 5 cells around the centroid) on cells
of 4 / 5 and 8 / 9 points (either side of a scan round of LG_PF points and of two), a cell above LG_BIG_CELL, a nearest point in ring 3,
a tie, centroids outside the grid, a NaN centroid, an empty table.  k_box_nms: a template over the Waymo pose, LDS by the batch's own
bound (cm3d_box_nms_bounded), the NMS of a frame of up to 64 masks on one wave's registers.  Tiny crafted inputs; every expectation
is the CPU oracle's."""
import numpy as np
import pytest

from tests.test_gpu_stage2 import BOX_TIGHT, NMS_CLASSES, _dev, _lane_lookup, _st, _t

pytestmark = pytest.mark.gpu

H = 4.0                  # LG_CELL0: the cell edge of a table this small
BIG = 12                 # LG_BIG_CELL


def _cell_points(ci, cj, n, rng):
    """n points strictly inside cell (ci, cj) of a grid that starts at (0, 0) with 4 m cells."""
    return np.stack([H * ci + rng.uniform(0.3, 3.7, n), H * cj + rng.uniform(0.3, 3.7, n)], 1)


def _lane_table(rng):
    """A 21 x 21-cell table (corner points pin the grid to [0, 80]^2) with, far from each other: cells of exactly 4, 5 (the LG_PF
    seam), 8, 9 (two rounds of LG_PF and one point more) and 20 points (above LG_BIG_CELL), a lone point three cells from an
    otherwise empty neighbourhood, and two points at the same distance from a centroid between them, the one with the smaller index
    in the cell the search visits later."""
    pts = [np.array([[0.0, 0.0], [80.0, 80.0], [0.0, 80.0], [80.0, 0.0]])]
    pts.append(np.array([[46.0, 50.0]]))                      # index 4: cell (11, 12)
    pts.append(np.array([[42.0, 50.0]]))                      # index 5: cell (10, 12); the centroid (44, 50) is 2 m from both
    pts.append(_cell_points(3, 3, 4, rng))
    pts.append(_cell_points(8, 3, 5, rng))
    pts.append(_cell_points(14, 3, 20, rng))
    pts.append(_cell_points(3, 14, 8, rng))
    pts.append(_cell_points(8, 14, 9, rng))
    pts.append(np.array([[74.0, 30.0]]))                      # cell (18, 7): ring 3 of a centroid in cell (15, 7)
    xy = np.concatenate(pts, 0)
    return np.concatenate([xy, rng.uniform(-np.pi, np.pi, (xy.shape[0], 1))], 1)


def test_lane_search_first_ring_batch_seams(oracle):
    """Centroids in and around cells of 4, 5, 8, 9 and 20 points, one whose nearest point lies in ring 3 (a second batch runs), one between two
    equidistant points (the smaller index wins), some outside the grid, one NaN, and a frame on an empty table: index and distance of
    every one bit for bit the float64 brute force's."""
    rng = np.random.default_rng(5)
    table = _lane_table(rng)
    assert table.shape[0] == 4 + 2 + 4 + 5 + 20 + 8 + 9 + 1
    cent = []
    for ci, cj in ((3, 3), (8, 3), (14, 3), (3, 14), (8, 14)):
        cent += [np.array([H * ci + 2.0, H * cj + 2.0]), np.array([H * ci + 0.01, H * cj + 3.99])]
        cent += list(_cell_points(ci, cj, 6, rng))
        cent += list(np.array([H * ci + 2.0, H * cj + 2.0]) + rng.uniform(-9.0, 9.0, (10, 2)))     # up to two cells off: still the first batch
    n_first = len(cent)
    cent.append(np.array([62.0, 30.0]))                       # cell (15, 7): the 5 x 5 cells around it are empty
    cent.append(np.array([44.0, 50.0]))                       # the tie
    cent += [np.array([-30.0, 40.0]), np.array([200.0, 200.0]), np.array([40.0, -3.0]), np.array([81.0, 81.0])]      # outside the grid
    nan_at = len(cent)
    cent.append(np.array([np.nan, 5.0]))
    cent = np.concatenate([np.array(cent), np.zeros((len(cent), 1))], 1).astype(np.float32)
    K = cent.shape[0]
    # frame 0 -> the table, frame 1 -> an empty table; every centroid once on each
    tables = [table, np.zeros((0, 3))]
    cent2 = np.concatenate([cent, cent[:8]], 0)
    mask_frame = np.concatenate([np.zeros(K), np.ones(8)]).astype(np.int32)
    idx, dist = _lane_lookup(tables, cent2, mask_frame, np.array([0, 1], np.int32), np.zeros(K + 8, np.int32))
    j, d = oracle.lane_nn(cent, table)
    bad = np.flatnonzero((idx[:K] != j) | (dist[:K].view(np.uint64) != d.view(np.uint64)))
    assert bad.size == 0, (bad.tolist(), idx[bad].tolist(), j[bad].tolist())
    assert idx[n_first] == table.shape[0] - 1 and dist[n_first] == 12.0               # found in ring 3
    assert idx[n_first + 1] == 4 and dist[n_first + 1] == 2.0                         # the tie: the smaller index
    assert idx[nan_at] == 0 and np.isinf(dist[nan_at])                                # np.argmin of an all-NaN row
    assert (idx[K:] == 0).all() and np.isinf(dist[K:]).all()                          # the empty table
    l32 = table.astype(np.float32)
    counts = {(int(x // H), int(y // H)) for x, y in l32[:, :2]}
    assert len(counts) == 4 + 2 + 5 + 1                                               # the cells are the ones meant


# ------------------------------------------------------------------------------------------------ boxes + NMS
def _box_call_bounded(frames, tables, frame_lane, classes, bound, pose_inv=None):
    """cm3d_box_nms_bounded over several frames in one call (tests.test_gpu_stage2._box_call with the bound)."""
    import torch
    from cm3d_amd import _lib
    L = _lib.lib()
    n = [f["cent"].shape[0] for f in frames]
    mask_off = np.concatenate([[0], np.cumsum(n)]).astype(np.int32)
    M = int(mask_off[-1])
    cat = lambda k, dt: np.concatenate([np.asarray(f[k], dt).reshape(-1) for f in frames])
    lane32 = [np.asarray(t, np.float64).astype(np.float32).reshape(-1, 3) for t in tables]
    lane_off = np.concatenate([[0], np.cumsum([t.shape[0] for t in lane32])]).astype(np.int32)
    d = dict(cent=_t(cat("cent", np.float32)), med=_t(np.where(cat("valid", bool), 0, -1).astype(np.int32)), off=_t(mask_off),
             cls=_t(cat("cls", np.int32)), score=_t(cat("score", np.float64)), lane=_t(np.concatenate(lane32)), lane_off=_t(lane_off),
             fl=_t(np.asarray(frame_lane, np.int32)), li=_t(cat("lane_idx", np.int32)), ld=_t(cat("lane_dist", np.float64)),
             prior=_t(classes.prior_wlh, np.float64), veh=_t(classes.is_vehicle, np.int32), grp=_t(classes.nms_group, np.int32),
             thr=_t(classes.nms_thr, np.float64), ego=_t(np.stack([np.asarray(f["ego"], np.float64) for f in frames]).reshape(-1)),
             inv=_t(pose_inv, np.float32) if pose_inv is not None else None)
    box = torch.full((M, _lib.BOX_STRIDE), -7.0, dtype=torch.float64, device=_dev())
    flags = torch.full((M,), -7, dtype=torch.int32, device=_dev())
    _lib.check(L.cm3d_box_nms_bounded(d["cent"].data_ptr(), d["med"].data_ptr(), d["off"].data_ptr(), len(frames), M, d["cls"].data_ptr(),
                                      d["score"].data_ptr(), d["lane"].data_ptr(), d["lane_off"].data_ptr(), d["fl"].data_ptr(), d["li"].data_ptr(),
                                      d["ld"].data_ptr(), d["prior"].data_ptr(), d["veh"].data_ptr(), d["grp"].data_ptr(), d["thr"].data_ptr(),
                                      len(classes.names), d["ego"].data_ptr(), d["inv"].data_ptr() if d["inv"] is not None else 0, bound,
                                      box.data_ptr(), flags.data_ptr(), _st()), "cm3d_box_nms_bounded")
    torch.cuda.synchronize()
    return box.cpu().numpy(), flags.cpu().numpy()


def _nms_frame(n, rng, classes, tie):
    """n boxes of the four classes that are not pushed (translation = centroid, exactly), in a few tight clusters so that most have a
    neighbour of their class within its threshold; about one in six without a medoid; tie: every third score the same value."""
    centres = rng.uniform([560, 1560], [640, 1640], (max(1, n // 12), 2))
    xy = centres[rng.integers(0, centres.shape[0], n)] + rng.normal(scale=0.3, size=(n, 2))
    cls = np.array([classes.index(NMS_CLASSES[i]) for i in rng.integers(0, 4, n)], np.int32)
    score = 0.05 + 0.9 * (rng.permutation(n) + 0.5) / max(n, 1)
    if tie:
        score[::3] = 0.5123456789
    valid = rng.random(n) > 0.16
    return dict(cent=np.concatenate([xy, rng.uniform(-1, 2, (n, 1))], 1).astype(np.float32), cls=cls, score=score.astype(np.float64),
                valid=valid, lane_dist=rng.uniform(0, 30, n), ego=np.array([598.0, 1603.0, 0.5]))


def _expect_unpushed(oracle, f, classes, yaw_table):
    v = f["valid"]
    c64 = f["cent"].astype(np.float64)
    keep = np.zeros(v.size, bool)
    vi = np.flatnonzero(v)
    if vi.size:
        keep[vi] = oracle.circle_nms(c64[vi, 0], c64[vi, 1], f["score"][vi], classes.nms_group[f["cls"][vi]], classes.nms_thr)
    fl = v.astype(np.int32) | (keep.astype(np.int32) << 1)
    yaw = np.asarray(yaw_table, np.float64).astype(np.float32)[f["lane_idx"], 2].astype(np.float64)
    exp = np.zeros((v.size, 10))
    exp[:, 0:3] = np.where(v[:, None], c64, 0.0)
    exp[:, 3] = 1.0
    exp[:, 5] = np.where(v, yaw, 0.0)
    exp[:, 6] = np.where(v, f["lane_dist"], 0.0)
    exp[:, 7], exp[:, 8], exp[:, 9] = f["score"], f["cls"], fl
    return exp, fl


@pytest.mark.parametrize("sizes,bound", [((0, 1, 64, 17, 64), 64), ((0, 1, 64, 65, 33), 65), ((0, 1, 64, 65, 1024), 1024)])
def test_box_nms_bounded_register_and_lds_paths(oracle, sizes, bound):
    """Frames of 0, 1, 64, 65 and CM3D_MAX_MASKS_PER_FRAME masks through cm3d_box_nms_bounded with the bound at 64 (no LDS: every
    frame's NMS on registers), 65 and 1024 (frames of up to 64 masks on registers, longer ones in LDS of the bound's size): groups of
    equal scores (the higher index goes first), masks without a medoid in between.  Every record column and flag is the oracle's."""
    from cm3d_amd.lifting import ClassTable
    classes = ClassTable.nuscenes()
    rng = np.random.default_rng(100 + bound)
    frames = [_nms_frame(n, rng, classes, tie=True) for n in sizes]
    table = np.stack([np.zeros(50), np.zeros(50), rng.uniform(-np.pi, np.pi, 50)], 1)
    for f in frames:
        f["lane_idx"] = rng.integers(0, 50, f["cent"].shape[0])
    box, flags = _box_call_bounded(frames, [table], np.zeros(len(frames), np.int32), classes, bound)
    off = np.concatenate([[0], np.cumsum(sizes)])
    suppressed = 0
    for fi, f in enumerate(frames):
        exp, fl = _expect_unpushed(oracle, f, classes, table)
        assert np.array_equal(flags[off[fi]:off[fi + 1]], fl), (fi, sizes[fi])
        assert np.array_equal(box[off[fi]:off[fi + 1]], exp), (fi, sizes[fi])
        suppressed += int((fl == 1).sum())
    assert suppressed >= 10


def test_box_nms_bounded_frame_above_its_bound(oracle):
    """A frame with more masks than the call's bound: the masks up to the bound as ever, those beyond it (without a medoid, as the
    projection leaves them) get the record of a mask without points."""
    from cm3d_amd.lifting import ClassTable
    classes = ClassTable.nuscenes()
    rng = np.random.default_rng(7)
    frames = [_nms_frame(40, rng, classes, tie=False), _nms_frame(20, rng, classes, tie=True)]
    frames[0]["valid"][32:] = False
    table = np.stack([np.zeros(9), np.zeros(9), rng.uniform(-np.pi, np.pi, 9)], 1)
    for f in frames:
        f["lane_idx"] = rng.integers(0, 9, f["cent"].shape[0])
    box, flags = _box_call_bounded(frames, [table], np.zeros(2, np.int32), classes, 32)
    for f, s in zip(frames, (slice(0, 40), slice(40, 60))):
        exp, fl = _expect_unpushed(oracle, f, classes, table)
        assert np.array_equal(flags[s], fl) and np.array_equal(box[s], exp)


def test_box_nms_bounded_pushed_classes_and_waymo_pose(oracle):
    """Both instances of the kernel on pushed classes, on registers (bound 64) and in LDS (a frame of 90): nuScenes against
    oracle.stage2_frame, Waymo (a pose per frame, centroids in the global frame) against oracle.stage2_frame_waymo -- flags equal,
    translations and rotation / heading within the tight bound of tests.test_gpu_stage2."""
    from cm3d_amd import waymo as wm
    from cm3d_amd.lifting import ClassTable
    rng = np.random.default_rng(9)
    for sizes, bound in (((40, 64, 1), 64), ((40, 90), 90)):
        # ---- nuScenes
        classes = ClassTable.nuscenes()
        frames, tables = [], []
        for n in sizes:
            ego = np.array([600.0, 1600.0, 1.0]) + rng.uniform(-5, 5, 3)
            xy = ego[:2] + rng.uniform(-45, 45, (n, 2))
            lane = np.concatenate([xy + rng.uniform(-0.8, 0.8, (n, 2)), rng.uniform(-np.pi, np.pi, (n, 1))], 1)
            f = dict(cent=np.concatenate([xy, rng.uniform(-1, 2, (n, 1))], 1).astype(np.float32), cls=rng.integers(0, 10, n).astype(np.int32),
                     score=rng.uniform(0.1, 1, n), valid=rng.random(n) > 0.1, ego=ego)
            e = oracle.stage2_frame(f["cent"], np.where(f["valid"], 0, -1), f["cls"], f["score"], lane, ego)
            f["lane_idx"], f["lane_dist"], f["exp"] = np.maximum(e["lane_idx"], 0), np.where(f["valid"], e["lane_dist"], 0.0), e
            frames.append(f); tables.append(lane)
        box, flags = _box_call_bounded(frames, tables, np.arange(len(sizes), dtype=np.int32), classes, bound)
        off = np.concatenate([[0], np.cumsum(sizes)])
        for fi, f in enumerate(frames):
            s, e, v = slice(off[fi], off[fi + 1]), f["exp"], f["valid"]
            assert np.array_equal(flags[s], v.astype(np.int32) | (e["keep"].astype(np.int32) << 1)), (sizes, fi)
            assert np.abs(box[s][v, 0:3] - e["translation"][v]).max(initial=0.0) < BOX_TIGHT
            assert np.abs(box[s][v, 3:5] - e["rotation"][v][:, [0, 3]]).max(initial=0.0) < BOX_TIGHT
        # ---- Waymo
        classes = ClassTable.waymo()
        frames, tables, invs = [], [], []
        for n, (pyaw, tr) in zip(sizes, ((0.3, (1234.5, -2345.25, 10.0)), (-2.9, (-310.75, 4021.0, -3.0)), (1.1, (5.5, 7.25, 0.0)))):
            P = np.eye(4)
            P[:2, :2] = [[np.cos(pyaw), -np.sin(pyaw)], [np.sin(pyaw), np.cos(pyaw)]]
            P[:3, 3] = tr
            rt, inv = wm.pose_records(P.reshape(16))
            cv = np.concatenate([rng.uniform(-40, 40, (n, 2)), rng.uniform(-1, 2, (n, 1))], 1).astype(np.float32)
            cg = np.array([oracle.centroid_transform(c, rt) for c in cv])
            lane = np.concatenate([cg[:, :2].astype(np.float64) + rng.uniform(-0.8, 0.8, (n, 2)), rng.uniform(-np.pi, np.pi, (n, 1))], 1)
            valid = rng.random(n) > 0.1
            cls = rng.integers(0, 10, n).astype(np.int32)
            score = np.float32(rng.uniform(0.1, 1, n)).astype(np.float64)
            e = oracle.stage2_frame_waymo(cv, np.where(valid, 0, -1), cls, score, lane, rt, inv)
            frames.append(dict(cent=cg.astype(np.float32), cls=cls, score=score, valid=valid, lane_idx=np.maximum(e["lane_idx"], 0),
                               lane_dist=np.where(valid, e["lane_dist"], 0.0), ego=np.zeros(3), exp=e))
            tables.append(lane); invs.append(inv)
        box, flags = _box_call_bounded(frames, tables, np.arange(len(sizes), dtype=np.int32), classes, bound, pose_inv=np.stack(invs))
        for fi, f in enumerate(frames):
            s, e, v = slice(off[fi], off[fi + 1]), f["exp"], f["valid"]
            assert np.array_equal(flags[s], v.astype(np.int32) | (e["keep"].astype(np.int32) << 1)), (sizes, fi)
            assert np.abs(box[s][v, 0:3] - e["translation"][v]).max(initial=0.0) < BOX_TIGHT
            assert np.abs(np.angle(np.exp(1j * (box[s][v, 3] - e["heading"][v])))).max(initial=0.0) < BOX_TIGHT
