"""GPU: the rotated-box NMS (cm3d_rotated_nms, cm3d_box_rotated_nms), LiftEngine(nms=...) and the entry points' --nms rotated.
The kernel is held to the host statement cm3d_amd.nms.rotated_nms_host element for element, and -- on the frames whose every
comparable pair is further from its threshold than its float64 error bound (tests/rotated_nms_cases.py) -- to the exact greedy NMS
in rational arithmetic."""
import json
import math
import os
import subprocess
import sys

import numpy as np
import pytest

from cm3d_amd import nms
from tests import rotated_nms_cases as rc

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ------------------------------------------------------------------------------------------------ 1. the stand-alone kernel
@pytest.mark.parametrize("measure", rc.MEASURES)
def test_kernel_equals_host_statement_and_exact_nms(measure):
    from cm3d_amd import ops
    exact = rc.exact_results()
    n_frames, shares, seen = 0, [], set()
    for agn, (cases, rec, score, group, frame_off, thr) in rc.batch(rc.all_cases(), measure).items():
        got = ops.rotated_nms(rec, score, group, frame_off, thr, measure, agn)
        exp = nms.rotated_nms_host(rec, score, group, frame_off, thr, measure, agn)
        assert got.dtype == np.int32 and got.shape == exp.shape
        bad = np.flatnonzero(got != exp)
        assert bad.size == 0, (measure, agn, [cases[int(np.searchsorted(frame_off[1::2], b, "right"))]["name"] for b in bad[:5]])
        assert (np.diff(frame_off)[1::2] == 0).all()                       # an empty frame between every two
        for c, keep in zip(cases, rc.split(cases, frame_off, got)):
            n_frames += 1
            seen.add(c["name"].split(":")[0].split("@")[0].rstrip("0123456789"))
            if c["want"] is not None:
                assert keep.tolist() == c["want"].tolist(), c["name"]
            if c["exact"]:
                assert rc.undecidable_pairs(c["rec"], c["group"], c["thr"], c["agnostic"], (measure,)) == [], c["name"]
                assert np.array_equal(keep, exact[c["name"], measure]), c["name"]
            if c["name"].startswith("crowd") and len(keep) >= 63:
                shares.append(1.0 - keep.mean())
                assert shares[-1] >= 1.0 / 3.0, (c["name"], shares[-1])
            if c["name"] == "beyond_the_frame_limit":
                assert len(keep) == 1030 and keep[1024:].tolist() == [0] * 6 and keep[:1024].sum() > 300
            if c["name"].startswith("degenerate_in_crowd"):
                assert keep[[10, 20, 30, 40, 50]].tolist() == [1] * 5
    print(f"{measure}: {n_frames} frames, suppressed share of the crowds {min(shares):.2f}..{max(shares):.2f}")
    own = {"chain", "thr_of_j_low", "thr_of_j_high"} if measure == "iou" else {"cover_small_inside", "cover_big_under_small"}
    assert own | {"pair", "straddle", "tie", "two_groups", "two_groups_agnostic", "degenerate_in_crowd", "crowd", "beyond_the_frame_limit"} <= seen, seen
    assert sorted({len(c["rec"]) for c in rc.crowd_cases()}) == list(rc.CROWD_SIZES) and len(shares) >= 25


def test_kernel_arguments():
    import torch
    from cm3d_amd import _lib, ops
    L = _lib.lib()
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda()
    rec, sc, grp, off, thr = t(np.zeros((2, 6))), t(np.zeros(2)), t(np.zeros(2, np.int32)), t(np.array([0, 2], np.int32)), t(np.array([0.4]))
    keep = torch.zeros(2, dtype=torch.int32, device="cuda")
    p = [x.data_ptr() for x in (rec, sc, grp, off)]
    st = torch.cuda.current_stream().cuda_stream
    assert L.cm3d_rotated_nms(*p, 1, thr.data_ptr(), 1, 0, 0, keep.data_ptr(), st) == 0
    for k in range(4):
        q = list(p); q[k] = None
        assert L.cm3d_rotated_nms(*q, 1, thr.data_ptr(), 1, 0, 0, keep.data_ptr(), st) == -1
    assert L.cm3d_rotated_nms(*p, 1, None, 1, 0, 0, keep.data_ptr(), st) == -1
    assert L.cm3d_rotated_nms(*p, 1, thr.data_ptr(), 1, 0, 0, None, st) == -1
    for nf, ng, m in ((0, 1, 0), (1, 0, 0), (1, 1, 2), (1, 1, -1)):
        assert L.cm3d_rotated_nms(*p, nf, thr.data_ptr(), ng, m, 0, keep.data_ptr(), st) == -1
    box, fl = t(np.zeros((2, 10))), t(np.zeros(2, np.int32))
    pri, ng_ = t(np.ones((1, 3))), t(np.zeros(1, np.int32))
    args = [box.data_ptr(), fl.data_ptr(), off.data_ptr(), 1, 2, grp.data_ptr(), pri.data_ptr(), ng_.data_ptr(), 1, thr.data_ptr(), 1, 0, 0, 0, 64, st]
    assert L.cm3d_box_rotated_nms(*args) == 0
    for k in (0, 1, 2, 5, 6, 7, 9):
        q = list(args); q[k] = None
        assert L.cm3d_box_rotated_nms(*q) == -1, k
    for k in (3, 4, 8, 10, 14):
        q = list(args); q[k] = 0
        assert L.cm3d_box_rotated_nms(*q) == -1, k
    q = list(args); q[11] = 2
    assert L.cm3d_box_rotated_nms(*q) == -1
    torch.cuda.synchronize()
    with pytest.raises(ValueError):
        ops.rotated_nms(np.zeros((1, 6)), [0.5], [0], [0, 1], 0.4, "giou")
    assert ops.rotated_nms(np.zeros((0, 6)), [], [], [0, 0], 0.4).size == 0


# ------------------------------------------------------------------------------------------------ 2., 3. behind a box launch
FRAME_SIZES = (0, 1, 64, 65, 30)
HEADINGS_AT_PI = (math.pi, -math.pi, np.nextafter(math.pi, 0.0), np.nextafter(-math.pi, 0.0), np.nextafter(math.pi, 4.0),
                  np.nextafter(-math.pi, -4.0), math.pi - 1e-9, -math.pi + 1e-9)


def _box_rows(classes, waymo, thr, seed):
    """Hand-made rows of a box launch for frames of FRAME_SIZES masks: centres around (1600, 1200), more than half of them second
    or third detections of an earlier box of the frame; nuScenes layout: rotation [qw, 0, 0, qz] of a yaw for the pushed classes,
    identity for the others; Waymo layout: a heading, for the first originals the values at +-pi, their second detections either
    side of the seam.  Every sixth mask has no box (flags bit 0 clear, the record of a mask without a medoid); bit 1 and column 9
    start as noise.  Waymo: a row that would put a pair within four times its error bound of a threshold is drawn again (the device's
    cos / sin may differ from numpy's by an ulp, which moves an overlap by no more than the float64 roundings the bound covers)."""
    rng = np.random.default_rng(seed)
    pri, nc = classes.prior_wlh, len(classes.names)
    rows, flags, mask_off = [], [], [0]
    for n in FRAME_SIZES:
        box, recs, grp, free, k = np.zeros((n, 10)), np.zeros((n, 6)), [], [], 0
        side = 6.0 * math.sqrt(n) + 4.0
        while k < n:
            if len(free) and rng.random() < 0.6:
                j = free.pop(int(rng.integers(0, len(free))))
                cls = int(box[j, 8]) if rng.random() < 0.8 else int(rng.integers(0, nc))
                l = pri[cls, 1]
                x, y, yaw, more = box[j, 0] + rng.normal(scale=0.06 * l), box[j, 1] + rng.normal(scale=0.06 * l), box[j, 5] + rng.normal(scale=0.1), []
            else:
                cls = int(rng.integers(0, nc))
                x, y, yaw, more = 1600.0 + rng.uniform(0, side), 1200.0 + rng.uniform(0, side), rng.uniform(-math.pi, math.pi), [k, k]
                if waymo and k < len(HEADINGS_AT_PI):
                    yaw = float(HEADINGS_AT_PI[k])
            if yaw > math.pi or yaw < -math.pi:
                yaw -= math.copysign(2.0 * math.pi, yaw)
            veh = bool(classes.is_vehicle[cls])
            if waymo:
                rot = [yaw if veh else 0.0, 0.0]
            else:
                rot = [math.cos(0.5 * yaw), math.sin(0.5 * yaw)] if veh else [1.0, 0.0]
            box[k] = [x, y, rng.uniform(-1, 2), rot[0], rot[1], yaw, rng.uniform(0, 5), 0.0, cls, 0.0]
            recs[k] = nms.records_from_boxes(box[k], pri, waymo)[0]
            g = int(classes.nms_group[cls])
            if waymo and rc.undecidable_pairs(recs[:k + 1], grp + [g], thr, True, only=[k], factor=4.0):
                continue
            grp.append(g)
            free += more
            k += 1
        box[:, 7] = 0.05 + 0.9 * (rng.permutation(n) + 0.5) / max(n, 1)
        if n >= 30:
            box[rng.integers(0, n, 5), 7] = 0.4321                             # score ties
        fl = np.ones(n, np.int32)
        fl[5::6] = 0
        box[fl == 0, 0:7] = [0.0, 0.0, 0.0, 0.0 if waymo else 1.0, 0.0, 0.0, 0.0]
        rows.append(box)
        flags.append(fl | (rng.integers(0, 2, n).astype(np.int32) << 1))
        mask_off.append(mask_off[-1] + n)
    box = np.concatenate(rows)
    flags = np.concatenate(flags)
    box[:, 9] = rng.uniform(-3, 3, len(box))
    return box, flags, np.array(mask_off, np.int32)


def _box_call(box, flags, mask_off, classes, thr, measure, agn, waymo, cap):
    import torch
    from cm3d_amd import _lib
    L = _lib.lib()
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda()
    d_box, d_fl, d_off = t(box), t(flags), t(mask_off)
    d_cls, d_pri, d_grp, d_thr = t(box[:, 8].astype(np.int32)), t(classes.prior_wlh), t(np.asarray(classes.nms_group, np.int32)), t(np.asarray(thr, np.float64))
    rc_ = L.cm3d_box_rotated_nms(d_box.data_ptr(), d_fl.data_ptr(), d_off.data_ptr(), len(mask_off) - 1, len(box), d_cls.data_ptr(), d_pri.data_ptr(),
                                 d_grp.data_ptr(), len(classes.names), d_thr.data_ptr(), len(thr), nms.measure_code(measure), int(agn), int(waymo),
                                 cap, torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    assert rc_ == 0
    return d_box.cpu().numpy(), d_fl.cpu().numpy()


def _take(flags, mask_off, cap):
    within = np.concatenate([np.arange(b - a) for a, b in zip(mask_off[:-1], mask_off[1:])]) if len(flags) else np.zeros(0, int)
    return ((flags & 1) == 1) & (within < cap)


@pytest.mark.parametrize("measure,agn,cap", [("iou", False, 64), ("cover", True, 64), ("iou", True, 1024), ("cover", False, 1024)])
def test_box_rows_nuscenes_layout(measure, agn, cap):
    from cm3d_amd.lifting import ClassTable
    classes = ClassTable.nuscenes()
    thr = nms.RotatedNms(thr={"car": 0.3, "pedestrian": 0.2, "bus": 0.5}).thr_by_group(classes)
    box, flags, mask_off = _box_rows(classes, False, thr, 11)
    veh = classes.is_vehicle[box[:, 8].astype(int)].astype(bool) & ((flags & 1) == 1)
    assert veh.sum() > 30 and (~veh & ((flags & 1) == 1)).sum() > 30 and (box[veh, 4] != 0).all() and ((flags & 1) == 0).sum() > 20
    got_box, got_fl = _box_call(box, flags, mask_off, classes, thr, measure, agn, False, cap)
    take = _take(flags, mask_off, cap)
    keep = nms.rotated_nms_host(nms.records_from_boxes(box, classes.prior_wlh, False), box[:, 7], classes.nms_group[box[:, 8].astype(int)],
                                mask_off, thr, measure, agn, take=take)
    assert np.array_equal(got_fl, (flags & 1) | (keep << 1))
    assert np.array_equal(got_box[:, 9], got_fl.astype(np.float64))
    assert got_box[:, :9].tobytes() == box[:, :9].tobytes()                  # every other byte is what it was
    assert (got_fl[(flags & 1) == 0] == 0).all()                              # no box: takes no part, bit 1 clear
    sup = take & (keep == 0)
    assert sup.sum() >= take.sum() / 5, (sup.sum(), take.sum())
    m64 = mask_off[3] + 64                                                    # the 65th mask of the frame of 65
    assert (got_fl[m64] == (flags[m64] & 1)) if cap == 64 else take[m64]
    if agn:                                                                   # a pair of different classes went
        cls = box[:, 8].astype(int)
        other = nms.rotated_nms_host(nms.records_from_boxes(box, classes.prior_wlh, False), box[:, 7], classes.nms_group[cls], mask_off, thr,
                                     measure, False, take=take)
        assert (keep < other).any()


@pytest.mark.parametrize("measure,agn", [("iou", False), ("cover", True)])
def test_box_rows_waymo_layout(measure, agn):
    from cm3d_amd.lifting import ClassTable
    classes = ClassTable.waymo()
    thr = nms.RotatedNms(thr={"car": 0.3, "pedestrian": 0.2}).thr_by_group(classes)
    box, flags, mask_off = _box_rows(classes, True, thr, 12)
    h = box[(flags & 1) == 1, 3]
    assert (h > 3.1).sum() >= 3 and (h < -3.1).sum() >= 3
    got_box, got_fl = _box_call(box, flags, mask_off, classes, thr, measure, agn, True, 1024)
    assert got_box[:, :9].tobytes() == box[:, :9].tobytes() and np.array_equal(got_box[:, 9], got_fl.astype(np.float64))
    rec = nms.records_from_boxes(box, classes.prior_wlh, True)                # c, s = numpy's cos, sin of the stored heading
    grp = classes.nms_group[box[:, 8].astype(int)]
    n_sup = 0
    for f in range(len(mask_off) - 1):
        a, b = int(mask_off[f]), int(mask_off[f + 1])
        take = (flags[a:b] & 1) == 1
        idx = np.flatnonzero(take)
        assert rc.undecidable_pairs(rec[a:b][idx], grp[a:b][idx], thr, agn, (measure,), factor=4.0) == []
        keep = rc.exact_nms(rec[a:b], box[a:b, 7], grp[a:b], thr, measure, agn, take=take)
        assert np.array_equal(got_fl[a:b], (flags[a:b] & 1) | (keep << 1)), f
        n_sup += int((take & (keep == 0)).sum())
    assert n_sup >= 20


# ------------------------------------------------------------------------------------------------ 4. the engine
def _run(eng, hb):
    import torch
    eng.upload(hb)
    eng.run(masks="rle")
    torch.cuda.synchronize()
    return eng.download(full=True)


@pytest.fixture(scope="module")
def batch():
    """Four tiny frames (one without a point); in each, the masks with the most points get a second detection (half the mask) of
    the same class and a third (the whole mask again) of another class, so that boxes overlap; the plain pass over them."""
    from cm3d_amd import lifting, synthetic as syn
    from tests.test_gpu_drivable import _half_mask
    frames = [syn.make_frame(syn.config("tiny", n_masks=12, seed=5200 + i), i) for i in range(4)]
    frames[2].sweeps_raw = [frames[2].sweeps_raw[0][:0]]
    frames[2].sweep_xf = frames[2].sweep_xf[:1]
    lanes = [syn.make_lane_table(frames[0].ego_xyz[:2], 1500, seed=2)]
    hb = lifting.pack_frames(frames, lanes, [0] * 4)
    first = _run(lifting.LiftEngine("cuda:0"), hb)
    names = lifting.ClassTable.nuscenes().names
    for f, fr in enumerate(frames):
        m0, n = int(hb.mask_off[f]), len(fr.rles)
        top = [int(k) for k in np.argsort(-np.diff(first["hit_off"])[m0:m0 + n], kind="stable")[:5]]
        for r, k in enumerate(top):
            other = names[(names.index(lifting.get_detection_name(fr.labels[k])) + 1 + r) % len(names)]
            for rle, label, score in ((_half_mask(fr.rles[k]), fr.labels[k], 0.95 - 0.01 * r), (fr.rles[k], other, 0.90 - 0.01 * r)):
                fr.rles.append(rle); fr.labels.append(label); fr.scores.append(score); fr.cam_nums.append(fr.cam_nums[k])
    hb = lifting.pack_frames(frames, lanes, [0] * 4)
    return frames, lanes, hb, _run(lifting.LiftEngine("cuda:0"), hb)


def _check_engine_result(B, A, hb, classes, r):
    """B: the pass with the rotated NMS, A: the same pass without.  Everything but the NMS decision is A's; the decision is the host's."""
    for key in A:
        if key not in ("box", "flags"):
            assert B[key].tobytes() == A[key].tobytes(), key
    assert B["box"][:, :9].tobytes() == A["box"][:, :9].tobytes() and np.array_equal(B["flags"] & 1, A["flags"] & 1)
    assert np.array_equal(B["box"][:, 9], B["flags"].astype(np.float64)) and set(np.unique(B["flags"])) <= {0, 1, 3}
    cls = B["box"][:, 8].astype(int)
    assert np.array_equal(cls, hb.class_id)
    keep = nms.rotated_nms_host(nms.records_from_boxes(B["box"], classes.prior_wlh, False), B["box"][:, 7], classes.nms_group[cls], hb.mask_off,
                                r.thr_by_group(classes), r.measure, r.class_agnostic, take=(B["flags"] & 1) == 1)
    assert np.array_equal(B["flags"] >> 1, keep)
    return keep


@pytest.mark.parametrize("kw", [dict(class_agnostic=True), dict(measure="cover", thr={"car": 0.3, "pedestrian": 0.6}, class_agnostic=True)],
                         ids=["iou", "cover"])
def test_engine(batch, kw):
    import torch
    from cm3d_amd import lifting
    frames, lanes, hb, A = batch
    classes = lifting.ClassTable.nuscenes()
    r = lifting.RotatedNms(**kw)
    eng = lifting.LiftEngine("cuda:0", nms=r)
    marks = []
    eng.upload(hb)
    eng.run(masks="rle", stage_events=marks)
    torch.cuda.synchronize()
    B = eng.download(full=True)
    assert len(marks) == 5 and set(B) == set(A)
    keep = _check_engine_result(B, A, hb, classes, r)
    has = (A["flags"] & 1) == 1
    assert has.sum() >= 30 and (keep[has] == 0).sum() >= 5
    differs = [f for f in range(hb.n_frames) if not np.array_equal(B["flags"][hb.mask_off[f]:hb.mask_off[f + 1]], A["flags"][hb.mask_off[f]:hb.mask_off[f + 1]])]
    assert differs, "the kept set equals the circle NMS's in every frame"
    m2 = slice(int(hb.mask_off[2]), int(hb.mask_off[3]))
    assert (B["flags"][m2] == 0).all()                                         # the frame without points
    # a second pass, then a graph replay
    eng.b.flags.fill_(-3); eng.b.box[:, 9] = -3.0
    eng.run(masks="rle")
    torch.cuda.synchronize()
    again = eng.download(full=True)
    assert all(again[k].tobytes() == B[k].tobytes() for k in B)
    g = eng.capture_graph(masks="rle")
    eng.b.flags.fill_(-3); eng.b.box[:, 9] = -3.0
    g.replay()
    torch.cuda.synchronize()
    rep = eng.download(full=True)
    assert all(rep[k].tobytes() == B[k].tobytes() for k in B)
    if r.measure == "cover":                                                   # the same batch through a pipeline slot (rerun takes its Python branch)
        pipe = lifting.LiftPipeline("cuda:0", depth=2, nms=r)
        slot = pipe.submit(hb, "rle")
        pipe.rerun(slot)
        _, res = pipe.collect(slot)
        assert all(res[k].tobytes() == B[k].tobytes() for k in B)
        off = lifting.LiftEngine("cuda:0", nms=None)                           # no NMS asked for: the plain pass, no threshold table
        C = _run(off, hb)
        assert off.nms is None and off.rot_thr is None and all(C[k].tobytes() == A[k].tobytes() for k in A)


def test_engine_with_filters_and_clustering(batch):
    from cm3d_amd import lifting
    frames, lanes, hb, A = batch
    classes = lifting.ClassTable.nuscenes()
    has = A["medoid_pos"] >= 0
    f = lifting.Stage2Filters(lane_max_dist=float(np.quantile(A["lane_dist"][has], 0.8)))
    c = lifting.DepthCluster(0.6, 6)
    r = lifting.RotatedNms(class_agnostic=True)
    for kw in (dict(filters=f), dict(cluster=c), dict(filters=f, cluster=c)):
        base = _run(lifting.LiftEngine("cuda:0", **kw), hb)
        both = _run(lifting.LiftEngine("cuda:0", nms=r, **kw), hb)
        keep = _check_engine_result(both, base, hb, classes, r)
        took = (base["flags"] & 1) == 1
        assert took.sum() >= 20 and (keep[took] == 0).sum() >= 3 and not np.array_equal(both["flags"], base["flags"]), list(kw)
        if "filters" in kw:
            assert (took < has).any()                                          # the filter dropped a box, which then took no part


# ------------------------------------------------------------------------------------------------ 5. the entry points
def test_nuscenes_entry_point(tmp_path):
    """src/nuscenes/2d_to_3d.py --nms rotated --nms-class-agnostic, both host routes: the file holds the boxes an engine with that NMS
    keeps, in the writer's order; with --nms circle (the other flags are then not read) the bytes are those of a run without any of
    the flags, made at the start of the test."""
    from cm3d_amd import lifting, nusc_io
    from tests.test_gpu_drivable import _nusc_dataset
    cfg, dataroot, mask_dir, names = _nusc_dataset(tmp_path)
    env = dict(os.environ, CM3D_VER_NAME="v1.0-synth", CM3D_INPUT_PATH=dataroot, CM3D_INPUT_DIR=mask_dir)
    flags = ["--nms", "rotated", "--nms-class-agnostic", "--nms-thr", "0.05"]
    blobs = {}
    for route, extra in (("plain", []), ("native", flags), ("python", flags + ["--reader-threads", "-1"]),
                         ("circle", ["--nms", "circle", "--nms-overlap", "cover", "--nms-class-agnostic"])):
        p = subprocess.run([sys.executable, "2d_to_3d.py", "--ratio", str(cfg.ratio)] + extra, cwd=os.path.join(ROOT, "src", "nuscenes"),
                           env=dict(env, CM3D_OUTPUT_DIR=str(tmp_path / route)), capture_output=True, text=True, timeout=600)
        assert p.returncode == 0, p.stderr[-2000:]
        blobs[route] = open(tmp_path / route / "pseudolabels_minival.json", "rb").read()
    assert blobs["circle"] == blobs["plain"]
    assert json.loads(blobs["native"]) == json.loads(blobs["python"])
    tables = nusc_io.NuscTables("v1.0-synth", dataroot)
    classes = lifting.ClassTable.nuscenes()
    r = lifting.RotatedNms("iou", 0.05, True)
    eng, plain = lifting.LiftEngine("cuda:0", nms=r), lifting.LiftEngine("cuda:0")
    want, n_changed = {}, 0
    for name in names:
        scene = tables.scene_by_name(name)
        frames = nusc_io.frames_of_scene(tables, scene, mask_dir, n_sweeps=3, ratio=cfg.ratio)
        lanes = [nusc_io.load_lane_points(dataroot, tables.location(scene))]
        hb = lifting.pack_frames(frames, lanes, [0] * len(frames))
        res, base = _run(eng, hb), _run(plain, hb)
        _check_engine_result(res, base, hb, classes, r)
        want.update(lifting.box_records(hb, res, classes))
        n_changed += int((res["flags"] != base["flags"]).sum())
    got = json.loads(blobs["native"])["results"]
    assert got == want and [list(map(json.dumps, got[k])) for k in got] == [list(map(json.dumps, want[k])) for k in want]
    assert sum(map(len, want.values())) > 5
    assert n_changed >= 1 and blobs["native"] != blobs["plain"]               # the flag changes the file
    print(f"nuScenes entry point: {n_changed} masks decided differently from the circle NMS")


def test_waymo_entry_point(tmp_path):
    """src/waymo/2d_to_3d.py --nms rotated: the file is the one an engine with that NMS gives; without the flag the bytes are those of
    the run at the start of the test."""
    from tests.test_gpu_entrypoint import _write_waymo_scene
    from cm3d_amd import lifting, pipeline_waymo as pw, waymo as wm
    scene = "segment-synthetic-0"
    _write_waymo_scene(tmp_path, scene, 0, 4)
    cwd = os.path.join(ROOT, "src", "waymo")
    args = ["--frames-dir", str(tmp_path / "frames"), "--mask-dir", str(tmp_path / "masks")]
    blobs = {}
    for key, extra in (("plain", []), ("rotated", ["--nms", "rotated", "--nms-overlap", "cover", "--nms-thr", "0.05", "--nms-class-agnostic"]),
                       ("circle", ["--nms", "circle", "--nms-thr", "0.05"])):
        p = subprocess.run([sys.executable, "2d_to_3d.py", *args, "--output", str(tmp_path / f"{key}.bin"), *extra], cwd=cwd,
                           capture_output=True, text=True, timeout=600)
        assert p.returncode == 0, p.stderr[-2000:]
        blobs[key] = open(tmp_path / f"{key}.bin", "rb").read()
    assert blobs["circle"] == blobs["plain"]
    frames, lanes = pw.load_scene(str(tmp_path / "frames"), str(tmp_path / "masks"), scene)
    classes = lifting.ClassTable.waymo()
    hb = lifting.pack_frames(frames, [lanes], [0] * len(frames), classes)
    r = lifting.RotatedNms("cover", 0.05, True)
    got = _run(lifting.LiftEngine("cuda:0", classes=classes, nms=r), hb)
    base = _run(lifting.LiftEngine("cuda:0", classes=classes), hb)
    assert got["box"][:, :9].tobytes() == base["box"][:, :9].tobytes() and np.array_equal(got["flags"] & 1, base["flags"] & 1)
    objs = wm.objects_from_results(hb, got, classes, [(f.context_name, f.timestamp_micros) for f in frames])
    assert blobs["rotated"] == wm.encode_objects(objs) and len(objs) >= 2
    print(f"Waymo entry point: {int((got['flags'] != base['flags']).sum())} masks decided differently from the circle NMS")
