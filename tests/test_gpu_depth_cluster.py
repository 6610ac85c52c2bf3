"""GPU: the depth clustering of the in-mask lists (cm3d_depth_cluster) and the clustered pass (cm3d_lift_pass_clustered).  Every
expectation is the host statement cm3d_amd.cluster.depth_cluster_host (held against the O(n^2) connected components by
tests/test_depth_cluster_host.py), and every comparison is exact: offsets, statuses, index entries, and the coordinates to the bit."""
import json
import os
import pickle
import subprocess
import sys

import numpy as np
import pytest

from cm3d_amd import cluster
from tests import depth_cluster_cases as cases

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TILE = 64


def _expected(lists, frames, eps, mp, pick, hit_idx):
    """cl_off, cl_tile_off, cl_status, cl_idx, cl_xyz of lists laid out back to back (xyz (n, 4) float32 each)."""
    keeps, status = [], []
    for p, f in zip(lists, frames):
        k, s = cluster.depth_cluster_host(p[:, :3], cases.ORIGINS[f], eps, mp, pick)
        keeps.append(k)
        status.append(s)
    cnt = np.array([int(k.sum()) for k in keeps], np.int64)
    keep = np.concatenate(keeps) if keeps else np.zeros(0, bool)
    allp = np.concatenate(lists, 0)
    return dict(cl_off=np.concatenate([[0], np.cumsum(cnt)]).astype(np.int32),
                cl_tile_off=np.concatenate([[0], np.cumsum((cnt + TILE - 1) // TILE)]).astype(np.int32),
                cl_status=np.array(status, np.int32), cl_idx=None if hit_idx is None else hit_idx[keep], cl_xyz=allp[keep])


def _check(got, exp, what=""):
    for key in ("cl_off", "cl_tile_off", "cl_status"):
        assert got[key].dtype == np.int32 and np.array_equal(got[key], exp[key]), (what, key)
    assert got["cl_xyz"].shape == exp["cl_xyz"].shape and np.array_equal(got["cl_xyz"].view(np.uint32), exp["cl_xyz"].view(np.uint32)), what
    if exp["cl_idx"] is None:
        assert got["cl_idx"] is None
    else:
        assert np.array_equal(got["cl_idx"], exp["cl_idx"]), what


def _with_w(xyz, rng):
    """(n, 4): the fourth column (the intensity) travels with the point."""
    return np.concatenate([np.asarray(xyz, np.float32).reshape(-1, 3), rng.uniform(0, 255, (len(xyz), 1)).astype(np.float32)], 1)


@pytest.fixture(scope="module")
def many_lists():
    """The lists of the one-call test: every length at which the kernel takes another turn (a wave, a workgroup's stride, the LDS limit
    L and beyond it), empty lists between them, the hand-written rows, over three frames with different origins."""
    from cm3d_amd import _lib
    L = _lib.DEPTH_CLUSTER_LDS_POINTS
    rng = np.random.default_rng(2024)
    lists, frames = [], []
    for k, n in enumerate([0, 1, 19, 20, 21, 63, 64, 65, 255, 256, 257, L - 1, L, L + 1, 3 * L + 5]):
        f = k % 3
        p = cases.random_list(rng, cases.ORIGINS[f], n=n, centres=1 + k % 4)
        if n >= 63:                                  # equal ranges: the position decides the sorted order
            dup = rng.integers(0, n, n // 8)
            p[rng.integers(0, n, n // 8)] = p[dup]
        lists.append(_with_w(p, rng))
        frames.append(f)
        if k % 2:
            lists.append(np.zeros((0, 4), np.float32))
            frames.append((f + 1) % 3)
    for name, (xyz, o, _, _, _) in cases.crafted().items():
        lists.append(_with_w(xyz, rng))
        frames.append(o)
    lists.append(np.zeros((0, 4), np.float32))
    frames.append(2)
    total = sum(len(p) for p in lists)
    hit_idx = rng.integers(0, 1 << 30, total).astype(np.int32)
    return lists, np.array(frames, np.int32), hit_idx


@pytest.mark.parametrize("pick,with_idx", [("largest", True), ("nearest", True), ("largest", False)])
def test_one_call_over_many_lists(many_lists, pick, with_idx):
    from cm3d_amd import ops
    lists, frames, hit_idx = many_lists
    assert {0, 1, 2} == set(frames.tolist()) and np.abs(np.concatenate(lists)[:, 1]).max() > 1600
    got = ops.depth_cluster_arrays(lists, cases.ORIGINS, frames, cases.EPS, cases.MIN_POINTS, pick, hit_idx=hit_idx, with_idx=with_idx)
    exp = _expected(lists, frames, cases.EPS, cases.MIN_POINTS, pick, hit_idx if with_idx else None)
    _check(got, exp, pick)
    st = exp["cl_status"]
    assert (st == 0).sum() >= 10 and (st == 1).sum() >= 5 and (st == 2).sum() >= 8
    n = np.array([len(p) for p in lists])
    assert (np.diff(exp["cl_off"])[(st == 0) & (n > 4000)] < n[(st == 0) & (n > 4000)]).any()       # a long list loses points


@pytest.mark.parametrize("pick", cluster.PICKS)
def test_crafted_rows_at_their_own_parameters(pick):
    """The hand-written rows again, each group of rows with the eps and min_points it was written for (one call per group)."""
    from cm3d_amd import ops
    rows = cases.crafted()
    groups = {}
    for name, (xyz, o, eps, mp, want) in rows.items():
        groups.setdefault((eps, mp), []).append(name)
    for (eps, mp), names in groups.items():
        lists = [np.concatenate([rows[n][0], np.zeros((len(rows[n][0]), 1), np.float32)], 1) for n in names]
        frames = np.array([rows[n][1] for n in names], np.int32)
        got = ops.depth_cluster_arrays(lists, cases.ORIGINS, frames, eps, mp, pick)
        _check(got, _expected(lists, frames, eps, mp, pick, np.concatenate([np.arange(len(p), dtype=np.int32) for p in lists])), names)
        for k, n in enumerate(names):
            want = rows[n][4]
            if want is not None and pick in want:
                assert (got["cl_idx"][got["cl_off"][k]:got["cl_off"][k + 1]].tolist(), int(got["cl_status"][k])) == want[pick], n
    kept, status = ops.depth_cluster([rows["min_points_one"][0]], [0.0, 0.0, 0.0], 1.0, 1, pick)
    assert kept[0].tolist() == rows["min_points_one"][4][pick][0] and status.tolist() == [0]


@pytest.mark.parametrize("pick", cluster.PICKS)
def test_random_lists(pick):
    from cm3d_amd import ops
    rl = cases.random_lists(77, 300)
    rng = np.random.default_rng(5)
    lists, frames = [_with_w(p, rng) for p, _ in rl], np.array([o for _, o in rl], np.int32)
    hit_idx = np.arange(sum(len(p) for p in lists), dtype=np.int32)[::-1].copy()
    got = ops.depth_cluster_arrays(lists, cases.ORIGINS, frames, cases.EPS, cases.MIN_POINTS, pick, hit_idx=hit_idx)
    exp = _expected(lists, frames, cases.EPS, cases.MIN_POINTS, pick, hit_idx)
    n, kept, st = np.array([len(p) for p in lists]), np.diff(exp["cl_off"]), exp["cl_status"]
    subset, whole = ((st == 0) & (kept < n)).mean(), (st == 1).mean()
    print(f"{pick}: strict subsets {subset:.2f}, kept whole {whole:.2f}")
    assert subset >= 0.25 and whole >= 0.10                  # otherwise the lists show nothing
    _check(got, exp, pick)


@pytest.mark.parametrize("hit_off", [[0, 100, 250, 700, 900, 901], [-5, 40, 30, 2147483647, 7, 299], [300, 300, 300, 300, 300, 2000]],
                         ids=["beyond", "garbage", "at_cap"])
def test_offsets_that_claim_more_than_exists(hit_off):
    """After a capacity overflow hit_off describes more than idx_cap positions: the call answers with a code, clamps every offset, and
    writes nothing behind idx_cap entries of its outputs nor behind its workspace (guard words there are intact)."""
    import torch
    from cm3d_amd import _lib
    L = _lib.lib()
    cap, guard, M = 300, 4096, len(hit_off) - 1
    dev = torch.device("cuda:0")
    rng = np.random.default_rng(1)
    pts = np.concatenate([cases.random_list(rng, cases.ORIGINS[0], n=cap + guard, centres=3), np.zeros((cap + guard, 1), np.float32)], 1)
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)
    d_xyz, d_idx, d_off = t(pts), t(np.arange(cap + guard, dtype=np.int32)), t(np.array(hit_off, np.int32))
    d_mf, d_org = t(np.zeros(M, np.int32)), t(cases.ORIGINS[:1])
    cl_xyz = torch.full((cap + guard, 4), -7.0, dtype=torch.float32, device=dev)
    cl_idx = torch.full((cap + guard,), -7, dtype=torch.int32, device=dev)
    cl_off = torch.full((M + 1 + guard,), -7, dtype=torch.int32, device=dev)
    cl_tile = torch.full((M + 1 + guard,), -7, dtype=torch.int32, device=dev)
    cl_st = torch.full((M + guard,), -7, dtype=torch.int32, device=dev)
    ws_bytes = int(L.cm3d_depth_cluster_workspace_bytes(M, cap))
    ws = torch.full((ws_bytes + guard,), 0x5A, dtype=torch.uint8, device=dev)
    rc = L.cm3d_depth_cluster(d_xyz.data_ptr(), d_idx.data_ptr(), d_off.data_ptr(), d_mf.data_ptr(), M, cap, d_org.data_ptr(), 1, 1.0, 20, 0,
                              cl_off.data_ptr(), cl_tile.data_ptr(), cl_idx.data_ptr(), cl_xyz.data_ptr(), cl_st.data_ptr(), ws.data_ptr(),
                              ws_bytes, torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    assert rc == 0
    assert (cl_xyz[cap:] == -7.0).all() and (cl_idx[cap:] == -7).all() and (ws[ws_bytes:] == 0x5A).all()
    assert (cl_off[M + 1:] == -7).all() and (cl_tile[M + 1:] == -7).all() and (cl_st[M:] == -7).all()
    off, st = cl_off[:M + 1].cpu().numpy(), cl_st[:M].cpu().numpy()
    assert off[0] == 0 and (np.diff(off) >= 0).all() and set(st.tolist()) <= {0, 1, 2}
    lo = np.clip(np.array(hit_off[:-1], np.int64), 0, cap)
    hi = np.maximum(np.clip(np.array(hit_off[1:], np.int64), 0, cap), lo)
    assert np.array_equal(st == 2, hi == lo) and (np.diff(off) <= hi - lo).all()
    if (np.diff(np.concatenate([lo[:1], hi])) >= 0).all() and (lo[1:] >= hi[:-1]).all():       # the clamped lists are disjoint: each is the statement's
        lists = [pts[a:b] for a, b in zip(lo, hi)]
        exp = _expected(lists, [0] * M, 1.0, 20, "largest", np.concatenate([np.arange(a, b, dtype=np.int32) for a, b in zip(lo, hi)]))
        k = int(off[-1])
        _check(dict(cl_off=off, cl_tile_off=cl_tile[:M + 1].cpu().numpy(), cl_status=st, cl_idx=cl_idx[:k].cpu().numpy(),
                    cl_xyz=cl_xyz[:k].cpu().numpy()), exp, "clamped")


# ------------------------------------------------------------------------------------------------ the clustered pass
PASS_EPS, PASS_MIN = 0.6, 6        # the tiny synthetic frames' lists are short: values at which both outcomes occur (asserted below)


def _run(eng, hb, marks=None):
    import torch
    eng.upload(hb)
    eng.run(masks="rle", stage_events=marks)
    torch.cuda.synchronize()
    return eng.download(full=True)


@pytest.fixture(scope="module")
def batch():
    """Four tiny frames, the third without a point; engine A's plain pass over them."""
    from cm3d_amd import lifting, synthetic as syn
    frames = [syn.make_frame(syn.config("tiny", seed=4100 + i), i) for i in range(4)]
    frames[2].sweeps_raw = [frames[2].sweeps_raw[0][:0]]
    frames[2].sweep_xf = frames[2].sweep_xf[:1]
    lanes = [syn.make_lane_table(frames[0].ego_xyz[:2], 1500, seed=2)]
    hb = lifting.pack_frames(frames, lanes, [0] * 4)
    return frames, lanes, hb, _run(lifting.LiftEngine("cuda:0"), hb)


def _host_clustered(hb, A, c):
    cl_off, cl_tile_off, keep, status = cluster.cluster_lists(A["hit_off"], A["hit_xyz"], hb.mask_frame, hb.ego_xyz, c.eps, c.min_points, c.pick)
    return dict(cl_off=cl_off, cl_tile_off=cl_tile_off, cl_status=status, cl_idx=A["hit_idx"][keep], cl_xyz=A["hit_xyz"][keep])


@pytest.mark.parametrize("pick", cluster.PICKS)
def test_clustered_pass(oracle, batch, pick):
    import torch
    from cm3d_amd import lifting, ops
    frames, lanes, hb, A = batch
    c = lifting.DepthCluster(PASS_EPS, PASS_MIN, pick)
    eng = lifting.LiftEngine("cuda:0", cluster=c)
    marks = []
    B = _run(eng, hb, marks)
    assert len(marks) == 7 and marks[5].elapsed_time(marks[6]) >= 0.0 and marks[1].elapsed_time(marks[5]) >= 0.0
    for key in ("hit_off", "hit_idx", "hit_xyz", "pt_off", "bbox"):                  # the raw lists stay the raw lists
        assert B[key].tobytes() == A[key].tobytes(), key
    exp = _host_clustered(hb, A, c)
    got = dict(B, cl_tile_off=eng.b.cl_tile_off.cpu().numpy())
    _check(got, exp, pick)
    n, kept, st = np.diff(A["hit_off"]), np.diff(exp["cl_off"]), exp["cl_status"]
    assert ((st == 0) & (kept < n)).sum() >= 3 and (st == 1).sum() >= 3 and (st == 2).sum() >= 3
    m2 = slice(int(hb.mask_off[2]), int(hb.mask_off[3]))
    assert (st[m2] == 2).all() and (B["flags"][m2] == 0).all()                      # the frame without points
    # the medoid of the clustered lists
    off = exp["cl_off"]
    lists = [exp["cl_xyz"][off[m]:off[m + 1], :3] for m in range(hb.n_masks)]
    med = np.array([oracle.medoid(exp["cl_xyz"], np.arange(off[m], off[m + 1], dtype=np.int32)) for m in range(hb.n_masks)], np.int32)      # (-1: empty)
    assert np.array_equal(B["medoid_pos"], med)
    assert np.array_equal(np.array(ops.get_medoids(lists), np.int32), med)           # the stand-alone call agrees
    cen = np.array([lists[m][med[m]] if med[m] >= 0 else np.zeros(3, np.float32) for m in range(hb.n_masks)], np.float32)
    assert B["centroid"].tobytes() == cen.tobytes()
    assert (B["medoid_pos"] >= 0).tolist() == (A["medoid_pos"] >= 0).tolist()       # the set of masks with a box does not change
    assert not np.array_equal(B["centroid"], A["centroid"])                          # ... and the clustering moved a medoid
    small = eng.download(full=False)
    assert np.array_equal(small["cl_off"], exp["cl_off"]) and np.array_equal(small["cl_status"], st) and "cl_idx" not in small
    # a second pass, then a graph replay
    for name in ("cl_off", "cl_idx", "cl_status", "medoid_pos", "flags"):
        getattr(eng.b, name).fill_(-3)
    eng.run(masks="rle")
    torch.cuda.synchronize()
    again = eng.download(full=True)
    assert all(again[k].tobytes() == B[k].tobytes() for k in B)
    g = eng.capture_graph(masks="rle")
    for name in ("cl_off", "cl_idx", "cl_status", "medoid_pos", "flags"):
        getattr(eng.b, name).fill_(-3)
    eng.b.cl_xyz.fill_(0.0)
    g.replay()
    torch.cuda.synchronize()
    rep = eng.download(full=True)
    assert all(rep[k].tobytes() == B[k].tobytes() for k in B)
    if pick == "largest":                            # the same batch through a pipeline slot (rerun takes its Python branch)
        pipe = lifting.LiftPipeline("cuda:0", depth=2, cluster=c)
        slot = pipe.submit(hb, "rle")
        pipe.rerun(slot)
        _, res = pipe.collect(slot)
        assert all(res[k].tobytes() == B[k].tobytes() for k in B)


@pytest.mark.parametrize("kw", [dict(eps=float("inf"), min_points=1), dict(eps=1.0, min_points=10 ** 6)], ids=["one_cluster", "none_qualifies"])
def test_clustering_that_keeps_every_list_whole_is_the_plain_pass(batch, kw):
    from cm3d_amd import lifting
    frames, lanes, hb, A = batch
    eng = lifting.LiftEngine("cuda:0", cluster=lifting.DepthCluster(**kw))
    B = _run(eng, hb)
    for key in ("box", "flags", "centroid", "lane_idx", "lane_dist", "medoid_pos", "hit_off", "hit_idx", "hit_xyz"):
        assert B[key].dtype == A[key].dtype and B[key].tobytes() == A[key].tobytes(), key
    assert np.array_equal(B["cl_off"], A["hit_off"]) and np.array_equal(B["cl_idx"], A["hit_idx"]) and B["cl_xyz"].tobytes() == A["hit_xyz"].tobytes()
    want = 0 if kw["min_points"] == 1 else 1
    assert np.array_equal(B["cl_status"], np.where(np.diff(A["hit_off"]) > 0, want, 2))
    # no clustering asked for: no buffer, no result key
    off = lifting.LiftEngine("cuda:0", cluster=None)
    C = _run(off, hb)
    assert off.cluster is None and not hasattr(off.b, "cl_off") and set(C) == set(A)


def test_filters_and_clustering_together(batch):
    from cm3d_amd import drivable, lifting
    frames, lanes, hb, A = batch
    has = A["medoid_pos"] >= 0
    thr = float(np.median(A["lane_dist"][has]))
    f = lifting.Stage2Filters(lane_max_dist=thr, vehicle_lane_max_dist=0.75 * thr)
    c = lifting.DepthCluster(PASS_EPS, PASS_MIN)
    marks = []
    both = _run(lifting.LiftEngine("cuda:0", filters=f, cluster=c), hb, marks)
    only = _run(lifting.LiftEngine("cuda:0", cluster=c), hb)
    assert len(marks) == 9
    for key in ("cl_off", "cl_idx", "cl_status", "medoid_pos", "centroid", "lane_idx", "lane_dist"):
        assert both[key].tobytes() == only[key].tobytes(), key
    cls = lifting.ClassTable.nuscenes()
    kept = drivable.filter_rule(both["medoid_pos"], hb.class_id, both["lane_dist"], None, cls.is_vehicle, cls.needs_road, thr, 0.75 * thr)
    assert np.array_equal(both["medoid_pos_kept"], kept)
    dropped = (both["medoid_pos"] >= 0) & (kept < 0)
    assert dropped.sum() >= 3 and (kept >= 0).sum() >= 3
    assert np.array_equal(both["flags"] & 1, (kept >= 0).astype(np.int32)) and (both["on_road"] == 0).all()
    assert np.array_equal(both["box"][kept >= 0, 0:9], only["box"][kept >= 0, 0:9])


def test_kitti_entry_point_with_depth_clustering(tmp_path, oracle):
    """src/kitti/2d_to_3d.py --depth-cluster 1 --obb device on one small frame: the labels' yaw is cm3d_obb of the clustered lists,
    their centre the clustered lists' medoid."""
    from cm3d_amd import kitti as kt, lifting, ops, synthetic as syn
    cfg = syn.config("tiny", n_points=60000, width=320, height=96, ratio=0.2, n_masks=16)
    kdir, mdir = tmp_path / "kitti", tmp_path / "masks"
    for d in (kdir / "training" / "velodyne", kdir / "training" / "calib", mdir):
        os.makedirs(d)
    fr, cal = syn.make_kitti_frame(cfg, 0)
    fr.sweeps_raw[0].astype(np.float32).tofile(kdir / "training" / "velodyne" / "000000.bin")
    with open(kdir / "training" / "calib" / "000000.txt", "w") as fh:
        for k, v in cal.items():
            fh.write(f"{k}: " + " ".join(repr(float(x)) for x in np.asarray(v).reshape(-1)) + "\n")
    pickle.dump(fr.rles, open(mdir / "0_masks.pkl", "wb"))
    json.dump({"labels": fr.labels, "detection_scores": fr.scores}, open(mdir / "0_data.json", "w"))
    r = subprocess.run([sys.executable, "2d_to_3d.py", "--kitti-dir", str(kdir), "--mask-dir", str(mdir), "--ratio", str(cfg.ratio),
                        "--depth-cluster", "1", "--obb", "device"],
                       cwd=os.path.join(ROOT, "src", "kitti"), capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-2000:]
    # the expectation: the plain pass's lists, clustered by the host statement (KITTI's origin is the reference camera: zeros)
    frame = kt.frame_from_files(0, str(kdir / "training" / "velodyne" / "000000.bin"), str(kdir / "training" / "calib" / "000000.txt"),
                                fr.rles, fr.labels, fr.scores, cfg.ratio)
    pri = json.load(open(os.path.join(ROOT, "src", "kitti", "cfg", "shape_priors_chatgpt.json")))       # what the entry point reads
    classes = lifting.ClassTable.nuscenes(pri)
    hb = lifting.pack_frames([frame], [[[0.0, 0.0, 0.0]]], [0], classes)
    assert not np.asarray(hb.ego_xyz).any()
    A = _run(lifting.LiftEngine("cuda:0", classes=classes), hb)
    exp = _host_clustered(hb, A, lifting.DepthCluster(1.0))
    off = exp["cl_off"]
    lists = [exp["cl_xyz"][off[m]:off[m + 1], :3] for m in range(hb.n_masks)]
    yaw, st, _ = ops.obb_yaws(lists)
    med = [oracle.medoid(exp["cl_xyz"], np.arange(off[m], off[m + 1], dtype=np.int32)) for m in range(hb.n_masks)]
    assert list(ops.get_medoids(lists)) == med
    cen = np.array([lists[m][med[m]] if med[m] >= 0 else np.zeros(3, np.float32) for m in range(hb.n_masks)], np.float32)
    res = dict(cl_off=off, cl_xyz=exp["cl_xyz"], hit_off=A["hit_off"], centroid=cen, obb_yaw=yaw, obb_status=st)
    pred, pseudo = kt.labels_of_frame(hb, res, 0, classes, pri, obb="device")
    assert open(kdir / "training" / "pred" / "000000.txt").read() == "".join(pred)
    assert open(kdir / "training" / "pseudo" / "000000.txt").read() == "".join(pseudo)
    n, kept = np.diff(A["hit_off"]), np.diff(off)
    assert len(pred) >= 3 and (kept < n).any()                # labels were written, and the clustering dropped points of some mask
    raw = [A["hit_xyz"][A["hit_off"][m]:A["hit_off"][m + 1], :3] for m in range(hb.n_masks)]
    ryaw, rst, _ = ops.obb_yaws(raw)
    plain_pred, _ = kt.labels_of_frame(hb, dict(A, obb_yaw=ryaw, obb_status=rst), 0, classes, pri, obb="device")
    assert plain_pred != pred                                 # ... which the labels show
