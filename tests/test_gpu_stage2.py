"""GPU: stage 2 (csrc/boxes.hip -- lane grid build and search, box assembly, the fused and the standalone circle NMS) in
the regimes real runs use and the synthetic parity frames never reach: city-scale lane tables (grown cells, crowded
cells, far rings, the exact-scan fallback, exact ties; tests/lane_maps.py, whose inputs test_lane_map_regimes.py
checks on the CPU), several different tables in one call, crowded NMS frames decided at the threshold's last bit, and
the push_centroid geometry at its branch points.  Every expectation is the CPU oracle, which the golden tests G4-G6
pin to the reference's own helpers.

Left out by design: NaN lane points (tests/lane_maps.py says why)."""
import json
import os
from concurrent.futures import ThreadPoolExecutor

import numpy as np
import pytest

from tests import lane_maps as lm

pytestmark = pytest.mark.gpu
G = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
BOX_TOL = 1e-4          # BASELINE.json north_star tolerance
# What is seen (test_box_assembly_geometry_sweep, 65 760 boxes): at most 2.2e-6, on the translation, where push_centroid's
# 1/sin, 1/cos amplify the one-ulp difference between the device's and the host's float32 cos/sin of the lane yaw (the Waymo
# set: 4e-8).  1e-5 leaves a factor of about 4.5 above that and stays ten times inside the north-star tolerance.
BOX_TIGHT = 1e-5


def _dev():
    import torch
    return torch.device("cuda", torch.cuda.current_device())


def _t(a, dtype=None):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a, dtype=dtype)).to(_dev())


def _st():
    import torch
    return torch.cuda.current_stream().cuda_stream


def _brute(oracle, cent, lane):
    """oracle.lane_nn (float64 brute force, first minimum) in chunks on a few threads (the C call releases the GIL)."""
    chunks = [(a, min(a + 64, cent.shape[0])) for a in range(0, cent.shape[0], 64)]
    with ThreadPoolExecutor(8) as ex:
        res = list(ex.map(lambda ab: oracle.lane_nn(cent[ab[0]:ab[1]], lane), chunks))
    if not res:
        return np.zeros(0, np.int32), np.zeros(0)
    return np.concatenate([r[0] for r in res]), np.concatenate([r[1] for r in res])


def _lane_lookup(tables, cent, mask_frame, frame_lane, medoid_pos):
    """cm3d_lane_grid_build + cm3d_lane_nn over all tables in one call of each."""
    import torch
    from cm3d_amd import _lib
    L = _lib.lib()
    lane32 = [np.asarray(t, np.float64).astype(np.float32).reshape(-1, 3) for t in tables]
    lane_off = np.concatenate([[0], np.cumsum([t.shape[0] for t in lane32])]).astype(np.int32)
    n_t, n_l, K = len(tables), int(lane_off[-1]), cent.shape[0]
    d_lane, d_off, d_fl = _t(np.concatenate(lane32)), _t(lane_off), _t(np.asarray(frame_lane, np.int32))
    d_c, d_med, d_mf = _t(cent, np.float32), _t(medoid_pos, np.int32), _t(mask_frame, np.int32)
    grid = torch.empty(int(L.cm3d_lane_grid_bytes(n_t, n_l)), dtype=torch.uint8, device=_dev())
    ws = torch.empty(max(16, int(L.cm3d_lane_nn_workspace_bytes(K))), dtype=torch.uint8, device=_dev())
    idx, dist = torch.empty(K, dtype=torch.int32, device=_dev()), torch.empty(K, dtype=torch.float64, device=_dev())
    _lib.check(L.cm3d_lane_grid_build(d_lane.data_ptr(), d_off.data_ptr(), n_t, n_l, grid.data_ptr(), grid.numel(), _st()),
               "cm3d_lane_grid_build")
    _lib.check(L.cm3d_lane_nn(d_c.data_ptr(), d_med.data_ptr(), d_mf.data_ptr(), K, d_lane.data_ptr(), d_off.data_ptr(), d_fl.data_ptr(),
                              n_t, n_l, grid.data_ptr(), idx.data_ptr(), dist.data_ptr(), ws.data_ptr(), ws.numel(), _st()), "cm3d_lane_nn")
    torch.cuda.synchronize()
    return idx.cpu().numpy(), dist.cpu().numpy()


def test_lane_lookup_on_city_maps_several_tables_in_one_call(oracle):
    """Five city maps (1.5-4 km, 0.4-0.55 M points, one at ~10 km) and six degenerate tables in ONE build and ONE search, a
    non-monotone frame -> table map, masks in shuffled order, a few without a medoid: index and distance of every centroid
    bit for bit the float64 brute force's; a sample also against scipy's cdist + argmin, the reference's own call."""
    from scipy.spatial.distance import cdist
    maps = lm.city_maps()
    tables = [m.lane for m in maps] + [t for _, t in lm.degenerate_tables(seed=7)]
    cents = [np.concatenate(list(lm.crafted_centroids(m, seed=k).values()), 0) for k, m in enumerate(maps)]
    cents += [lm.degenerate_centroids(t, seed=k) for k, t in enumerate(tables[len(maps):])]
    rng = np.random.default_rng(11)
    T = len(tables)
    frame_lane = rng.permutation(np.repeat(np.arange(T), 2)).astype(np.int32)          # two frames per table, any order
    frames_of = [np.flatnonzero(frame_lane == t) for t in range(T)]
    cent = np.concatenate(cents, 0)
    table_of = np.concatenate([np.full(c.shape[0], t) for t, c in enumerate(cents)])
    mask_frame = np.array([frames_of[t][rng.integers(0, 2)] for t in table_of], np.int32)
    perm = rng.permutation(cent.shape[0])
    cent, table_of, mask_frame = cent[perm], table_of[perm], mask_frame[perm]
    medoid_pos = np.where(rng.random(cent.shape[0]) < 0.02, -1, 0).astype(np.int32)
    idx, dist = _lane_lookup(tables, cent, mask_frame, frame_lane, medoid_pos)
    none = medoid_pos < 0
    assert (idx[none] == -1).all() and np.isinf(dist[none]).all()
    for t in range(T):
        sel = np.flatnonzero((table_of == t) & ~none)
        j, d = _brute(oracle, cent[sel], tables[t])
        bad = np.flatnonzero((idx[sel] != j) | (dist[sel].view(np.uint64) != d.view(np.uint64)))
        assert bad.size == 0, (t, bad.size, cent[sel[bad[:5]]].tolist(), idx[sel[bad[:5]]].tolist(), j[bad[:5]].tolist())
    # the reference's call on float32-rounded inputs, for a sample spread over every table
    for t in range(T):
        sel = np.flatnonzero((table_of == t) & ~none)[:40]
        l64 = np.asarray(tables[t], np.float64).astype(np.float32)[:, :2].astype(np.float64)
        for a in range(0, sel.size, 8):
            s = sel[a:a + 8]
            D = cdist(cent[s, :2].astype(np.float64), l64)
            j = np.argmin(D, axis=1)
            assert np.array_equal(idx[s], j) and np.array_equal(dist[s], D[np.arange(s.size), j]), t


def test_ring_stop_margin_decides_the_lane(oracle):
    """Tables on which the margin of the ring-stop test (k_lane_nn_grid: `best < r h - margin`) decides the answer
    (lane_maps.margin_cases, host-checked against an emulation of the search): a lane point the float32 binning puts one
    cell further out than it lies, nearer than r h, and a visited point between it and r h.  All tables in one call; index
    and distance bit for bit the brute force's.  A search that stops without the margin returns the visited point."""
    cases = lm.margin_cases()
    tables = [t for t, _, _ in cases]
    cent = np.stack([c for _, c, _ in cases])
    n = len(cases)
    idx, dist = _lane_lookup(tables, cent, np.arange(n, dtype=np.int32), np.arange(n, dtype=np.int32), np.zeros(n, np.int32))
    for k, (t, c, R) in enumerate(cases):
        j, d = oracle.lane_nn(c[None], t)
        assert idx[k] == j[0] and dist[k] == d[0], (k, R, int(idx[k]), int(j[0]), float(dist[k]), float(d[0]))


def _city_frames(n_default, n_far):
    from cm3d_amd import synthetic as syn
    near = [syn.make_frame(syn.config("tiny", seed=4321), i) for i in range(n_default)]          # ego ~(600, 1600) m
    far = [syn.make_frame(syn.config("tiny", seed=4321, ego_magnitude=10000.0), i) for i in range(n_far)]   # ego ~(3.5, 9.4) km
    return near + far


def test_lift_engine_on_city_maps_and_its_lane_index_cache(oracle):
    """Whole passes of LiftEngine with the egos inside city maps, one batch over three maps (one of them the ~10 km copy):
    every output equals the oracle's (test_gpu_parity._compare).  Then the engine's cache of lane indices: batch A (maps X),
    batch B (maps Y -- the same shapes, every point 1 m further east), A again on ONE engine: each pass gives its own batch's
    results."""
    import torch
    from cm3d_amd import lifting
    from tests.helpers import oracle_batch
    from tests.test_gpu_parity import _compare
    maps = lm.city_maps()
    frames = _city_frames(4, 2)
    tables_x = [maps[0].lane, maps[2].lane, maps[4].lane]
    frame_lane = [1, 0, 1, 0, 2, 2]
    tables_y = [t + np.array([1.0, 0.0, 0.0]) for t in tables_x]
    hb_a = lifting.pack_frames(frames, tables_x, frame_lane)
    hb_b = lifting.pack_frames(frames, tables_y, frame_lane)
    exp_a = oracle_batch(oracle, frames, tables_x, frame_lane, hb_a)
    exp_b = oracle_batch(oracle, frames, tables_y, frame_lane, hb_b)
    assert (exp_a["medoid_pos"] >= 0).sum() >= 20
    assert not np.array_equal(exp_a["lane_dist"], exp_b["lane_dist"])
    eng = lifting.LiftEngine("cuda:0")
    for hb, exp in ((hb_a, exp_a), (hb_b, exp_b), (hb_a, exp_a)):
        eng.upload(hb)
        eng.run(masks="rle")
        torch.cuda.synchronize()
        _compare(hb, eng.download(), exp)


# ------------------------------------------------------------------------------------------------ boxes + NMS
def _box_call(frames, tables, frame_lane, classes, pose_inv=None):
    """cm3d_box_nms over several frames in one call.  frames: dicts with cent (n,3) f32, cls, score, valid, lane_idx (into
    the frame's table), lane_dist, ego (3,).  Returns (box (M,10), flags (M,))."""
    import torch
    from cm3d_amd import _lib
    L = _lib.lib()
    n = [f["cent"].shape[0] for f in frames]
    mask_off = np.concatenate([[0], np.cumsum(n)]).astype(np.int32)
    M = int(mask_off[-1])
    cat = lambda k, dt: np.concatenate([np.asarray(f[k], dt).reshape(-1) for f in frames]) if M else np.zeros(1, dt)
    lane32 = [np.asarray(t, np.float64).astype(np.float32).reshape(-1, 3) for t in tables]
    lane_off = np.concatenate([[0], np.cumsum([t.shape[0] for t in lane32])]).astype(np.int32)
    d = dict(cent=_t(cat("cent", np.float32)), med=_t(np.where(cat("valid", bool), 0, -1).astype(np.int32)), off=_t(mask_off),
             cls=_t(cat("cls", np.int32)), score=_t(cat("score", np.float64)), lane=_t(np.concatenate(lane32)), lane_off=_t(lane_off),
             fl=_t(np.asarray(frame_lane, np.int32)), li=_t(cat("lane_idx", np.int32)), ld=_t(cat("lane_dist", np.float64)),
             prior=_t(classes.prior_wlh, np.float64), veh=_t(classes.is_vehicle, np.int32), grp=_t(classes.nms_group, np.int32),
             thr=_t(classes.nms_thr, np.float64), ego=_t(np.stack([np.asarray(f["ego"], np.float64) for f in frames]).reshape(-1)),
             inv=_t(pose_inv, np.float32) if pose_inv is not None else None)
    box = torch.empty(max(M, 1), _lib.BOX_STRIDE, dtype=torch.float64, device=_dev())
    flags = torch.empty(max(M, 1), dtype=torch.int32, device=_dev())
    _lib.check(L.cm3d_box_nms(d["cent"].data_ptr(), d["med"].data_ptr(), d["off"].data_ptr(), len(frames), max(M, 1), d["cls"].data_ptr(),
                              d["score"].data_ptr(), d["lane"].data_ptr(), d["lane_off"].data_ptr(), d["fl"].data_ptr(), d["li"].data_ptr(),
                              d["ld"].data_ptr(), d["prior"].data_ptr(), d["veh"].data_ptr(), d["grp"].data_ptr(), d["thr"].data_ptr(),
                              len(classes.names), d["ego"].data_ptr(), d["inv"].data_ptr() if d["inv"] is not None else 0,
                              box.data_ptr(), flags.data_ptr(), _st()), "cm3d_box_nms")
    torch.cuda.synchronize()
    return box.cpu().numpy()[:M], flags.cpu().numpy()[:M]


NMS_CLASSES = ["pedestrian", "traffic_cone", "bicycle", "motorcycle"]       # not pushed: translation = centroid, exactly


def _threshold_pair(T):
    """Two float32 centroids a = (ax, 0), b = (bx, by) whose squared distance, as the reference computes it in float64
    ((ax - bx)^2 + (0 - by)^2), is exactly T.  Host search: bx just above sqrt(T); the tiny ax moves (bx - ax)^2 in steps of
    ~1e-15 to just below T; by closes the gap (its square is far finer than one ulp of T)."""
    f32 = np.float32
    bx = np.nextafter(f32(np.sqrt(T)), f32(1), dtype=f32)
    for _ in range(3):
        bx = np.nextafter(bx, f32(1), dtype=f32)
    ax0 = f32(float(bx) - np.sqrt(T))
    cands = [ax0]
    for _ in range(200):
        cands.append(np.nextafter(cands[-1], f32(1), dtype=f32))
    for ax in cands:
        dx = float(ax) - float(bx)
        D = dx * dx
        if D > T:
            continue
        by0 = f32(np.sqrt(T - D))
        for k in range(-4, 5):
            by = by0
            for _ in range(abs(k)):
                by = np.nextafter(by, f32(np.inf) if k > 0 else f32(0), dtype=f32)
            dy = 0.0 - float(by)
            if D + dy * dy == T:
                return np.array([ax, 0.0], np.float32), np.array([bx, by], np.float32)
    raise AssertionError(f"no float32 pair at squared distance {T!r}")


def _crowd(n, rng, thr_by_cls, classes, tie=False):
    """n boxes of the four unpushed classes around (600, 1600): a chain longer than 64 (each box within the threshold of
    its neighbours only; decreasing scores, so every other one survives), a chain of the same shape with shuffled scores,
    dense clusters, boxes of other classes on the same spots; distinct scores except, with tie=True, one group of 16
    equal ones inside a cluster (the pinned rule: higher index first)."""
    xs, ys, cls = [], [], []
    n_chain = min(n // 3, 140)
    for c0, (y, shuffled) in enumerate(((1650.0, False), (1660.0, True))):
        if n_chain < 2:
            break
        ci = classes.index(NMS_CLASSES[c0])
        s = 0.6 * np.sqrt(thr_by_cls[ci])
        xs += list(600.0 + s * np.arange(n_chain)); ys += [y] * n_chain; cls += [ci] * n_chain
    rest = n - len(xs)
    if rest > 0:
        centres = rng.uniform([560, 1560], [640, 1640], (max(1, rest // 24), 2))
        k = rng.integers(0, centres.shape[0], rest)
        p = centres[k] + rng.normal(scale=0.35, size=(rest, 2))
        c = np.array([classes.index(NMS_CLASSES[i]) for i in rng.integers(0, 4, rest)])
        dup = rng.random(rest) < 0.2              # another class on the very spot of an earlier box
        dup[0] = False
        src = np.maximum(np.arange(rest) - 1, 0)
        p[dup] = p[src[dup]]
        c[dup] = np.array([classes.index(NMS_CLASSES[(NMS_CLASSES.index(classes.names[q]) + 1) % 4]) for q in c[src[dup]]])
        xs += list(p[:, 0]); ys += list(p[:, 1]); cls += list(c)
    xy = np.stack([xs, ys], 1)[:n].astype(np.float32)
    cls = np.array(cls[:n], np.int32)
    score = (0.05 + 0.9 * (rng.permutation(n) + 0.5) / n).astype(np.float64)
    if n_chain >= 2:
        score[:n_chain] = np.sort(score[:n_chain])[::-1]
    if tie and rest >= 40:
        k = rng.integers(0, rest)
        grp = n - rest + np.argsort(np.hypot(*(xy[n - rest:] - xy[n - rest + k]).T))[:16]
        score[grp] = 0.5123456789
    return xy, cls, score


def _nms_frames(classes, rng):
    thr = classes.nms_thr
    frames = []
    for n, tie in ((0, False), (1, False), (63, False), (64, False), (65, True), (200, True), (1024, True), (700, False)):
        xy, cls, score = _crowd(n, rng, thr, classes, tie)
        frames.append(dict(xy=xy, cls=cls, score=score))
    # threshold pairs at the origin: squared distance one ulp below, at, one ulp above the class threshold; each class
    # has its own pair on the same spot (the classes must not suppress each other)
    for side in (-1, 0, 1):
        xy, cls, score = [], [], []
        for name in NMS_CLASSES:
            ci = classes.index(name)
            T = float(thr[ci])
            T = T if side == 0 else float(np.nextafter(T, np.inf if side > 0 else 0.0))
            a, b = _threshold_pair(T)
            xy += [a, b]; cls += [ci, ci]; score += [0.999 - 0.001 * len(score), 0.998 - 0.001 * len(score)]
        c_xy, c_cls, c_score = _crowd(120, rng, thr, classes)         # a crowd elsewhere: the pairs sit behind 64 others
        frames.append(dict(xy=np.concatenate([c_xy, np.array(xy, np.float32)]), cls=np.concatenate([c_cls, cls]).astype(np.int32),
                           score=np.concatenate([c_score * 0.5 + 0.46, score]), pairs=True))
    for f in frames:
        nf = f["xy"].shape[0]
        f["cent"] = np.concatenate([f["xy"], rng.uniform(-1, 2, (nf, 1))], 1).astype(np.float32)
        f["valid"] = rng.random(nf) > 0.15
        if nf > 100:
            f["valid"][1::7] = False              # interleaved masks without a medoid
        if f.get("pairs"):
            f["valid"][-8:] = True
        f["lane_dist"] = rng.uniform(0, 30, nf)
        f["ego"] = np.array([598.0, 1603.0, 0.5])
    return frames


def test_crowded_frames_nms_equals_oracle(oracle):
    """The fused NMS of k_box_nms on frames of 0, 1, 63, 64, 65, 200, 1024 and 700 boxes plus three threshold frames: chains
    longer than 64, dense clusters, classes on the same spots, invalid masks interleaved, one tie group, pairs whose squared
    distance is the class threshold exactly and one double ulp either side.  Flags equal oracle.circle_nms (pinned to the
    reference by G5) frame by frame; the standalone kernel (ops.circle_nms) keeps the same set; every box column is the
    oracle's, the lane yaw looked up in each frame's own table (tables of different sizes, non-monotone frame -> table)."""
    from cm3d_amd import ops
    from cm3d_amd.lifting import THRESHS_BY_LABEL, ClassTable
    classes = ClassTable.nuscenes()
    rng = np.random.default_rng(21)
    frames = _nms_frames(classes, rng)
    F = len(frames)
    tables = [np.stack([np.zeros(s), np.zeros(s), rng.uniform(-np.pi, np.pi, s)], 1) for s in rng.integers(1, 1500, F)]
    frame_lane = rng.permutation(F).astype(np.int32)
    for f, t in zip(frames, frame_lane):
        f["lane_idx"] = rng.integers(0, tables[t].shape[0], f["cent"].shape[0])
    box, flags = _box_call(frames, tables, frame_lane, classes)
    off = np.concatenate([[0], np.cumsum([f["cent"].shape[0] for f in frames])])
    decided_at_threshold = 0
    for fi, f in enumerate(frames):
        b, fl = box[off[fi]:off[fi + 1]], flags[off[fi]:off[fi + 1]]
        v = f["valid"]
        c64 = f["cent"].astype(np.float64)
        keep = np.zeros(v.size, bool)
        vi = np.flatnonzero(v)
        if vi.size:
            keep[vi] = oracle.circle_nms(c64[vi, 0], c64[vi, 1], f["score"][vi], classes.nms_group[f["cls"][vi]], classes.nms_thr)
        want = v.astype(np.int32) | (keep.astype(np.int32) << 1)
        bad = np.flatnonzero(fl != want)
        assert bad.size == 0, (fi, v.size, bad[:10].tolist())
        assert np.array_equal(b[:, 9], want)
        dets = np.concatenate([c64[vi, :2], f["score"][vi, None]], 1)
        assert ops.circle_nms(dets, [classes.names[c] for c in f["cls"][vi]], THRESHS_BY_LABEL) == np.flatnonzero(keep[vi]).tolist(), fi
        yaw = np.asarray(tables[frame_lane[fi]], np.float64).astype(np.float32)[f["lane_idx"], 2].astype(np.float64)
        exp = np.zeros((v.size, 9))
        exp[:, 0:3] = np.where(v[:, None], c64, 0.0)
        exp[:, 3] = 1.0
        exp[:, 5] = np.where(v, yaw, 0.0)
        exp[:, 6] = np.where(v, f["lane_dist"], 0.0)
        exp[:, 7], exp[:, 8] = f["score"], f["cls"]
        assert np.array_equal(b[:, :9], exp), fi
        if fi >= F - 3:       # the threshold frames: at and below the threshold the lower score goes, above it stays
            pairs = slice(v.size - 8, v.size)
            decided_at_threshold += int((v[pairs][0::2] & v[pairs][1::2]).sum())
            for k in range(4):
                a, bb = v.size - 8 + 2 * k, v.size - 7 + 2 * k
                if v[a] and v[bb]:
                    assert keep[a] and keep[bb] == (fi == F - 1), (fi, k)
    assert decided_at_threshold >= 4
    assert (np.diff(off) > 64).sum() >= 5


# ------------------------------------------------------------------------------------------------ box geometry
def _host_theta(yaw32):
    """theta of push_centroid for a float32 lane yaw (2d_to_3d.py:164-198), to place centroids around it."""
    cs, sn = float(np.cos(np.float32(yaw32))), float(np.sin(np.float32(yaw32)))
    if cs < -cs:
        t = 1.0 - cs - cs + 1.0; fct = 0.5 / np.sqrt(t); qw, qz = (sn + sn) * fct, t * fct
    else:
        t = 1.0 + cs + cs + 1.0; fct = 0.5 / np.sqrt(t); qw, qz = t * fct, (sn + sn) * fct
    phi = 2.0 * np.arctan2(qw, qz)
    phi = phi - 2 * np.pi if phi > np.pi else (phi + 2 * np.pi if phi <= -np.pi else phi)
    return -phi


def _ulp_steps(v, ks):
    out = []
    for k in ks:
        x = np.float32(v)
        for _ in range(abs(k)):
            x = np.nextafter(x, np.float32(np.inf) if k > 0 else np.float32(-np.inf), dtype=np.float32)
        out.append(x)
    return out


def _geometry_frames(classes, rng):
    """One frame per (vehicle class, ego, lane yaw): yaws at and a few ulp around 0, +-pi/2, +-pi and random ones;
    centroids on and 1-2 ulp off the ego's axes, on the ego itself, and where theta - alpha is near 0, +-pi/2, pi and the
    angles where min(|w/2sin|, |l/2cos|) switches sides."""
    egos = [np.array([600.25, 1600.5, 1.0]), np.array([0.0, 0.0, 0.0]), np.array([3511.125, 9363.25, 0.5])]
    yaws = []
    for a in (0.0, np.pi / 2, -np.pi / 2, np.pi, -np.pi):
        yaws += _ulp_steps(a, range(-3, 4))
    yaws += list(rng.uniform(-np.pi, np.pi, 5).astype(np.float32))
    yaws = np.array(yaws, np.float32)
    frames, frame_yaw = [], []
    for ci in np.flatnonzero(classes.is_vehicle):
        w, l = classes.prior_wlh[ci, 0], classes.prior_wlh[ci, 1]
        sw = np.arctan2(l, w)                                        # o1 == o2 where |tan(theta - alpha)| = l / w (prior [w, l])
        for ego in egos:
            for yi, yaw in enumerate(yaws):
                th = _host_theta(yaw)
                pts = [ego[:2].astype(np.float32)]
                for axis in (0, 1):
                    for sgn in (-1.0, 1.0):
                        for e in _ulp_steps(ego[1 - axis], (-2, -1, 0, 1, 2)):
                            p = np.zeros(2, np.float32)
                            p[axis] = np.float32(ego[axis] + sgn * 7.5)
                            p[1 - axis] = e
                            pts.append(p)
                for base in (0.0, np.pi / 2, -np.pi / 2, np.pi, sw, -sw, np.pi - sw):
                    for eps in (0.0, 1e-7, -1e-7, 1e-4, -1e-4):
                        for R in (4.0, 30.0):
                            a = th - base + eps
                            pts.append(np.array([ego[0] + R * np.cos(a), ego[1] + R * np.sin(a)], np.float32))
                xy = np.array(pts, np.float32)
                n = xy.shape[0]
                frames.append(dict(cent=np.concatenate([xy, rng.uniform(-1, 2, (n, 1))], 1).astype(np.float32), cls=np.full(n, ci, np.int32),
                                   score=rng.uniform(0.1, 1, n), valid=np.ones(n, bool), lane_idx=np.full(n, yi, np.int32),
                                   lane_dist=rng.uniform(0, 5, n), ego=ego))
    return frames, yaws


def _compare_boxes(got_t, got_q, exp_t, exp_q, what):
    """Translations and quaternions (w, z) against the oracle: same NaN positions, same signs, north-star tolerance and the
    tight bound; returns the largest deviation."""
    assert np.array_equal(np.isnan(got_t), np.isnan(exp_t)), what
    ok = ~np.isnan(exp_t)
    dev_t = np.abs(got_t - exp_t)[ok].max() if ok.any() else 0.0
    dev_q = np.abs(got_q - exp_q).max()
    assert np.array_equal(np.sign(got_q), np.sign(exp_q)), (what, np.argwhere(np.sign(got_q) != np.sign(exp_q))[:5].tolist())
    assert dev_t < BOX_TOL and dev_q < BOX_TOL, (what, dev_t, dev_q)
    assert dev_t < BOX_TIGHT and dev_q < BOX_TIGHT, (what, dev_t, dev_q)
    return max(dev_t, dev_q)


def test_box_assembly_geometry_sweep(oracle):
    """push_centroid in k_box_nms against oracle.box_assemble (pinned by G4): all 240 G4 cases (and the reference's values
    in them), then dense sweeps for every pushed class over the branch points of the quaternion and of the offset."""
    from cm3d_amd.lifting import ClassTable
    classes = ClassTable.nuscenes()
    rng = np.random.default_rng(31)
    cases = json.load(open(os.path.join(G, "g4_push_centroid.json")))
    assert len(cases) == 240
    g4 = [dict(cent=np.array([c["centroid"]], np.float32), cls=np.array([c["class"]], np.int32), score=np.array([1.0]), valid=np.ones(1, bool),
               lane_idx=np.array([k], np.int32), lane_dist=np.zeros(1), ego=np.array(c["ego"], np.float64)) for k, c in enumerate(cases)]
    g4_table = np.stack([np.zeros(240), np.zeros(240), np.array([c["yaw"] for c in cases], np.float32).astype(np.float64)], 1)
    box, flags = _box_call(g4, [g4_table], np.zeros(240, np.int32), classes)
    exp_t, exp_q = [], []
    for c in cases:
        t, q = oracle.box_assemble(np.float32(c["centroid"]), oracle.PRIORS_WLH[c["class"]], np.float32(c["yaw"]), c["ego"],
                                   oracle.IS_VEHICLE[c["class"]])
        exp_t.append(t); exp_q.append(q[[0, 3]])
    worst = _compare_boxes(box[:, 0:3], box[:, 3:5], np.array(exp_t), np.array(exp_q), "G4")
    veh = oracle.IS_VEHICLE[[c["class"] for c in cases]]
    assert np.abs(box[veh, 0:3] - np.array([c["pushed"] for c in cases])[veh]).max() < BOX_TOL
    assert (flags & 1).all()
    frames, yaws = _geometry_frames(classes, rng)
    table = np.stack([np.zeros(yaws.size), np.zeros(yaws.size), yaws.astype(np.float64)], 1)
    box, flags = _box_call(frames, [table], np.zeros(len(frames), np.int32), classes)
    exp_t, exp_q = [], []
    for f in frames:
        for k in range(f["cent"].shape[0]):
            ci = int(f["cls"][k])
            t, q = oracle.box_assemble(f["cent"][k], oracle.PRIORS_WLH[ci], yaws[f["lane_idx"][k]], f["ego"], True)
            exp_t.append(t); exp_q.append(q[[0, 3]])
    exp_t, exp_q = np.array(exp_t), np.array(exp_q)
    worst = max(worst, _compare_boxes(box[:, 0:3], box[:, 3:5], exp_t, exp_q, "sweep"))
    assert box.shape[0] > 20000 and np.isnan(exp_t).any()
    print(f"box assembly: {box.shape[0] + 240} boxes, largest deviation from the oracle {worst:.3g}")


def test_waymo_box_assembly_across_the_heading_wrap(oracle):
    """The Waymo chain of stage 2 (centroid to the global frame, lane lookup, push in the vehicle frame with pose_inv, heading
    of R_inv Rz(lane yaw)) against oracle.stage2_frame_waymo, with lane yaws chosen so that the headings straddle +-pi.
    Headings are compared as angles (+pi and -pi are one heading; which of the two a float32 cos/sin ulp gives is not a
    difference); the side of the wrap each lands on is counted so the cases stay across it."""
    import torch
    from cm3d_amd import _lib, waymo as wm
    from cm3d_amd.lifting import ClassTable
    classes = ClassTable.waymo()
    rng = np.random.default_rng(41)
    L = _lib.lib()
    frames, tables, rts, invs = [], [], [], []
    for fi, (pyaw, tr) in enumerate(((0.3, (1234.5, -2345.25, 10.0)), (-2.9, (-310.75, 4021.0, -3.0)), (3.1, (5.5, 7.25, 0.0)),
                                     (-1.5707964, (8812.0, 1502.5, 20.0)))):
        P = np.eye(4)
        P[:2, :2] = [[np.cos(pyaw), -np.sin(pyaw)], [np.sin(pyaw), np.cos(pyaw)]]
        P[:3, 3] = tr
        rt, inv = wm.pose_records(P.reshape(16))
        n = 150
        cv = np.concatenate([rng.uniform(-40, 40, (n, 2)), rng.uniform(-1, 2, (n, 1))], 1).astype(np.float32)
        cg = np.array([oracle.centroid_transform(c, rt) for c in cv])
        eps = rng.choice([0.0, 1e-7, -1e-7, 1e-6, -1e-6, 1e-3, -1e-3, 0.05, -0.05], n)
        lyaw = np.angle(np.exp(1j * (pyaw + np.pi + eps)))
        lane = np.concatenate([cg[:, :2].astype(np.float64) + rng.uniform(-0.8, 0.8, (n, 2)), lyaw[:, None]], 1)
        frames.append(dict(cv=cv, cls=rng.integers(0, 10, n).astype(np.int32), score=np.float32(rng.uniform(0.1, 1, n)).astype(np.float64),
                           valid=rng.random(n) > 0.1))
        tables.append(lane); rts.append(rt); invs.append(inv)
    F = len(frames)
    off = np.concatenate([[0], np.cumsum([f["cv"].shape[0] for f in frames])]).astype(np.int32)
    M = int(off[-1])
    mask_frame = np.repeat(np.arange(F), np.diff(off)).astype(np.int32)
    med = np.concatenate([np.where(f["valid"], 0, -1) for f in frames]).astype(np.int32)
    d_cv, d_med, d_mf = _t(np.concatenate([f["cv"] for f in frames])), _t(med), _t(mask_frame)
    d_rt = _t(np.stack(rts), np.float32)
    d_cg = torch.empty(M, 3, dtype=torch.float32, device=_dev())
    _lib.check(L.cm3d_centroid_transform(d_cv.data_ptr(), d_med.data_ptr(), d_mf.data_ptr(), M, d_rt.data_ptr(), d_cg.data_ptr(), _st()),
               "cm3d_centroid_transform")
    torch.cuda.synchronize()
    cg_all = d_cg.cpu().numpy()
    frame_lane = np.arange(F, dtype=np.int32)
    idx, dist = _lane_lookup(tables, cg_all, mask_frame, frame_lane, med)
    bframes = []
    for fi, f in enumerate(frames):
        s = slice(off[fi], off[fi + 1])
        bframes.append(dict(cent=cg_all[s], cls=f["cls"], score=f["score"], valid=f["valid"], lane_idx=np.maximum(idx[s], 0),
                            lane_dist=np.where(f["valid"], dist[s], 0.0), ego=np.zeros(3)))
    box, flags = _box_call(bframes, tables, frame_lane, classes, pose_inv=np.stack(invs))
    worst, sides = 0.0, set()
    for fi, f in enumerate(frames):
        s = slice(off[fi], off[fi + 1])
        e = oracle.stage2_frame_waymo(f["cv"], np.where(f["valid"], 0, -1), f["cls"], f["score"], tables[fi], rts[fi], invs[fi])
        v = f["valid"]
        assert np.array_equal(cg_all[s][v].view(np.uint32), e["centroid_global"][v].view(np.uint32)), fi
        assert np.array_equal(idx[s][v], e["lane_idx"][v]) and np.array_equal(dist[s][v], e["lane_dist"][v]), fi
        assert np.array_equal(flags[s], v.astype(np.int32) | (e["keep"].astype(np.int32) << 1)), fi
        b = box[s]
        assert np.abs(b[v, 0:3] - e["translation"][v]).max() < BOX_TIGHT, fi
        dh = np.angle(np.exp(1j * (b[v, 3] - e["heading"][v])))
        assert np.abs(dh).max() < BOX_TIGHT, fi
        veh = v & classes.is_vehicle[f["cls"]].astype(bool)
        sides |= set(np.sign(e["heading"][veh]).tolist())
        worst = max(worst, np.abs(b[v, 0:3] - e["translation"][v]).max(), np.abs(dh).max())
    assert sides >= {-1.0, 1.0}
    print(f"waymo box assembly: largest deviation from the oracle {worst:.3g}")
