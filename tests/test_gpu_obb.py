"""GPU: KITTI's oriented-box yaw on the device (cm3d_obb, src/kitti/2d_to_3d.py:855-876, :1524) -- the euler step against scipy,
the hull vertices against Qhull, the fit against the canonical host restatement kitti.obb_canonical, degenerate lists, the engine
stage (LiftEngine(obb=True)) and the KITTI entry point with --obb device."""
import json
import os
import pickle
import subprocess
import sys
import warnings

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden")


def _ang(a, b):
    return np.abs((np.asarray(a) - np.asarray(b) + np.pi) % (2 * np.pi) - np.pi)


def _g3b_lists():
    g = np.load(os.path.join(GOLDEN, "g3b_medoid_lists.npz"))
    pts, off = g["pts"], g["off"]
    return [pts[off[k]:off[k + 1], :3].astype(np.float32) for k in range(len(off) - 1)]


def _box_surface(rng, m, dims):
    c = rng.uniform(-1, 1, (m, 3))
    ax = rng.integers(0, 3, m)
    c[np.arange(m), ax] = rng.choice([-1.0, 1.0], m)
    c = np.concatenate([c, [[sx, sy, sz] for sx in (-1, 1) for sy in (-1, 1) for sz in (-1, 1)]])
    return (c * dims).astype(np.float32)


def _hull_clouds():
    """(cloud, strict) pairs; strict: exactly coplanar face points whose status Qhull and the device both decide exactly (no
    exclusion allowed)."""
    rng = np.random.default_rng(21)
    out = []
    for m in (4, 5, 8, 20, 50, 120, 500, 2000, 5000, 20000):
        out.append((rng.normal(size=(m, 3)) * [3.0, 1.5, 0.8], False))                       # Gaussian
        out.append((rng.uniform(-1, 1, (m, 3)) * [2.0, 1.0, 0.7], False))                    # uniform cube
        out.append((_box_surface(rng, m, [2.0, 1.0, 0.5]), True))                           # box surface: only the 8 corners
        c = rng.normal(size=(m, 3))
        out.append((np.concatenate([c, c[rng.integers(0, m, max(1, m // 3))]]), False))     # duplicated rows
        out.append((rng.normal(size=(m, 3)) * [2.0, 1.0, 0.6] + [1000.0, -1300.0, 4.0], False))   # 10^3 m from the origin
    return [(np.asarray(c, np.float32), s) for c, s in out]


def _near_plane(c, hull, rel=1e-9):
    """Some point within `rel` (relative to the list's extent) of a facet plane of scipy's hull without being one of its vertices
    (or a copy of one)."""
    p = np.asarray(c, np.float64)
    scale = max(float(np.abs(p - p.mean(0)).max()), 1e-300)
    d = np.abs(p @ hull.equations[:, :3].T + hull.equations[:, 3])
    near = (d <= rel * scale).any(1)
    verts = _keyset(np.asarray(c)[hull.vertices])
    return any(near[i] and tuple(np.asarray(c[i], np.float32).tolist()) not in verts for i in range(len(p)))


def _keyset(a):
    return {tuple(r) for r in np.asarray(a, np.float32).tolist()}


def test_obb_euler_selftest_against_scipy():
    """as_euler('zyx')[0] on the device: 10^5 random rotations to 1e-12; matrices 1e-9 ... 1e-6 from gimbal lock to scipy's value
    (its locked branch where it takes it) within 1e-9."""
    from scipy.spatial.transform import Rotation
    from cm3d_amd import ops
    R = Rotation.random(100000, random_state=7).as_matrix()
    got = ops.obb_selftest_yaw(R)
    want = Rotation.from_matrix(R).as_euler("zyx")[:, 0]
    assert _ang(got, want).max() <= 1e-12
    rng = np.random.default_rng(8)
    n = 4000
    a, c = rng.uniform(-np.pi, np.pi, n), rng.uniform(-np.pi, np.pi, n)
    b = rng.choice([np.pi / 2, -np.pi / 2], n) + 10 ** rng.uniform(-9, -6, n) * rng.choice([-1.0, 1.0], n)
    R = Rotation.from_euler("zyx", np.stack([a, b, c], 1)).as_matrix()
    got = ops.obb_selftest_yaw(R)
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")               # scipy warns at gimbal lock
        want = np.array([Rotation.from_matrix(r).as_euler("zyx")[0] for r in R])
    assert _ang(got, want).max() <= 1e-9


def test_obb_hull_vertices_match_qhull():
    """Vertex marks of one cm3d_obb call over every kind of list against ConvexHull(p).vertices, as coordinate sets."""
    from scipy.spatial import ConvexHull
    from cm3d_amd import ops
    pairs = [(c, s) for c, s in _hull_clouds() + [(g, False) for g in _g3b_lists()] if len(c) >= 4]
    lists = [c for c, _ in pairs]
    yaw, st, R, verts = ops.obb_yaws(lists, vertices=True)
    excluded, checked = 0, 0
    for k, (c, strict) in enumerate(pairs):
        hull = ConvexHull(c.astype(np.float64))
        want, got = _keyset(c[hull.vertices]), _keyset(c[verts[k]])
        assert st[k] == 0, (k, st[k])
        assert len(verts[k]) == len(got), k                   # one position per distinct vertex
        if strict:
            assert len(want) == 8
        if got != want:
            assert not strict and _near_plane(c, hull), (k, len(c), len(want), len(got))
            excluded += 1
        checked += 1
    print(f"hull: {checked} lists, {excluded} excluded (a point within 1e-9 of a facet plane)")
    assert checked > 350 and excluded <= 0.02 * checked


def _fit_clouds():
    rng = np.random.default_rng(31)
    out = []
    for k in range(500):
        m = int(rng.choice([4, 6, 10, 30, 50, 80, 200, 1000, 3000]))
        kind = k % 3
        if kind == 0:
            c = rng.normal(size=(m, 3)) * rng.uniform(0.2, 4.0, 3)
        elif kind == 1:
            c = rng.uniform(-1, 1, (m, 3)) * rng.uniform(0.2, 4.0, 3)
        else:
            c = _box_surface(rng, m, rng.uniform(0.3, 3.0, 3))
        a, tilt = rng.uniform(-np.pi, np.pi), rng.normal(scale=0.2, size=2)
        Rz = np.array([[np.cos(a), -np.sin(a), 0], [np.sin(a), np.cos(a), 0], [0, 0, 1]])
        Rx = np.array([[1, 0, 0], [0, np.cos(tilt[0]), -np.sin(tilt[0])], [0, np.sin(tilt[0]), np.cos(tilt[0])]])
        out.append((np.asarray(c) @ (Rz @ Rx).T + rng.uniform(-80, 80, 3)).astype(np.float32))
    return out


EIG_GAP_MIN = 1e-3      # below this relative eigenvalue gap a 1e-9 comparison cannot pin the eigenvectors: such lists are left out, and counted


def _eig_gap(c, vidx):
    h = np.asarray(c, np.float64)[vidx]
    w = np.linalg.eigvalsh(np.cov(h.T, bias=True))
    return float(np.min(np.diff(w)) / max(w[-1], 1e-300))


def test_obb_fit_matches_canonical_restatement():
    """Rm and yaw of 500 random clouds and the G3b lists equal kitti.obb_canonical to 1e-9; only lists with a relative eigenvalue gap
    below 1e-3 (eigenvectors that a 1e-9 comparison cannot pin) are left out, and counted."""
    from cm3d_amd import kitti as kt, ops
    lists = [c for c in _fit_clouds() + _g3b_lists() if len(c) >= 4]
    yaw, st, R = ops.obb_yaws(lists)
    small_gap = 0
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        for k, c in enumerate(lists):
            yc, Rc, vidx = kt.obb_canonical(c)
            if _eig_gap(c, vidx) < EIG_GAP_MIN:
                small_gap += 1
                continue
            assert st[k] == 0, k
            assert np.abs(R[k] - Rc).max() <= 1e-9, (k, R[k], Rc)
            assert _ang(yaw[k], yc) <= 1e-9, (k, yaw[k], yc)
    print(f"fit: {len(lists)} lists, {small_gap} left out with a relative eigenvalue gap below 1e-3")
    assert len(lists) - small_gap >= 700


def _sphere(rng, m, radius, centre):
    v = rng.normal(size=(m, 3))
    return (v / np.linalg.norm(v, axis=1, keepdims=True) * radius + centre).astype(np.float32)


def test_obb_convex_position_lists_alone_in_a_call():
    """Lists whose every point is a hull vertex (sphere and cylinder surfaces: hulls far beyond the facets LDS holds), each alone in a
    call whose capacity is exactly its length -- the tightest workspace a caller can have: status 0, vertices = Qhull's, fit =
    kitti.obb_canonical.  Then all of them in one call, with the same results."""
    from scipy.spatial import ConvexHull
    from cm3d_amd import kitti as kt, ops
    rng = np.random.default_rng(41)
    lists = [_sphere(rng, m, r, c) for m, r, c in ((150, 1.0, [0, 0, 0]), (400, 2.5, [300.0, -20.0, 1.0]), (3000, 1.5, [-800.0, 1200.0, 2.0]))]
    t = rng.uniform(-np.pi, np.pi, 1000)
    lists.append(np.stack([2.0 * np.cos(t), 0.8 * np.sin(t), rng.uniform(-0.5, 0.5, 1000)], 1).astype(np.float32))   # elliptic cylinder wall
    alone = [ops.obb_yaws([c], vertices=True) for c in lists]
    yaw, st, R, verts = ops.obb_yaws(lists, vertices=True)
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        for k, c in enumerate(lists):
            y1, s1, R1, v1 = alone[k]
            assert s1[0] == 0 and st[k] == 0, (k, s1[0], st[k])
            hull = ConvexHull(c.astype(np.float64))
            assert _keyset(c[v1[0]]) == _keyset(c[hull.vertices]), (k, len(v1[0]), len(hull.vertices))
            assert len(hull.vertices) > 100
            assert y1[0] == yaw[k] and np.array_equal(R1[0], R[k]) and np.array_equal(v1[0], verts[k])
            yc, Rc, vidx = kt.obb_canonical(c)
            if _eig_gap(c, vidx) >= 1e-3:
                assert np.abs(R[k] - Rc).max() <= 1e-9 and _ang(yaw[k], yc) <= 1e-9, k


def test_obb_known_answers():
    """test_host_logic's known answers on the device: an axis-aligned box has yaw 0 (mod pi), turned by 30, -20 or 40 degrees about z
    the yaw is +- the turn (mod pi)."""
    from cm3d_amd import ops
    rng = np.random.default_rng(4)
    box = rng.uniform(-0.5, 0.5, (400, 3)) * [4.2, 1.8, 1.4]
    box = np.concatenate([box, np.array([[sx * 2.1, sy * 0.9, sz * 0.7] for sx in (-1, 1) for sy in (-1, 1) for sz in (-1, 1)])])
    lists = [box + [10.0, -3.0, 25.0]]
    turns = (30.0, -20.0, 40.0)
    for deg in turns:
        a = np.deg2rad(deg)
        Rz = np.array([[np.cos(a), -np.sin(a), 0], [np.sin(a), np.cos(a), 0], [0, 0, 1]])
        lists.append(box @ Rz.T + [3.0, 1.0, 12.0])
    yaw, st, _ = ops.obb_yaws(lists)
    assert (st == 0).all()

    def mod_pi(a):
        return (a + np.pi / 2) % np.pi - np.pi / 2

    assert abs(mod_pi(yaw[0])) < 1e-6
    for y, deg in zip(yaw[1:], turns):
        a = np.deg2rad(deg)
        assert min(abs(mod_pi(y - a)), abs(mod_pi(y + a))) < 1e-6, (deg, y)


def test_obb_degenerate_lists_beside_normal_ones():
    """Flat, collinear, all-identical and four coplanar points: status 2, yaw 0, R = identity; <= 3 points: status 1, yaw NaN.  The
    normal lists of the same call give the same bits as in a call of their own."""
    from scipy.spatial import ConvexHull
    from cm3d_amd import ops
    rng = np.random.default_rng(9)
    normal = [rng.normal(size=(m, 3)).astype(np.float32) * [2, 1, 0.5] for m in (4, 60, 700, 20000)]
    flat = np.concatenate([rng.normal(size=(80, 2)), np.full((80, 1), 3.25)], 1)
    t = rng.integers(-40, 40, 50)[:, None].astype(np.float64)
    collinear = np.array([1.0, -2.0, 0.5]) + t * np.array([0.5, 0.25, -1.0])      # exactly collinear in float32
    same = np.tile([[7.5, -1.25, 0.5]], (12, 1))
    coplanar4 = np.array([[0, 0, 0], [1, 0, 0], [0, 1, 0], [1, 1, 0.0]]) + [500.0, 20.0, 1.0]
    for c in (flat, collinear, same, coplanar4):                                       # Qhull has no hull for any of them either
        with pytest.raises(Exception):
            ConvexHull(np.asarray(c, np.float32).astype(np.float64))
    tiny = [np.zeros((0, 3)), rng.normal(size=(1, 3)), rng.normal(size=(2, 3)), rng.normal(size=(3, 3))]
    mixed = [normal[0], flat, normal[1], collinear, tiny[0], same, normal[2], tiny[1], coplanar4, tiny[2], normal[3], tiny[3]]
    kinds = ["n", "d", "n", "d", "t", "d", "n", "t", "d", "t", "n", "t"]
    yaw, st, R = ops.obb_yaws([np.asarray(c, np.float32) for c in mixed])
    y0, s0, R0 = ops.obb_yaws(normal)
    ni = 0
    for k, kind in enumerate(kinds):
        if kind == "d":
            assert st[k] == 2 and yaw[k] == 0.0 and np.array_equal(R[k], np.eye(3)), (k, st[k], yaw[k])
        elif kind == "t":
            assert st[k] == 1 and np.isnan(yaw[k]), (k, st[k])
        else:
            assert st[k] == 0 and s0[ni] == 0
            assert yaw[k] == y0[ni] and np.array_equal(R[k], R0[ni]), k
            ni += 1


def _kitti_frames(n, cfg):
    from cm3d_amd import synthetic as syn
    return [syn.make_kitti_frame(cfg, i)[0] for i in range(n)]


@pytest.mark.parametrize("raw_layout", ["quads", "rows"], indirect=True)
def test_engine_obb_stage(raw_layout):
    """LiftEngine(obb=True) on KITTI-shaped frames: obb_yaw equals ops.obb_yaws on the downloaded hit_xyz, every other result is
    bit-identical to obb=False, and a second pass and a graph replay give the same OBB outputs."""
    import torch
    from cm3d_amd import lifting, ops, synthetic as syn
    cfg = syn.config("tiny", n_points=20000, width=320, height=96, ratio=0.2, n_masks=12)
    frames = _kitti_frames(4, cfg)
    classes = lifting.ClassTable.nuscenes()
    hb = lifting.pack_frames(frames, [[[0.0, 0.0, 0.0]]], [0] * len(frames), classes)
    assert (hb.raw_stride == lifting._lib.RAW_QUADS) == (raw_layout == "quads")
    outs = {}
    for obb in (False, True):
        eng = lifting.LiftEngine("cuda:0", classes=classes, obb=obb)
        eng.upload(hb)
        eng.run(masks="rle")
        torch.cuda.synchronize()
        outs[obb] = (eng, eng.download())
    a, b = outs[False][1], outs[True][1]
    assert "obb_yaw" not in a and "obb_yaw" in b
    for key in a:
        assert np.array_equal(a[key], b[key], equal_nan=True), key
    eng = outs[True][0]
    off = b["hit_off"]
    lists = [b["hit_xyz"][off[m]:off[m + 1], :3] for m in range(len(off) - 1)]
    assert sum(len(x) > 3 for x in lists) >= 10
    yaw, st, _ = ops.obb_yaws(lists)
    assert np.array_equal(st, b["obb_status"]) and np.array_equal(yaw, b["obb_yaw"], equal_nan=True)
    assert (b["obb_status"][[len(x) > 3 for x in lists]] != 1).all()
    # the per-mask download carries the OBB results as well
    small = eng.download(full=False)
    assert np.array_equal(small["obb_yaw"], b["obb_yaw"], equal_nan=True) and np.array_equal(small["obb_status"], b["obb_status"])
    # a second pass, then a captured graph
    eng.b.obb_yaw.fill_(123.0)
    eng.run(masks="rle")
    torch.cuda.synchronize()
    again = eng.download(full=False)
    assert np.array_equal(again["obb_yaw"], b["obb_yaw"], equal_nan=True)
    g = eng.capture_graph(masks="rle")
    eng.b.obb_yaw.fill_(123.0)
    eng.b.obb_status.fill_(77)
    g.replay()
    torch.cuda.synchronize()
    rep = eng.download(full=False)
    assert np.array_equal(rep["obb_yaw"], b["obb_yaw"], equal_nan=True) and np.array_equal(rep["obb_status"], b["obb_status"])
    assert np.array_equal(rep["box"], b["box"]) and np.array_equal(rep["flags"], b["flags"])


def test_kitti_entry_point_device_obb(tmp_path, oracle):
    """src/kitti/2d_to_3d.py --obb device on the files test_kitti_entry_point writes: the same files and lines as the default run,
    every field but the yaw string-identical, the yaw within 1e-9 of kitti.obb_canonical on the oracle's in-mask lists."""
    from cm3d_amd import kitti as kt, lifting, synthetic as syn
    from tests.helpers import oracle_batch
    cfg = syn.config("tiny", width=320, height=96, ratio=0.2, n_masks=10)
    kdir, mdir = tmp_path / "kitti", tmp_path / "masks"
    for d in (kdir / "training" / "velodyne", kdir / "training" / "calib", mdir):
        os.makedirs(d)
    for i in range(3):
        fr, cal = syn.make_kitti_frame(cfg, i)
        fr.sweeps_raw[0].astype(np.float32).tofile(kdir / "training" / "velodyne" / f"{i:06d}.bin")
        with open(kdir / "training" / "calib" / f"{i:06d}.txt", "w") as fh:
            for k, v in cal.items():
                fh.write(f"{k}: " + " ".join(repr(float(x)) for x in np.asarray(v).reshape(-1)) + "\n")
        pickle.dump(fr.rles, open(mdir / f"{i}_masks.pkl", "wb"))
        json.dump({"labels": fr.labels, "detection_scores": fr.scores}, open(mdir / f"{i}_data.json", "w"))
    runs = {}
    for mode in ("host", "device"):
        extra = [] if mode == "host" else ["--obb", "device"]
        r = subprocess.run([sys.executable, "2d_to_3d.py", "--kitti-dir", str(kdir), "--mask-dir", str(mdir), "--ratio", str(cfg.ratio)] + extra,
                           cwd=os.path.join(ROOT, "src", "kitti"), capture_output=True, text=True, timeout=600)
        assert r.returncode == 0, r.stderr[-2000:]
        files = sorted(os.listdir(kdir / "training" / "pred")), sorted(os.listdir(kdir / "training" / "pseudo"))
        runs[mode] = (files, {(kind, f): open(kdir / "training" / kind / f).read().splitlines()
                              for kind, names in zip(("pred", "pseudo"), files) for f in names}, r.stdout)
    assert runs["host"][0] == runs["device"][0]
    assert runs["host"][2].split(" in ")[0] == runs["device"][2].split(" in ")[0]        # "wrote N labels for F frames"
    # the expected yaw: the canonical restatement on the oracle's lists of the same frames
    frames = []
    for i in range(3):
        rles = pickle.load(open(mdir / f"{i}_masks.pkl", "rb"))
        data = json.load(open(mdir / f"{i}_data.json"))
        frames.append(kt.frame_from_files(i, str(kdir / "training" / "velodyne" / f"{i:06d}.bin"), str(kdir / "training" / "calib" / f"{i:06d}.txt"),
                                          rles, data["labels"], data["detection_scores"], cfg.ratio))
    hb = lifting.pack_frames(frames, [[[0.0, 0.0, 0.0]]], [0] * 3)
    exp = oracle_batch(oracle, frames, [np.zeros((1, 3))], [0] * 3, hb)
    per_mask_frame = np.repeat(np.arange(3), np.diff(hb.mask_off))
    exp["hit_xyz"] = exp["points"][np.repeat(exp["pt_off"][per_mask_frame], np.diff(exp["hit_off"])) + exp["hit_idx"]]
    n_lines = 0
    for i in range(3):
        want = []
        for m in range(hb.mask_off[i], hb.mask_off[i + 1]):
            o, e = exp["hit_off"][m], exp["hit_off"][m + 1]
            if e - o <= 3:
                continue
            try:
                want.append(kt.obb_canonical(exp["hit_xyz"][o:e, :3])[0])
            except Exception:
                want.append(0.0)
        for kind, yaw_col in (("pred", -2), ("pseudo", -1)):
            host, dev = runs["host"][1][(kind, f"{i:06d}.txt")], runs["device"][1][(kind, f"{i:06d}.txt")]
            assert len(host) == len(dev) == len(want), (kind, i)
            for hl, dl, wy in zip(host, dev, want):
                hs, ds = hl.split(" "), dl.split(" ")
                assert len(hs) == len(ds)
                assert hs[:yaw_col] + hs[len(hs) + yaw_col + 1:] == ds[:yaw_col] + ds[len(ds) + yaw_col + 1:], (hl, dl)
                assert _ang(float(ds[yaw_col]), wy) <= 1e-9, (dl, wy)
                n_lines += 1
    assert n_lines > 6
