"""CPU: the C-ABI of the device OBB fit (ABI v5: cm3d_obb, cm3d_obb_workspace_bytes, cm3d_selftest_obb_yaw) and the host
restatement with canonical eigenvector signs (kitti.obb_canonical), pinned against the reference's restatement kitti.obb_yaw
(src/kitti/2d_to_3d.py:855-876, :1524) up to the signs of the eigenvectors."""
import ctypes
import itertools

import numpy as np
import pytest


def test_obb_symbols_exported_and_abi_v5():
    from cm3d_amd import _lib
    h = ctypes.CDLL(_lib.LIB_PATH)
    for name in ("cm3d_obb", "cm3d_obb_workspace_bytes", "cm3d_selftest_obb_yaw"):
        assert hasattr(h, name), name
        assert name in _lib.SIGNATURES
    assert _lib.ABI_VERSION == 5 and _lib.lib().cm3d_abi_version() == 5


def test_obb_workspace_size_is_positive_and_monotone():
    from cm3d_amd import _lib
    L = _lib.lib()
    assert L.cm3d_obb_workspace_bytes(0, 100) == 0 and L.cm3d_obb_workspace_bytes(10, 0) == 0
    prev = 0
    for m, cap in ((1, 1), (1, 4), (20, 1024), (20, 5000), (5120, 5000), (5120, 10 ** 6), (5120, 2 * 10 ** 8), (6000, 2 * 10 ** 8)):
        b = L.cm3d_obb_workspace_bytes(m, cap)
        assert b > 0 and b >= prev, (m, cap, b, prev)
        prev = b
    for cap in (10, 1000, 10 ** 5, 10 ** 7):
        assert L.cm3d_obb_workspace_bytes(50, cap) <= L.cm3d_obb_workspace_bytes(51, cap) <= L.cm3d_obb_workspace_bytes(51, cap + 1)


def test_obb_argument_errors_never_launch():
    from cm3d_amd import _lib
    L = _lib.lib()
    buf = ctypes.create_string_buffer(4096)
    p = ctypes.addressof(buf)
    assert L.cm3d_obb(0, p, 1, 16, p, p, 0, 0, p, 4096, 0) == -1            # null points
    assert L.cm3d_obb(p, 0, 1, 16, p, p, 0, 0, p, 4096, 0) == -1            # null offsets
    assert L.cm3d_obb(p, p, 1, 16, 0, p, 0, 0, p, 4096, 0) == -1            # null yaw
    assert L.cm3d_obb(p, p, 1, 16, p, 0, 0, 0, p, 4096, 0) == -1            # null status
    assert L.cm3d_obb(p, p, 1, 16, p, p, 0, 0, 0, 4096, 0) == -1            # null workspace
    assert L.cm3d_obb(p, p, 0, 16, p, p, 0, 0, p, 4096, 0) == -1            # no masks
    assert L.cm3d_obb(p, p, 1, 0, p, p, 0, 0, p, 4096, 0) == -1             # no capacity
    assert L.cm3d_obb(p, p, 1, 16, p, p, 0, 0, p, 8, 0) == -3               # workspace too small
    assert L.cm3d_selftest_obb_yaw(0, 1, p, 0) == -1 and L.cm3d_selftest_obb_yaw(p, 1, 0, 0) == -1
    assert L.cm3d_selftest_obb_yaw(p, 0, p, 0) == -1


def _yaw_with_signs(pts, signs):
    """kitti.obb_yaw with the eigenvectors of eigh multiplied by `signs` (one of the 8 sign patterns LAPACK could return)."""
    from scipy.spatial import ConvexHull
    from scipy.spatial.transform import Rotation
    p = np.asarray(pts, np.float64)
    hull = p[ConvexHull(p).vertices]
    mean = hull.mean(0)
    cov = (hull - mean).T @ (hull - mean) / hull.shape[0]
    w, v = np.linalg.eigh(cov)
    Rm = (v * np.asarray(signs, np.float64))[:, ::-1].copy()
    if np.linalg.det(Rm) < 0:
        Rm[:, 2] = -Rm[:, 2]
    size = p.max(0) - p.min(0)
    axis = [a for _, a in sorted(zip(size, "xyz"), key=lambda t: t[0])]
    Rm = np.stack([Rm[:, axis.index("z")], Rm[:, axis.index("y")], Rm[:, axis.index("x")]], axis=1)
    if np.linalg.det(Rm) < 0:
        Rm[:, 0] = -Rm[:, 0]
    return float(Rotation.from_matrix(Rm).as_euler("zyx")[0])


def _ang(a, b):
    return abs((a - b + np.pi) % (2 * np.pi) - np.pi)


def _test_box():
    rng = np.random.default_rng(4)                 # the known-answer box of test_host_logic.test_kitti_obb_yaw_known_answers
    box = rng.uniform(-0.5, 0.5, (400, 3)) * [4.2, 1.8, 1.4]
    return np.concatenate([box, np.array([[sx * 2.1, sy * 0.9, sz * 0.7] for sx in (-1, 1) for sy in (-1, 1) for sz in (-1, 1)])])


def _clouds(n, seed):
    rng = np.random.default_rng(seed)
    out = []
    for k in range(n):
        m = int(rng.integers(4, 400))
        c = rng.normal(size=(m, 3)) * rng.uniform(0.2, 4.0, 3)
        a = rng.uniform(-np.pi, np.pi)
        Rz = np.array([[np.cos(a), -np.sin(a), 0], [np.sin(a), np.cos(a), 0], [0, 0, 1]])
        out.append((c @ Rz.T + rng.uniform(-50, 50, 3)).astype(np.float32))
    return out


def test_canonical_restatement_is_obb_yaw_up_to_eigenvector_signs():
    import warnings
    from cm3d_amd import kitti as kt
    box = _test_box()
    clouds = [box + [10.0, -3.0, 25.0]]
    for deg in (30.0, -20.0, 40.0):
        a = np.deg2rad(deg)
        Rz = np.array([[np.cos(a), -np.sin(a), 0], [np.sin(a), np.cos(a), 0], [0, 0, 1]])
        clouds.append(box @ Rz.T + [3.0, 1.0, 12.0])
    clouds += _clouds(200, 11)
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")                # scipy warns at gimbal lock
        for c in clouds:
            yc, Rm, vidx = kt.obb_canonical(c)
            assert np.allclose(Rm.T @ Rm, np.eye(3), atol=1e-12) and abs(np.linalg.det(Rm) - 1) < 1e-12
            family = [_yaw_with_signs(c, s) for s in itertools.product((1.0, -1.0), repeat=3)]
            assert min(_ang(yc, y) for y in family) < 1e-9, (yc, family)
            assert min(_ang(kt.obb_yaw(c), y) for y in family) < 1e-9
            assert np.array_equal(np.sort(vidx), vidx)
    # canonical: every column's largest component is positive after the eigen-solve -- the known answers hold for it as well
    assert min(_ang(kt.obb_canonical(box)[0], 0.0), _ang(kt.obb_canonical(box)[0], np.pi)) < 1e-6


def test_canonical_restatement_raises_exactly_where_obb_yaw_raises():
    from cm3d_amd import kitti as kt
    rng = np.random.default_rng(5)
    cases = [np.array([[0, 0, 0], [1, 0, 0], [2, 0, 0], [3, 0, 0.0]]),                     # collinear
             np.concatenate([rng.normal(size=(50, 2)), np.full((50, 1), 2.5)], 1),         # flat
             np.ones((7, 3)),                                                              # one point, repeated
             np.array([[0, 0, 0], [1, 0, 0], [0, 1, 0], [1, 1, 0.0]]),                     # four coplanar points
             rng.normal(size=(30, 3)), _test_box()]
    for c in cases:
        try:
            kt.obb_yaw(c)
            host_raises = False
        except Exception:
            host_raises = True
        try:
            kt.obb_canonical(c)
            canon_raises = False
        except Exception:
            canon_raises = True
        assert host_raises == canon_raises
    assert all(_raises(kt.obb_canonical, c) for c in cases[:4]) and not any(_raises(kt.obb_canonical, c) for c in cases[4:])


def _raises(f, *a):
    try:
        f(*a)
        return False
    except Exception:
        return True


def test_canonical_signs_rule():
    from cm3d_amd import kitti as kt
    v = np.array([[0.6, -0.8, 0.0], [-0.8, -0.6, 0.0], [0.0, 0.0, -1.0]])
    c = kt.canonical_signs(v)
    assert np.array_equal(c, np.array([[-0.6, 0.8, 0.0], [0.8, 0.6, 0.0], [0.0, 0.0, 1.0]]))
    tie = np.array([[-np.sqrt(0.5)], [np.sqrt(0.5)], [0.0]])          # exact tie: the first component decides
    assert np.array_equal(kt.canonical_signs(tie), -tie)


def test_labels_of_frame_device_mode_reads_device_yaw():
    """obb="device": the yaw comes from res["obb_yaw"] (status 2 -> 0.0), hit_xyz is not needed; every other field as in host mode."""
    from types import SimpleNamespace
    from cm3d_amd import kitti as kt, lifting
    hb = SimpleNamespace(mask_off=np.array([0, 3]), labels=[["car", "pedestrian", "car"]], score=np.array([0.9, 0.8, 0.7]))
    res = dict(hit_off=np.array([0, 10, 15, 17]), centroid=np.array([[1.0, 2.0, 3.0], [4.0, 5.0, 6.0], [7.0, 8.0, 9.0]], np.float32),
               obb_yaw=np.array([0.25, np.nan, np.nan]), obb_status=np.array([0, 2, 1], np.int32))
    pred, pseudo = kt.labels_of_frame(hb, res, 0, lifting.ClassTable.nuscenes(), lifting.SHAPE_PRIORS_CHATGPT, obb="device")
    assert len(pred) == 2 and len(pseudo) == 2                     # the third mask has 2 points: skipped (:1479-1480)
    assert pred[0].split()[14] == "0.25" and pred[1].split()[14] == "0.0"
    assert pseudo[0].rstrip("\n").split()[-1] == "0.25"
    with pytest.raises(ValueError):
        kt.labels_of_frame(hb, res, 0, lifting.ClassTable.nuscenes(), lifting.SHAPE_PRIORS_CHATGPT, obb="gpu")


def test_labels_of_frame_device_mode_fits_unfitted_masks_on_the_host():
    """A mask the device could not fit (status 4) gets the host fit from res["hit_xyz"] when the points are there, and a clear error
    when they are not."""
    from types import SimpleNamespace
    from cm3d_amd import kitti as kt, lifting
    rng = np.random.default_rng(6)
    pts = np.zeros((40, 4), np.float32)
    pts[:, :3] = rng.normal(size=(40, 3)) * [3.0, 1.0, 0.5]
    hb = SimpleNamespace(mask_off=np.array([0, 2]), labels=[["car", "car"]], score=np.array([0.9, 0.8]))
    res = dict(hit_off=np.array([0, 20, 40]), centroid=np.zeros((2, 3), np.float32), obb_yaw=np.array([0.5, np.nan]),
               obb_status=np.array([0, kt.OBB_OVERFLOW], np.int32), hit_xyz=pts)
    pred, _ = kt.labels_of_frame(hb, res, 0, lifting.ClassTable.nuscenes(), lifting.SHAPE_PRIORS_CHATGPT, obb="device")
    assert pred[0].split()[14] == "0.5" and pred[1].split()[14] == repr(kt.obb_yaw(pts[20:40, :3]))
    del res["hit_xyz"]
    with pytest.raises(RuntimeError, match="--obb host"):
        kt.labels_of_frame(hb, res, 0, lifting.ClassTable.nuscenes(), lifting.SHAPE_PRIORS_CHATGPT, obb="device")
