"""The view wedges on each camera's mask-column hull, on the CPU (tests/wedge_hull_cases.py restates csrc/project.hip's
wedge_compose / wedge_setup / k_frame_tables in numpy): no point the exact chain can put into a mask's columns falls outside the
wedge, and the wedge is no wider than two pixels beyond the hull.  No GPU."""
import numpy as np
import pytest

from cm3d_amd import synthetic as syn
from tests import wedge_hull_cases as wh
from tests.magnitude_cases import H, W

MAGNITUDES = [0.0, 1700.0, 10000.0]
MIN_DIST = 2.3
N_PER_MASK = 400


def _rig(mag, index):
    cfg = syn.config("tiny", n_points=64, n_sweeps=1, n_masks=2, width=W, height=H, ratio=0.32, ego_magnitude=mag, point_order="firing")
    return syn.make_frame(cfg, 300 + index)


def _random_boxes(rng, n):
    """n eroded boxes (x0, y0, x1, y1) inside the image: narrow, wide, at the borders."""
    out = []
    for _ in range(n):
        w, h = int(rng.integers(1, 200)), int(rng.integers(1, 120))
        x0, y0 = int(rng.integers(1, W - 1 - w)), int(rng.integers(1, H - 1 - h))
        out.append((x0, y0, x0 + w - 1, y0 + h - 1))
    return out


def _points_in_columns(rng, rec, box, min_dist, n):
    """float32 global points whose composed image lies in the box's columns (the edges included), at depths min_dist .. 100 m."""
    x0, y0, x1, y1 = box
    u = np.concatenate([rng.uniform(x0, x1 + 1, n - 40), x0 + rng.uniform(0, 0.02, 20), x1 + 1 - rng.uniform(0, 0.02, 20)])
    v = rng.uniform(y0, y1 + 1, n)
    z = np.exp(rng.uniform(np.log(min_dist), np.log(100.0), n))
    z[:10] = min_dist + rng.uniform(0, 2e-3, 10)
    return wh.back_project(rec, u, v, z).astype(np.float32)


@pytest.mark.parametrize("mag", MAGNITUDES)
def test_no_point_of_a_masks_columns_is_outside_the_wedge(oracle, mag):
    rng = np.random.default_rng(int(mag) + 11)
    n_checked = n_hull = 0
    for index in range(4):
        fr = _rig(mag, index)
        for c, rec in enumerate(fr.cams):
            boxes = _random_boxes(rng, int(rng.integers(1, 4)))
            u_lo, u_hi = wh.camera_interval(rec, W, MIN_DIST, boxes)
            pad = wh.hull_pad(rec, W, MIN_DIST)
            assert pad is not None and pad >= wh.issue_pad_floor(rec, W, MIN_DIST)
            assert (u_lo, u_hi) == (max(min(b[0] for b in boxes) - pad, 0), min(max(b[2] for b in boxes) + 1 + pad, W))
            n_hull += (u_lo, u_hi) != (0, W)
            planes = wh.wedge_planes(rec, W, MIN_DIST, u_lo, u_hi)
            for box in boxes:
                P = _points_in_columns(rng, rec, box, MIN_DIST, N_PER_MASK)
                P4 = np.zeros((P.shape[0], 4), np.float32)               # (the oracle's cloud rows: x, y, z, intensity)
                P4[:, :3] = P
                uvz = oracle.project_points(P4, rec)                      # the exact chain's float32 pixel and depth
                iu = np.floor(uvz[:, 0])
                inside = (iu >= box[0]) & (iu <= box[2]) & (uvz[:, 2] > np.float32(MIN_DIST))
                assert inside.sum() > N_PER_MASK // 2
                m = wh.wedge_min(planes, P[inside])
                assert (m >= 0).all(), (mag, index, c, box, float(m.min()))
                n_checked += int(inside.sum())
    assert n_checked > 10000 and n_hull > 12


@pytest.mark.parametrize("mag", MAGNITUDES)
def test_the_wedge_ends_within_two_pixels_of_the_hull(mag):
    rng = np.random.default_rng(int(mag) + 12)
    sides = 0
    for index in range(4):
        fr = _rig(mag, index)
        for rec in fr.cams:
            boxes = _random_boxes(rng, 2)
            u_lo, u_hi = wh.camera_interval(rec, W, MIN_DIST, boxes)
            planes = wh.wedge_planes(rec, W, MIN_DIST, u_lo, u_hi)
            v = rng.uniform(2, H - 2, 8)
            z = np.full(8, 20.0)
            for u_out, u_in, open_side in ((u_lo - 2.0, u_lo + 0.5, u_lo > 0), (u_hi + 2.0, u_hi - 0.5, u_hi < W)):
                if not open_side:                   # clamped to the image: that side is the image's plane
                    continue
                out = wh.wedge_min(planes, wh.back_project(rec, np.full(8, u_out), v, z).astype(np.float32))
                ins = wh.wedge_min(planes, wh.back_project(rec, np.full(8, u_in), v, z).astype(np.float32))
                assert (out < 0).all() and (ins >= 0).all(), (mag, index, u_lo, u_hi, out, ins)
                sides += 1
    assert sides > 20


def test_the_image_interval_gives_the_image_wedge():
    """u_lo = 0, u_hi = W is the wedge of the whole image: what a camera without a bound or without a non-empty mask keeps."""
    fr = _rig(1700.0, 0)
    rec = fr.cams[0]
    assert wh.camera_interval(rec, W, MIN_DIST, []) == (0, W)
    assert wh.camera_interval(rec, W, MIN_DIST, [(5, 5, 4, 9)]) == (0, W)                   # empty after the erosion
    planes = wh.wedge_planes(rec, W, MIN_DIST, 0, W)
    P_in = wh.back_project(rec, np.array([0.5, W - 0.5]), np.array([50.0, 60.0]), np.array([20.0, 20.0])).astype(np.float32)
    P_out = wh.back_project(rec, np.array([-2.0, W + 2.0]), np.array([50.0, 60.0]), np.array([20.0, 20.0])).astype(np.float32)
    assert (wh.wedge_min(planes, P_in) >= 0).all() and (wh.wedge_min(planes, P_out) < 0).all()


def test_no_bound_no_hull():
    """zmin <= 0.1 (a small minimum depth far from the origin) and a composition that is no rotation to 1e-5 keep the image."""
    from tests import camera_cases as cc
    fr = _rig(10000.0, 1)
    assert wh.hull_pad(fr.cams[0], W, 1.0) is None and wh.camera_interval(fr.cams[0], W, 1.0, [(100, 50, 140, 90)]) == (0, W)
    near = cc.near_rot(_rig(1700.0, 1).cams[2])
    assert wh.hull_pad(near, W, MIN_DIST) is None and (wh.wedge_planes(near, W, MIN_DIST, 0, W)[:3] != 0).any()
    skew = cc.skew(_rig(1700.0, 1).cams[2])
    assert wh.hull_pad(skew, W, MIN_DIST) is None and np.array_equal(wh.wedge_planes(skew, W, MIN_DIST, 0, W), [0, 0, 0, 1, 0, 0, 0, 1])
