"""GPU: the view wedges stand on the hull of each camera's mask columns (csrc/project.hip k_frame_tables, wedge_setup).

Every case runs the whole path against the CPU oracle (index lists, in-mask coordinates, medoids, boxes: the wedge culls work,
never a result) and probes the planes the device wrote (LiftEngine.wedges) against the numpy restatement of tests/wedge_hull_cases.py:
inside at the hull's own first and last column, outside two pixels beyond the padded hull -- which ties the run to the branch.
Frames are `tiny`-sized (256 x 144), 2-3 per case, at most 2048 rows each."""
import functools

import numpy as np
import pytest

from cm3d_amd import synthetic as syn
from tests import camera_cases as cc
from tests import mixed_size_cases as X
from tests import wedge_hull_cases as wh
from tests.helpers import oracle_batch
from tests.magnitude_cases import _rect_rle
from tests.test_gpu_parity import _compare

pytestmark = pytest.mark.gpu

W, H = 256, 144
ACCEPT_ALL = np.array([0, 0, 0, 1, 0, 0, 0, 1], np.float32)
NOTHING = np.array([0, 0, 0, -1, 0, 0, 0, -1], np.float32)


# ---------------------------------------------------------------------------------------------------------------- frames
def _frames(n=3, first=500, **over):
    kw = dict(n_points=900, n_sweeps=2, point_order="firing")
    kw.update(over)
    cfg = syn.config("tiny", **kw)
    return [syn.make_frame(cfg, first + i) for i in range(n)]


def _set_masks(fr, masks):
    """masks: [(camera, (x0, y0, x1, y1) filled rectangle)]"""
    fr.rles = [_rect_rle(*r, fr.width, fr.height) for _, r in masks]
    fr.cam_nums = [int(c) for c, _ in masks]
    fr.labels = ["car" if k % 2 == 0 else "human" for k in range(len(masks))]
    fr.scores = [round(0.9 - 0.005 * k, 3) for k in range(len(masks))]


def _edge_rows(fr, masks, depths, fracs=(0.03, 0.5, 0.97)):
    """Rows back-projected in float64 through the columns bb.x - 1, bb.x, bb.z, bb.z + 1 of every rectangle's ERODED box, at the
    box's middle row and next to each column's two ends, at `depths`; appended to sweep 0."""
    rows = []
    for cam, r in masks:
        x0, y0, x1, y1 = wh.eroded_box(*r)
        if x1 < x0 or y1 < y0:
            continue
        for col in (x0 - 1, x0, x1, x1 + 1):
            for frac in fracs:
                for z in depths:
                    rows.append(wh.back_project(fr.cams[cam], [col + frac], [0.5 * (y0 + y1) + 0.5], [z]))
    if rows:
        fr.sweeps_raw[0] = np.ascontiguousarray(np.concatenate([fr.sweeps_raw[0], wh.to_sensor_rows(fr, np.concatenate(rows, 0))], 0))


def _many(n_masks):
    """n_masks small rectangles per frame on cameras 0, 2 and 5, each camera's inside a band of columns of its own."""
    band = {0: 10, 2: 90, 5: 150}
    out = []
    for k in range(n_masks):
        cam = (0, 2, 5)[k % 3]
        j = k // 3
        x0, y0 = band[cam] + 5 * (j % 8) + (40 if k >= 64 else 0), 20 + 22 * (j // 8)       # (masks 64.. widen their cameras' hulls)
        out.append((cam, (x0, y0, x0 + 14 + (j % 3), y0 + 18)))
    return out


def _build(case):
    """(frames, min_dist, classes or None, masks per frame or None)"""
    md, classes, per_frame = 2.3, None, None
    if case == "synthetic":
        frames = _frames()
    elif case == "edges":                       # eroded boxes at the image's first and last columns, and within the pad of them
        frames = _frames()
        per_frame = [[(0, (0, 30, 40, 90)), (1, (W - 41, 30, W - 1, 90)), (2, (1, 30, 40, 90)), (3, (W - 41, 30, W - 2, 90)),
                      (4, (100, 40, 140, 100))]] * 3
    elif case == "narrow":                      # 3 pixels wide: 1 column after the erosion
        md = 1.0
        frames = _frames()
        per_frame = [[(2, (120, 20, 122, 120)), (0, (60, 40, 110, 100))], [(2, (30, 20, 32, 120))], [(2, (200, 10, 202, 130)), (3, (10, 10, 12, 130))]]
    elif case == "opposite":                    # two masks at opposite edges of one camera: the hull is the whole image
        frames = _frames()
        per_frame = [[(0, (0, 30, 12, 110)), (0, (W - 13, 30, W - 1, 110)), (3, (100, 30, 130, 90))]] * 3
    elif case == "one_cam":
        frames = _frames()
        for fr in frames:
            fr.cam_nums = [3] * len(fr.cam_nums)
    elif case == "empty_cam":                   # camera 1's masks are all empty after the erosion
        frames = _frames()
        per_frame = [[(1, (50, 30, 51, 100)), (1, (90, 60, 140, 61)), (0, (80, 30, 150, 100)), (5, (20, 30, 70, 100))]] * 3
    elif case == "no_masks":                    # a frame with no mask at all between two ordinary ones
        frames = _frames()
        _set_masks(frames[1], [])
    elif case in ("m40", "m70"):
        frames = _frames(n=2, n_points=850)
        per_frame = [_many(int(case[1:]))] * 2
    elif case == "sweeps3":                     # sweep boundaries at rows 600 and 1200: inside wave-chunks 2 and 4
        frames = _frames(n_points=600, n_sweeps=3)
    elif case == "waymo":
        from cm3d_amd import lifting
        cfg = syn.config("tiny", n_cams=5, n_points=1000, n_sweeps=1)
        frames = [syn.make_waymo_frame(cfg, 20 + i) for i in range(3)]
        classes = lifting.ClassTable.waymo()
    elif case == "skew":
        frames = _frames()
        for fr in frames:
            fr.cams = np.stack([cc.skew(r) for r in fr.cams]).astype(np.float32)
    elif case == "mixed_sizes":                 # rule R: cameras 3 and 4 cropped to 256 x 100, one mask to 200 x 144
        cfg = syn.config("tiny", n_cams=5, n_points=1000, n_sweeps=2, point_order="firing")
        frames = []
        for i in range(3):
            fr = syn.make_frame(cfg, 700 + i)
            other = [k for k, c in enumerate(fr.cam_nums) if int(c) not in (3, 4)]
            frames.append(X.crop_frame(fr, {3: X.SIDE, 4: X.SIDE}, {other[0]: X.ODD} if other else None, ()))
    elif case in ("far", "far_no_bound"):       # 10 km from the origin; with min_dist 1.0 zmin <= 0.1: no bound, the image's wedge
        md = 2.3 if case == "far" else 1.0
        frames = _frames(ego_magnitude=10000.0)
    else:
        raise ValueError(case)
    if per_frame is not None:
        for fr, masks in zip(frames, per_frame):
            _set_masks(fr, masks)
            if len(masks) > 8:                  # (many masks: one row per column, so that a frame stays below 2048 rows)
                _edge_rows(fr, masks, (50.0,), (0.5,))
            else:
                _edge_rows(fr, masks, (md + 1e-3, 2.3, 50.0))
    return frames, md, classes, per_frame


def _lanes(frames):
    if getattr(frames[0], "pose", None) is not None:
        return [syn.make_lane_table(np.asarray(frames[0].pose).reshape(4, 4)[:2, 3], 3000, seed=4, extent=400.0)]
    return [syn.make_lane_table(frames[0].ego_xyz[:2], 3000, seed=1)]


@functools.lru_cache(maxsize=None)
def _case(case, stride=5):
    """Built once, shared by the layouts, never written to: (frames, lanes, min_dist, classes, masks per frame, oracle's results)."""
    from oracle import oracle as orc
    from cm3d_amd import lifting
    orc.lib()
    frames, md, classes, per_frame = _build(case)
    if stride == 4:
        for fr in frames:
            fr.sweeps_raw = [np.ascontiguousarray(r[:, :4]) for r in fr.sweeps_raw]
    lanes = _lanes(frames)
    hb = lifting.pack_frames(frames, lanes, [0] * len(frames), classes, layout="rows")
    exp = oracle_batch(orc, frames, lanes, [0] * len(frames), hb, min_dist=None if classes is not None else md)
    if case == "mixed_sizes":                   # rule R: a cropped mask loses its own last row / column on the canvas
        from tests.test_gpu_mixed_sizes import _rule_r_bbox
        exp["bbox"] = _rule_r_bbox(orc, frames, hb.width, hb.height)
    for v in exp.values():
        v.setflags(write=False)
    return frames, lanes, md, classes, per_frame, exp


# ---------------------------------------------------------------------------------------------------------------- the run
def _lift(case, layout="quads", fused=True, stride=5):
    import torch
    from cm3d_amd import lifting
    frames, lanes, md, classes, per_frame, exp = _case(case, stride)
    assert max(sum(r.shape[0] for r in fr.sweeps_raw) for fr in frames) <= 2048
    hb = lifting.pack_frames(frames, lanes, [0] * len(frames), classes, layout=layout)
    kw = {} if classes is None else {"classes": classes}
    eng = lifting.LiftEngine(keep_colsum=True, **({} if classes is not None else {"min_dist": md}), **kw)
    eng.fused_sweeps = fused
    eng.upload(hb)
    assert eng.b.fused == fused
    eng.run(masks="rle")
    torch.cuda.synchronize()
    got = eng.download()
    _compare(hb, got, exp)
    return hb, eng, exp


def _probe(rec, planes, u, n=4):
    v = np.linspace(0.25 * H, 0.75 * H, n)
    return wh.wedge_min(planes, wh.back_project(rec, np.full(n, float(u)), v, np.full(n, 20.0)).astype(np.float32))


def _assert_wedges(case, hb, eng, exp):
    """The planes of every camera of every frame: on the restated interval, probed inside and outside."""
    frames, _, md, classes, _, _ = _case(case)
    md = float(eng.min_dist)
    got = eng.wedges()
    Wc = hb.width
    assert got.shape == (len(frames), 8, 8)
    n_hull = 0
    for f, fr in enumerate(frames):
        m0, m1 = int(hb.mask_off[f]), int(hb.mask_off[f + 1])
        for c in range(8):
            if c >= fr.cams.shape[0]:
                assert np.array_equal(got[f, c], NOTHING), (f, c, got[f, c])
                continue
            rec = fr.cams[c]
            boxes = [tuple(int(x) for x in exp["bbox"][m]) for m in range(m0, m1) if int(hb.mask_cam[m]) == c]
            u_lo, u_hi = wh.camera_interval(rec, Wc, md, boxes)
            want = wh.wedge_planes(rec, Wc, md, u_lo, u_hi)
            if np.array_equal(want, ACCEPT_ALL):
                assert np.array_equal(got[f, c], ACCEPT_ALL), (f, c, got[f, c])
                continue
            assert np.allclose(got[f, c, [0, 1, 2, 4, 5, 6]], want[[0, 1, 2, 4, 5, 6]], rtol=0, atol=1e-5), (f, c, got[f, c], want)
            live = [b for b in boxes if b[2] >= b[0] and b[3] >= b[1]]
            hull = (u_lo, u_hi) != (0, Wc)
            n_hull += hull
            in_lo, in_hi = (min(b[0] for b in live) + 0.5, max(b[2] for b in live) + 0.5) if hull else (0.5, Wc - 0.5)
            for u in (in_lo, in_hi):
                assert (_probe(rec, got[f, c], u) >= 0).all(), (f, c, u, u_lo, u_hi)
            for u in (u_lo - 2.0, u_hi + 2.0):           # hull: its own first column - pad - 2, last + 1 + pad + 2; else the image's
                assert (_probe(rec, got[f, c], u) < 0).all(), (f, c, u, u_lo, u_hi)
    return got, n_hull


def _run(case, **kw):
    hb, eng, exp = _lift(case, **kw)
    got, n_hull = _assert_wedges(case, hb, eng, exp)
    return hb, eng, exp, got, n_hull


def _intervals(case, hb, exp):
    frames, _, md, _, _, _ = _case(case)
    out = {}
    for f, fr in enumerate(frames):
        for c in range(fr.cams.shape[0]):
            boxes = [tuple(int(x) for x in exp["bbox"][m]) for m in range(int(hb.mask_off[f]), int(hb.mask_off[f + 1])) if int(hb.mask_cam[m]) == c]
            out[f, c] = wh.camera_interval(fr.cams[c], hb.width, md, boxes)
    return out


# ---------------------------------------------------------------------------------------------------------------- the cases
def test_boxes_that_touch_the_image_clamp_the_hull():
    """The hull clamps to the image, and that side's plane is the image's.  (The erosion takes pixels outside the image as set, so
    an eroded box that reaches column 1 reaches column 0 too: no box STARTS at column 1 or ENDS at column W - 2.  Cameras 0 and 1
    have boxes from column 0 and up to column W - 1, cameras 2 and 3 boxes from column 2 and up to column W - 3, which the pad of 2
    pixels takes to the image's edge exactly.)"""
    hb, eng, exp, got, n_hull = _run("edges")
    iv = _intervals("edges", hb, exp)
    frames, _, md = _case("edges")[:3]
    for f, fr in enumerate(frames):
        cols = [tuple(int(x) for x in exp["bbox"][hb.mask_off[f] + k][[0, 2]]) for k in range(4)]
        assert cols == [(0, 39), (W - 40, W - 1), (2, 39), (W - 40, W - 3)]
        assert all(wh.hull_pad(fr.cams[c], W, md) == 2 for c in range(4))
        assert iv[f, 0] == (0, 42) and iv[f, 1] == (W - 42, W) and iv[f, 2] == (0, 42) and iv[f, 3] == (W - 42, W)
        image = [wh.wedge_planes(fr.cams[c], W, md, 0, W) for c in range(4)]
        for c, side in ((0, 0), (2, 0), (1, 4), (3, 4)):            # the clamped side: the image's plane; the other: not
            assert np.allclose(got[f, c, side:side + 3], image[c][side:side + 3], rtol=0, atol=1e-6)
            assert not np.allclose(got[f, c, 4 - side:7 - side], image[c][4 - side:7 - side], rtol=0, atol=1e-3)
    assert n_hull == 15 and exp["hit_idx"].size > 50


def test_a_mask_one_column_wide():
    """A 3-pixel mask is one column after the erosion; rows through bb.x - 1, bb.x, bb.z, bb.z + 1 at min_dist + 1e-3, 2.3 and 50 m."""
    hb, eng, exp, got, n_hull = _run("narrow")
    iv = _intervals("narrow", hb, exp)
    pad = wh.hull_pad(_case("narrow")[0][1].cams[2], W, 1.0)
    assert iv[1, 2] == (31 - pad, 32 + pad)
    cnt = np.diff(exp["hit_off"])
    assert (cnt[[0, 2, 3, 4]] >= 6).all()               # the crafted rows of column bb.x = bb.z are in the oracle's lists
    assert n_hull == 5


def test_masks_at_opposite_edges_give_the_whole_image():
    hb, eng, exp, got, n_hull = _run("opposite")
    iv = _intervals("opposite", hb, exp)
    assert all(iv[f, 0] == (0, W) for f in range(3)) and n_hull == 3         # (camera 3 has a hull)


def test_all_masks_on_one_camera():
    hb, eng, exp, got, n_hull = _run("one_cam")
    assert (eng.culling()["cam_has"] == 1 << 3).all() and exp["hit_idx"].size > 20


def test_a_camera_whose_masks_are_all_empty():
    hb, eng, exp, got, n_hull = _run("empty_cam")
    iv = _intervals("empty_cam", hb, exp)
    assert (eng.culling()["cam_has"] == 0b100001).all() and all(iv[f, 1] == (0, W) for f in range(3)) and n_hull == 6


def test_a_frame_without_masks():
    hb, eng, exp, got, n_hull = _run("no_masks")
    assert hb.mask_off[1] == hb.mask_off[2] and eng.culling()["cam_has"][1] == 0 and n_hull > 0
    for c in range(6):                              # every camera of the empty frame keeps the image's wedge
        assert (_probe(_case("no_masks")[0][1].cams[c], got[1, c], 0.5) >= 0).all()


@pytest.mark.parametrize("n_masks", [40, 70])
def test_many_masks_per_frame(n_masks):
    """40: two hit-word planes (the multi-plane k_project_hits).  70: the table kernel's second round of mask loads."""
    hb, eng, exp, got, n_hull = _run(f"m{n_masks}")
    assert eng.b.planes == (n_masks + 31) // 32 and n_hull == 6 and exp["hit_idx"].size > 100
    iv = _intervals(f"m{n_masks}", hb, exp)
    assert all(hi - lo < 120 for lo, hi in (iv[0, 0], iv[0, 2], iv[0, 5]))
    if n_masks == 70:                                # masks 64.. widen their cameras' hulls: only the second round sees them
        for c in (0, 2, 5):
            first64 = wh.camera_interval(_case("m70")[0][0].cams[c], W, 2.3, [wh.eroded_box(*r) for cam, r in _many(64) if cam == c])
            assert first64[0] == iv[0, c][0] and first64[1] + 30 < iv[0, c][1]


@pytest.mark.parametrize("layout, stride, fused", [("quads", 5, True), ("rows", 5, True), ("rows", 4, True), ("rows", 5, False), ("quads", 5, False)])
def test_raw_row_layouts(layout, stride, fused):
    """Quads, rows of stride 5 and of stride 4, and the prepared cloud through cm3d_project_hits."""
    hb, eng, exp, got, n_hull = _run("synthetic", layout=layout, stride=stride, fused=fused)
    assert n_hull >= 6 and exp["hit_idx"].size > 20
    if layout == "rows":
        assert hb.raw_stride == stride


def test_a_sweep_boundary_inside_a_chunk():
    hb, eng, exp, got, n_hull = _run("sweeps3")
    assert int(np.diff(hb.frame_sweep_off).max()) == 3 and n_hull >= 6


def test_a_single_stage_camera():
    hb, eng, exp, got, n_hull = _run("waymo")
    assert hb.pose_rt is not None and int(_case("waymo")[0][0].cams[0][54]) == 1 and n_hull >= 5


def test_a_skewed_camera_accepts_everything():
    hb, eng, exp, got, n_hull = _run("skew")
    cul = eng.culling()
    assert n_hull == 0 and (got[:, :6] == ACCEPT_ALL).all() and (cul["wedge"] == 0).all() and (cul["apx_ok"] == 0).all()


def test_mixed_mask_sizes_in_one_batch():
    hb, eng, exp, got, n_hull = _run("mixed_sizes")
    assert hb.mask_wh is not None and n_hull >= 5


@pytest.mark.parametrize("case", ["far", "far_no_bound"])
def test_ten_kilometres_from_the_origin(case):
    hb, eng, exp, got, n_hull = _run(case)
    if case == "far":
        assert n_hull >= 6
    else:
        assert n_hull == 0 and (eng.culling()["apx_ok"] == 0).all() and (eng.culling()["wedge"] == 0x3F).all()
