"""GPU parity on the cameras the projection's culling does NOT cover (tests/camera_cases.py).  csrc/project.hip wedge_setup
derives a view wedge, an approximate projection and a depth bound per camera and switches them off one by one for a record
outside its derivation (skew, a non-trivial third row of K, stages that are no rotation, a long focal length, a small minimum
depth); the kernels then take branches no nuScenes-, Waymo- or KITTI-shaped record reaches: no pre-test, per-camera bit masks
that differ inside a frame, the run-time stage layout, the IEEE division behind `redo`, the eighth camera slot.

Every case: the whole path against the oracle (index lists, in-mask coordinates, medoids, boxes), and the culling decisions
the device took (LiftEngine.culling) against their numpy restatement -- which is what ties a run to the branch it was built
for.  tests/test_camera_cases_host.py proves on the CPU that the crafted rows of every case fall on both sides of every limit."""
import functools

import numpy as np
import pytest

from cm3d_amd import rle as rlemod, synthetic as syn
from tests import camera_cases as cc
from tests.helpers import oracle_batch
from tests.magnitude_cases import H, W
from tests.test_camera_cases_host import culling_gates          # noqa: F401  (frame_gates applies it per camera)
from tests.test_gpu_parity import _compare

pytestmark = pytest.mark.gpu
both_layouts = pytest.mark.parametrize("raw_layout", ["quads", "rows"], indirect=True)


def _lanes(frames):
    return [syn.make_lane_table(frames[0].ego_xyz[:2], 3000, seed=1)]


@functools.lru_cache(maxsize=None)
def _case(kind, arg, min_dist=None):
    """(frames, lane tables, the oracle's results) of one case: built once, shared by both layouts, never written to."""
    from oracle import oracle as orc
    from cm3d_amd import lifting
    orc.lib()
    if kind == "class":
        frames = cc.class_frames(arg, **({} if min_dist is None else {"min_dist": min_dist}))[0]
    elif kind == "cams":
        frames = cc.class_frames("covered", n_cams=arg)[0]
    else:
        frames = cc.mixed_frames(arg)[0]
    lanes = _lanes(frames)
    oframes, bad = cc.oracle_view(frames)
    hb = lifting.pack_frames(oframes, lanes, [0] * len(frames), layout="rows")
    exp = oracle_batch(orc, oframes, lanes, [0] * len(frames), hb, min_dist=min_dist)
    m = 0
    for fr in frames:                       # a mask of an out-of-range camera keeps its own bounding box (and gets no points)
        for k, rl in enumerate(fr.rles):
            if m + k in bad:
                ys, xs = np.nonzero(orc.erode3x3(orc.rle_decode(rl).T))
                exp["bbox"][m + k] = [xs.min(), ys.min(), xs.max(), ys.max()]
        m += len(fr.rles)
    for v in exp.values():
        v.setflags(write=False)
    return frames, lanes, exp, bad


def _whole_image_masks(frames):
    whole = cc._whole_rle(W, H)["counts"]
    return np.array([rl["counts"] == whole for fr in frames for rl in fr.rles])


def _assert_not_vacuous(frames, exp, bad=()):
    """The oracle's whole-image list of every camera with masks holds points."""
    whole = _whole_image_masks(frames)
    n_has = sum(len(set(c for c in fr.cam_nums if 0 <= c < fr.cams.shape[0])) for fr in frames)
    assert int(whole.sum()) == n_has
    assert (np.diff(exp["hit_off"])[whole] > 0).all()
    for k in bad:
        assert exp["hit_off"][k + 1] == exp["hit_off"][k]


def _assert_culling(eng, frames, min_dist):
    got = eng.culling()
    for f, fr in enumerate(frames):
        want = cc.frame_gates(fr, min_dist)
        for key in ("apx_ok", "cam_has", "wedge", "margin_px"):
            assert int(got[key][f]) == int(want[key]), (f, key, int(got[key][f]), int(want[key]))
        assert abs(float(got["zmin"][f]) - float(want["zmin"])) <= 1e-6
    return got


def _lift(case, layout, min_dist=2.3, keep_cloud=False, fused=True, real_cams=False):
    import torch
    from cm3d_amd import lifting
    frames, lanes, exp, bad = case
    hb = lifting.pack_frames(frames, lanes, [0] * len(frames), layout=layout)
    eng = lifting.LiftEngine(keep_colsum=True, keep_cloud=keep_cloud, min_dist=min_dist)
    eng.fused_sweeps = fused
    real = hb.mask_cam.copy()
    if bad:                                  # upload() refuses such a batch: hand it a valid one, then put the real camera numbers back
        hb.mask_cam[bad] = 0
    eng.upload(hb)
    if bad:
        eng.b.mask_cam.copy_(torch.from_numpy(real))
    assert eng.b.fused == fused
    eng.run(masks="rle")
    torch.cuda.synchronize()
    return hb, eng


def _run_and_compare(case, layout, min_dist=2.3, **kw):
    frames, _, exp, _ = case
    _assert_not_vacuous(frames, exp)
    hb, eng = _lift(case, layout, min_dist, **kw)
    got = eng.download()
    assert ("points" in got) == bool(kw.get("keep_cloud") or not kw.get("fused", True))
    _compare(hb, got, exp)
    return eng, _assert_culling(eng, frames, min_dist)


@both_layouts
@pytest.mark.parametrize("name", sorted(cc.CLASSES))
def test_one_class_on_every_camera(raw_layout, name):
    """Uniform frames.  (The rows layout also keeps the cloud and compares it; the quad layout re-derives the in-mask coordinates
    from the raw rows, the product's default.)"""
    eng, cul = _run_and_compare(_case("class", name), raw_layout, keep_cloud=raw_layout == "rows")
    wedge, apx = cc.CLASSES[name][2]
    assert (cul["wedge"] == (0x3F if wedge else 0)).all() and (cul["apx_ok"] == (0x3F if apx else 0)).all()
    assert (cul["cam_has"] == 0x3F).all() and eng.b.planes == 1


@both_layouts
@pytest.mark.parametrize("variant", ["plain", "many", "garbage"])
def test_frames_whose_cameras_differ(raw_layout, variant):
    """covered, skew, shear, near_rot, k_tiny, covered in ONE frame, camera 3 without a mask: the per-camera bit masks of the frame
    table differ.  many: three hit-word planes (the multi-plane kernel), more than 32 masks on a camera without a wedge and on one
    with.  garbage: NaN, infinite, 1e6 m and denormal rows among the ordinary ones."""
    eng, cul = _run_and_compare(_case("mixed", variant), raw_layout, keep_cloud=variant == "garbage")
    assert (cul["wedge"] == 0b101001).all() and (cul["apx_ok"] == 0b100001).all() and (cul["cam_has"] == 0b110111).all()
    assert eng.b.planes == (3 if variant == "many" else 1)


@both_layouts
def test_frames_whose_cameras_differ_on_the_prepared_cloud(raw_layout):
    """The same frames through the separate sweep and projection launches (the kernels' variant for a prepared cloud)."""
    _run_and_compare(_case("mixed", "plain"), raw_layout, fused=False)


@both_layouts
def test_a_mask_of_a_camera_that_does_not_exist(raw_layout):
    """One mask per frame names camera n_cams: it gets no points, every other mask the oracle's, and status bit 2 says so (which is
    why download() raises on such a batch)."""
    from cm3d_amd import _lib
    case = _case("mixed", "bad_cam")
    frames, _, exp, bad = case
    assert len(bad) == len(frames)
    _assert_not_vacuous(frames, exp, bad)
    hb, eng = _lift(case, raw_layout)
    status = eng.b.status.cpu().numpy()
    assert status[0] & 4 and not status[0] & ~4
    with pytest.raises(_lib.Cm3dError):
        eng.download()
    eng.check_status = lambda: status                    # the results behind the refusal
    _compare(hb, eng.download(), exp)
    _assert_culling(eng, frames, 2.3)


@both_layouts
@pytest.mark.parametrize("n_cams", [1, 7, 8])
def test_camera_counts_up_to_the_last_slot(raw_layout, n_cams):
    """1, 7 and CM3D_MAX_CAMS = 8 cameras, masks on every one of them, the last included."""
    eng, cul = _run_and_compare(_case("cams", n_cams), raw_layout)
    full = (1 << n_cams) - 1
    assert (cul["wedge"] == full).all() and (cul["apx_ok"] == full).all() and (cul["cam_has"] == full).all()


@both_layouts
@pytest.mark.parametrize("which", range(4))
def test_minimum_depths(raw_layout, which):
    """min_dist just below and just above the value at which zmin crosses 0.1 (approximate projection off / on), 1.0 and 5.0: the
    depth test, the margin and -- through LiftEngine -- the ego box all move with it.  Crafted rows sit at min_dist +- dz."""
    md = cc.min_dist_values()[which]
    eng, cul = _run_and_compare(_case("class", "covered", md), raw_layout, min_dist=md)
    assert (cul["wedge"] == 0x3F).all() and (cul["apx_ok"] == (0 if which == 0 else 0x3F)).all()


@pytest.mark.parametrize("which", range(4))
def test_minimum_depths_through_the_single_frame_call(oracle, which):
    """ops.points_in_masks(..., min_dist=...): one frame, a prepared cloud, the unfused projection launch."""
    from cm3d_amd import ops
    md = cc.min_dist_values()[which]
    fr = _case("class", "covered", md)[0][0]
    P = cc.frame_cloud(oracle, fr, md)
    packed, bbox = ops.erode_rle([rlemod.string_to_counts(r["counts"]) for r in fr.rles], W, H)
    got = ops.points_in_masks(P, fr.cams, packed, bbox, fr.cam_nums, W, H, min_dist=md)
    n = 0
    for k, (rl, c) in enumerate(zip(fr.rles, fr.cam_nums)):
        want = oracle.points_in_mask(P, fr.cams[c], oracle.erode3x3(oracle.rle_decode(rl).T), np.float32(md))
        assert np.array_equal(got[k], want), (md, k)
        n += want.size
    assert n > 500
