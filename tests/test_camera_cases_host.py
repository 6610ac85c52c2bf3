"""CPU: the camera cases of tests/camera_cases.py reach the branches they are built for, and mean something.
  * `culling_gates` (a numpy restatement of csrc/project.hip wedge_setup's decisions) puts every class where the table of
    tests/camera_cases.CLASSES says: view wedge on / off, approximate projection on / off;
  * the oracle puts a fair share of every crafted kind on each side of its limit, for every class and minimum depth;
  * the classes that only re-express the control's arithmetic give its lists bit for bit, the ones that change the map do not;
  * no garbage row is listed, except the far ones, which are.
tests/test_gpu_camera_cases.py runs the same frames on the GPU and ties the run to the gates through cm3d_project_culling."""
import numpy as np
import pytest

from tests import camera_cases as cc
from tests.camera_cases import culling_gates            # noqa: F401  (the restatement; the GPU tests import it from here)
from tests.magnitude_cases import H, N_EACH, N_KINDS, W

LOW = 3           # at least LOW and at most N_EACH - LOW of the N_EACH crafted rows of a (camera, kind) fall inside


@pytest.mark.parametrize("name", sorted(cc.CLASSES))
def test_every_class_reaches_its_gates(name):
    frames, _ = cc.class_frames(name)
    want_wedge, want_apx = cc.CLASSES[name][2]
    for fr in frames:
        for rec in fr.cams:
            g = culling_gates(rec, W, H, 2.3)
            assert (g["wedge"], g["apx"]) == (want_wedge, want_apx), (name, g)
            if name in ("skew", "krow3", "k_tiny", "k_huge"):
                assert not g["plain"] and g["dev"] < 1e-5
            elif name == "shear":
                assert g["plain"] and g["dev"] >= 1e-3
            elif name == "near_rot":
                assert g["plain"] and 1e-5 <= g["dev"] < 1e-3
            elif name == "tele":        # the margin alone switches the approximate projection off
                assert g["plain"] and g["dev"] < 1e-5 and g["zmin"] > 0.1
                delta = 1e-6 * float(g["omax"]) + 1e-4
                assert 1 + np.ceil(2 * 5000.0 * delta / float(g["zmin"])) >= 64
            else:
                assert g["plain"] and g["dev"] < 1e-5 and g["zmin"] > 0.1 and 0 < g["margin_px"] < 64
            if name.startswith("stages_"):
                assert (int(rec[54]), int(rec[55])) == tuple(int(v) for v in name.split("_")[1:])
                assert (int(rec[54]), int(rec[55])) not in ((2, 5), (1, 1), (3, 10))          # the run-time stage layout


def test_k_scaled_classes_force_the_ieee_division():
    """Every point the depth test accepts has zh = K[8] * depth outside [1e-30, 1e30): project_quad's `redo` branch."""
    for name, lo in (("k_tiny", True), ("k_huge", False)):
        frames, _ = cc.class_frames(name, n_frames=1)
        k8 = float(frames[0].cams[0][cc.CAM_K + 8])
        assert (k8 * 1000.0 < 1e-30) if lo else (k8 * 2.3 > 1e30)          # depths lie in (2.3, 1000) m


def test_min_dist_values_straddle_the_depth_gate():
    lo, hi = cc.straddling_min_dists()
    assert 0.2 < lo < hi < 0.45 and hi - lo < 0.08
    for md, want_apx in ((lo, False), (hi, True), (1.0, True), (5.0, True)):
        frames, _ = cc.class_frames("covered", min_dist=md)
        for fr in frames:
            fg = cc.frame_gates(fr, md)
            assert fg["wedge"] == 0x3F and fg["apx_ok"] == (0x3F if want_apx else 0), (md, fg)
            assert (fg["zmin"] > 0.1) == want_apx
    assert cc.frame_gates(cc.class_frames("covered", min_dist=1.0, n_frames=1)[0][0], 1.0)["margin_px"] == 3


def test_mixed_frame_differs_per_camera():
    frames, _, _ = cc.mixed_frames("plain")
    for fr in frames:
        fg = cc.frame_gates(fr, 2.3)
        assert fg["wedge"] == 0b101001 and fg["apx_ok"] == 0b100001 and fg["cam_has"] == 0b110111
    many = cc.mixed_frames("many", n_frames=1)[0][0]
    assert len(many.rles) > 64 and many.cam_nums.count(1) >= 40 and many.cam_nums.count(0) >= 33
    bad = cc.mixed_frames("bad_cam", n_frames=1)[0][0]
    assert bad.cam_nums[-1] == bad.cams.shape[0]


def _assert_both_sides(oracle, frames, crafted, min_dist, what):
    for fr, rows in zip(frames, crafted):
        inside = cc.crafted_sides(oracle, fr, rows, min_dist)
        assert LOW <= inside.min() and inside.max() <= N_EACH - LOW, (what, inside.tolist())
        # the real run's ego box (half width f32(sqrt(min_dist))) drops no crafted row: they all reach the projection
        x = fr.sweep_xf[0]
        kept = oracle.sweep_prep(rows, x[0:9], x[9:12], x[12:21], x[21:24], np.float32(np.sqrt(min_dist)))
        assert kept.shape[0] == rows.shape[0]


@pytest.mark.parametrize("name", sorted(cc.CLASSES))
def test_crafted_rows_fall_on_both_sides_for_every_class(oracle, name):
    frames, crafted = cc.class_frames(name)
    _assert_both_sides(oracle, frames, crafted, 2.3, name)


@pytest.mark.parametrize("which", range(4))
def test_crafted_rows_fall_on_both_sides_for_every_min_dist(oracle, which):
    md = cc.min_dist_values()[which]
    frames, crafted = cc.class_frames("covered", min_dist=md)
    _assert_both_sides(oracle, frames, crafted, md, md)


@pytest.mark.parametrize("n_cams", [1, 7, 8])
def test_crafted_rows_fall_on_both_sides_for_every_camera_count(oracle, n_cams):
    frames, crafted = cc.class_frames("covered", n_cams=n_cams)
    assert frames[0].cams.shape[0] == n_cams and set(frames[0].cam_nums) == set(range(n_cams))
    _assert_both_sides(oracle, frames, crafted, 2.3, n_cams)


def test_crafted_rows_fall_on_both_sides_in_the_mixed_frame(oracle):
    frames, crafted, _ = cc.mixed_frames("plain")
    _assert_both_sides(oracle, frames, crafted, 2.3, "mixed")


def _lists(oracle, P, cams):
    full, rect = cc.eroded_masks(oracle)
    return [oracle.points_in_mask(P, cam, m) for cam in cams for m in (full, rect)]


@pytest.mark.parametrize("name", sorted(set(cc.CLASSES) - {"covered", "tele", "near_rot"}))
def test_lists_against_the_control(oracle, name):
    """On the SAME points: a K scaled by a power of two, an identity stage and zero or moved translations leave every float32
    operation of the chain as it was -- the control's lists bit for bit; skew, a third row of K and a shear do not."""
    frames, _ = cc.class_frames(name)
    same = differ = 0
    for fr in frames:
        P = cc.frame_cloud(oracle, fr, 2.3)
        got, ctl = _lists(oracle, P, fr.cams), _lists(oracle, P, fr.meta["base_cams"])
        assert all(l.size > 0 for l in ctl[0::2])
        if name in cc.SAME_AS_CONTROL:
            assert all(np.array_equal(a, b) for a, b in zip(got, ctl)), name
        elif name in cc.DIFFERENT_FROM_CONTROL:
            assert all(l.size > 0 for l in got[0::2])
            assert all(not np.array_equal(a, b) for a, b in zip(got[0::2], ctl[0::2])), name
        else:
            # stages_1_3 composes the two rotations into one float32 matrix: the same map, another rounding.  Its lists can only
            # differ from the control's in points within that rounding of a limit (the crafted rows are): a few per cent at most.
            assert name == "stages_1_3"
            for a, b in zip(got, ctl):
                same += np.intersect1d(a, b).size
                differ += np.setxor1d(a, b).size
    if name == "stages_1_3":
        assert same > 1000 and differ < 0.05 * same, (same, differ)


def test_garbage_rows(oracle):
    """No NaN, infinite or denormal row is in any list; the rows 1e6 m down an optical axis are in that camera's whole-image list."""
    frames, _, garbage = cc.mixed_frames("garbage")
    for fr, g in zip(frames, garbage):
        assert g.shape == (20, 5)
        P = cc.frame_cloud(oracle, fr, 2.3)
        gi = np.flatnonzero(P[:, 3] >= 1000.0)                        # garbage rows of the cloud; their number in `g`:
        num = (P[gi, 3] - 1000.0).astype(int)
        assert sorted(num.tolist()) == list(range(16))                # the four denormal rows (16..19) fall to the ego box
        assert not np.isfinite(P[gi[num < 12], :3]).all(1).any() and np.abs(P[gi[num >= 12], :3]).max(1).min() > 5e5
        lists = _lists(oracle, P, fr.cams)
        listed = np.zeros(P.shape[0], bool)
        for l in lists:
            listed[l] = True
        assert not listed[gi[num < 12]].any()
        for j, c in enumerate(cc.GARBAGE_FAR_CAMS):
            assert gi[num == 12 + j][0] in lists[2 * c], (j, c)


def test_culling_read_back_validates_its_arguments():
    """cm3d_project_culling without a workspace or an output returns an error code and touches no device."""
    from cm3d_amd import _lib
    L = _lib.lib()
    out = np.zeros(8, np.int32)
    assert L.cm3d_project_culling(0, 0, 1, 256, 1, out.ctypes.data, 0) == -1
    assert L.cm3d_project_culling(out.ctypes.data, 32, 1, 256, 1, 0, 0) == -1
    assert L.cm3d_project_culling(out.ctypes.data, 32, 0, 256, 1, out.ctypes.data, 0) == -1
    assert L.cm3d_project_culling(out.ctypes.data, 32, 1, 256, 1, out.ctypes.data, 0) == -3          # too small a workspace
    assert not out.any()


def test_magnitude_cases_are_untouched():
    """tests/magnitude_cases.crafted_frames keeps its own `_craft`: the generalised builder never feeds it."""
    from tests import magnitude_cases as mc
    assert mc._craft.__module__ == "tests.magnitude_cases" and cc.craft_rows is not mc._craft
    assert (N_KINDS, N_EACH) == (10, 24)
