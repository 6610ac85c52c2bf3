"""CPU: the host side of the yaw fit (cm3d_amd/bevfit.py, csrc/pass_options.cpp).  The statement's axis against the true yaw of
noise-free two-face lists, within a bound that is derived and not measured; the statement against a separately written plain loop; the
conditions the case tables of tests/bev_fit_cases.py must meet; YawFit's argument checks; the new descriptor's layout; and the call
sequences of cm3d_lift_pass_yaw_fitted / cm3d_yaw_fit_boxes, traced over stubs by a stand-alone program built with the address and
undefined-behaviour sanitizers."""
import ctypes
import math
import os
import shutil
import subprocess

import numpy as np
import pytest

from cm3d_amd import bevfit
from tests import bev_fit_cases as cases
from tests import pass_options_trace as T

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _fit(name, K=128):
    return bevfit.bev_fit_host(cases.standalone()[name][0], K, cases.D0, cases.MIN_POINTS, cases.MIN_LENGTH)


@pytest.mark.parametrize("K", cases.ANGLES)
def test_axis_of_noise_free_cars_within_the_derived_bound(K):
    """delta + asin(d0 / Lmax) of the true yaw modulo pi / 2, delta = pi / (2K) the grid step: inside asin(d0 / Lmax) of the truth every
    point's deviation from its face is below d0, where the criterion is flat, so the maximum can sit one step beyond that."""
    worst, noisy = 0.0, 0.0
    for name, (xyz, meta) in cases.standalone().items():
        if meta["kind"] not in ("car", "car_far", "car_noisy"):
            continue
        k, rect, st = _fit(name, K)
        assert st == bevfit.FITTED and 0 <= k < K, name
        err = cases.axis_error(rect, meta["yaw"])
        if meta["kind"] == "car_noisy":
            noisy = max(noisy, err)
            continue
        worst = max(worst, err)
        assert err <= cases.known_answer_bound(K, meta["lmax"]), (name, err)
        assert abs(rect[2] - cases.CAR_L) < 0.1 and abs(rect[3] - cases.CAR_W) < 0.1, (name, rect)
    step = math.pi / (2 * K)
    print(f"K={K}: noise-free worst {worst / step:.2f} steps (bound {cases.known_answer_bound(K) / step:.2f}); "
          f"3 cm of noise: worst {noisy / step:.2f} steps (printed, not asserted)")


def test_tables_hold_what_they_are_for():
    lists = cases.standalone()
    n = {name: len(v[0]) for name, v in lists.items()}
    st = {name: _fit(name)[2] for name in lists}
    assert set(st.values()) == {0, 1, 2, 3, 4}
    C = cases.BEV_FIT_CHUNK
    for want in (0, 1, 2, cases.MIN_POINTS - 1, cases.MIN_POINTS, 63, 64, 65, 127, 128, 129, C - 1, C, C + 1):
        assert want in n.values(), want
    assert any(900 <= v <= 1100 for v in n.values()) and any(4500 <= v <= 5500 for v in n.values())
    assert st["len_0"] == bevfit.EMPTY and st["len_1"] == st["len_2"] == st[f"len_{cases.MIN_POINTS - 1}"] == bevfit.FEW_POINTS
    assert st[f"len_{cases.MIN_POINTS}"] == bevfit.FITTED and st["len_5003"] == bevfit.FITTED
    assert st["nan_row"] == st["inf_first_row"] == bevfit.NON_FINITE and st["short"] == st["all_the_same_point"] == bevfit.SHORT
    assert np.unique(lists["duplicates"][0], axis=0).shape[0] < n["duplicates"] and st["duplicates"] == bevfit.FITTED
    k, rect, s = _fit("collinear")
    assert s == 0 and k == 0 and rect[3] == 0.0 and rect[2] == 0.125 * 39 and tuple(rect[4:]) == (1.0, 0.0)
    k, rect, s = _fit("square")                    # a == b: the axis is (c, s), not (-s, c)
    assert s == 0 and k == 0 and rect[2] == rect[3] == 2.0 and tuple(rect[4:]) == (1.0, 0.0) and tuple(rect[:2]) == (601.0, 1201.0)
    assert sum(m["kind"] == "car" for _, m in lists.values()) == 41 == sum(m["kind"] == "car_noisy" for _, m in lists.values())
    yaws = [m["yaw"] for _, m in lists.values() if m["kind"] == "car"]
    assert min(yaws) > -math.pi and max(yaws) == math.pi
    assert max(np.abs(v[0][:, :2]).max() for v in lists.values() if len(v[0]) and np.isfinite(v[0]).all()) > 9900
    # both branches of the axis choice
    sides = {bool(abs(_fit(f"car_{i:02d}")[1][4] - bevfit.angle_table(128)[_fit(f"car_{i:02d}")[0], 0]) < 1e-15) for i in range(41)}
    assert sides == {True, False}


@pytest.mark.parametrize("waymo", [False, True])
def test_select_tables_hold_what_they_are_for(waymo):
    t = cases.select_table(waymo)
    assert (t["pose_rt"] is not None) == waymo
    if waymo:
        yaws = np.arctan2(t["pose_rt"][:, 3], t["pose_rt"][:, 0])
        assert np.any(np.abs(yaws - np.pi / 2) < 0.05) and np.any(np.abs(np.abs(yaws) - np.pi) < 0.05)
    assert set(t["fit_status"]) == {0, 1, 2, 3, 4} and (t["medoid_pos"] < 0).any()
    assert (cases.IS_VEHICLE[np.clip(t["class_id"], 0, 9)] == 0).any()
    dots, flips = [], set()
    for m in range(len(t["medoid_pos"])):
        if t["fit_status"][m] == 0 and t["medoid_pos"][m] >= 0:
            _, _, dot = bevfit.select_dot(t["fit_rect"][m], t["lane_yaw"][m], None if not waymo else t["pose_rt"][t["mask_frame"][m]])
            dots.append(abs(dot))
            flips.add(bool(dot < 0))
    # NO case has |dot| < 1e-9: the flip is never decided by the last bit of a library's cosine
    assert min(dots) >= 1e-9 and min(dots) < 0.03 and flips == {True, False}
    seen = set()
    for lmd in cases.LANE_MIN_DISTS:
        yaw, src = cases.select_host(t, lmd)
        assert set(src) == {0, 1} and yaw.dtype == np.float32
        seen |= {(lmd, int(np.sign(d - lmd))) for d in t["lane_dist"][np.isfinite(t["lane_dist"])]}
        lane_src = src == 0
        has = t["medoid_pos"] >= 0
        assert np.array_equal(yaw[lane_src & has].view(np.uint32), t["lane_yaw"][lane_src & has].view(np.uint32))
        assert not yaw[~has].any() and not src[~has].any()
    assert {(2.0, -1), (2.0, 0), (2.0, 1), (3.0, -1), (3.0, 0), (3.0, 1)} <= seen        # either side of a lane distance, and exactly on it
    a, b = cases.select_host(t, 0.0)[1], cases.select_host(t, 3.0)[1]
    assert (a != b).any() and b.sum() < a.sum()
    # the fitted yaw is the axis or its opposite, whichever lies along the lane (in the lane's frame)
    yaw, src = cases.select_host(t, 0.0)
    for m in np.flatnonzero(src == 1):
        cg, sg, _ = bevfit.select_dot(t["fit_rect"][m], t["lane_yaw"][m], None if not waymo else t["pose_rt"][t["mask_frame"][m]])
        d = (float(yaw[m]) - math.atan2(sg, cg)) % math.pi
        assert min(d, math.pi - d) < 1e-6
        assert math.cos(float(yaw[m]) - float(t["lane_yaw"][m])) > 0


def _plain_loop(xyz, K, d0, min_points, min_length):
    """The rule of include/cm3d_hip.h written out point by point in Python floats (IEEE double, no contraction)."""
    pts = [(np.float32(p[0]), np.float32(p[1])) for p in xyz]
    n = len(pts)
    if n == 0:
        return -1, [0.0] * 6, 2
    if n < min_points:
        return -1, [0.0] * 6, 1
    if any(not (math.isfinite(x) and math.isfinite(y)) for x, y in pts):
        return -1, [0.0] * 6, 4
    x0, y0 = float(pts[0][0]), float(pts[0][1])
    rel = [(float(x) - x0, float(y) - y0) for x, y in pts]
    best = None
    for k in range(K):
        th = k * math.pi / (2.0 * K)
        c, s = float(np.cos(np.float64(th))), float(np.sin(np.float64(th)))
        c1 = [(x * c) + (y * s) for x, y in rel]
        c2 = [(y * c) - (x * s) for x, y in rel]
        lo1, hi1, lo2, hi2 = min(c1), max(c1), min(c2), max(c2)
        q = 0.0
        for u, v in zip(c1, c2):
            q = q + 1.0 / max(min(min(hi1 - u, u - lo1), min(hi2 - v, v - lo2)), d0)
        if best is None or q > best[0]:
            best = (q, k, c, s, lo1, hi1, lo2, hi2)
    _, k, c, s, lo1, hi1, lo2, hi2 = best
    a, b = hi1 - lo1, hi2 - lo2
    if max(a, b) < min_length:
        return -1, [0.0] * 6, 3
    m1, m2 = (lo1 + hi1) * 0.5, (lo2 + hi2) * 0.5
    ax = (c, s) if a >= b else (-s, c)
    return k, [((m1 * c) - (m2 * s)) + x0, ((m1 * s) + (m2 * c)) + y0, max(a, b), min(a, b), ax[0], ax[1]], 0


def test_statement_equals_a_plain_loop():
    names = ["len_0", "len_2", "len_19", "len_20", "len_63", "len_65", "len_129", "nan_row", "short", "duplicates", "collinear", "square",
             "car_03", "car_noisy_17", "car_far_02"]
    for name in names:
        xyz = cases.standalone()[name][0]
        for K, d0, mp, ml in ((64, 0.05, 20, 1.0), (128, 0.1, 2, 0.0)):
            k, rect, st = bevfit.bev_fit_host(xyz, K, d0, mp, ml)
            pk, prect, pst = _plain_loop(xyz, K, d0, mp, ml)
            assert (k, st) == (pk, pst), (name, K)
            assert np.array_equal(np.asarray(rect).view(np.uint64), np.array(prect, np.float64).view(np.uint64)), (name, K, rect, prect)


def test_yaw_fit_arguments():
    Y = bevfit.YawFit
    y = Y()
    assert (y.angles, y.min_points, y.min_length, y.d0, y.lane_min_dist, y.active) == (128, 20, 1.0, 0.05, 0.0, True)
    assert Y(192).angles == 192 and Y(256, 2, 0.0, 1e-3, float("inf")).lane_min_dist == float("inf")
    for bad in (dict(angles=0), dict(angles=32), dict(angles=100), dict(angles=320), dict(angles=64.5), dict(min_points=1), dict(min_points=2.5),
                dict(min_length=-0.1), dict(min_length=float("nan")), dict(min_length=float("inf")), dict(d0=0.0), dict(d0=-1.0),
                dict(d0=float("nan")), dict(d0=float("inf")), dict(lane_min_dist=-1.0), dict(lane_min_dist=float("nan"))):
        with pytest.raises(ValueError):
            Y(**bad)
    assert Y.from_args("lane", 64, 5, 2.0, 0.1, 1.0) is None
    got = Y.from_args("fit", 64, 5, 2.0, 0.1, 1.0)
    assert (got.angles, got.min_points, got.min_length, got.d0, got.lane_min_dist) == (64, 5, 2.0, 0.1, 1.0)
    with pytest.raises(ValueError):
        Y.from_args("pca")
    import argparse
    ap = argparse.ArgumentParser()
    bevfit.add_arguments(ap)
    assert bevfit.from_namespace(ap.parse_args([])) is None and bevfit.from_namespace(ap.parse_args(["--yaw", "lane"])) is None
    assert bevfit.from_namespace(ap.parse_args(["--yaw", "fit"])) == Y()
    c = bevfit.from_namespace(ap.parse_args(["--yaw", "fit", "--yaw-fit-angles", "256", "--yaw-fit-min-points", "7", "--yaw-fit-min-length", "2",
                                             "--yaw-fit-d0", "0.02", "--yaw-fit-lane-min-dist", "4"]))
    assert (c.angles, c.min_points, c.min_length, c.d0, c.lane_min_dist) == (256, 7, 2.0, 0.02, 4.0)
    for bad in (dict(angles=96), dict(d0=0.0), dict(min_points=1), dict(min_length=-1.0)):
        with pytest.raises(ValueError):
            bevfit.bev_fit_host(np.zeros((30, 3), np.float32), **bad)
    t = bevfit.angle_table(64)
    assert t.shape == (64, 2) and t.dtype == np.float64 and tuple(t[0]) == (1.0, 0.0) and t[32, 0] == np.cos(np.pi / 4)


def test_yaw_fit_descriptor_layout_matches_the_header(tmp_path):
    if shutil.which("gcc") is None:
        pytest.skip("no gcc")
    from cm3d_amd import _lib
    names = [n for n, _ in _lib.YawFitDesc._fields_]
    assert names == ["size", "angle_cs", "hit_xyz", "hit_off", "medoid_pos", "fit_k", "fit_rect", "fit_status", "yaw_tab", "yaw_idx", "yaw_src",
                     "tab_off", "tab_frame", "ev", "d0", "min_length", "lane_min_dist", "K", "min_points"]
    src = tmp_path / "t.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "cm3d_hip.h"\nint main(void) {\n'
                   + "".join(f'printf("%zu\\n", offsetof(cm3d_yaw_fit_desc, {n}));\n' for n in names)
                   + 'printf("%zu\\n%d\\n", sizeof(cm3d_yaw_fit_desc), CM3D_BEV_FIT_CHUNK); return 0; }\n')
    exe = tmp_path / "t"
    r = subprocess.run(["gcc", "-std=c99", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    got = [int(x) for x in subprocess.run([str(exe)], capture_output=True, text=True).stdout.split()]
    assert got == [getattr(_lib.YawFitDesc, n).offset for n in names] + [ctypes.sizeof(_lib.YawFitDesc), _lib.BEV_FIT_CHUNK]
    assert 16 * _lib.BEV_FIT_CHUNK <= 16 * 1024       # a staged chunk: a fraction of a CU's LDS, so masks run side by side


def test_new_symbols_within_abi_5_and_bad_descriptors_never_launch():
    from cm3d_amd import _lib
    L = _lib.lib()
    assert _lib.ABI_VERSION == 5 and L.cm3d_abi_version() == 5
    d, y = _lib.LiftPassDesc(), _lib.YawFitDesc()
    for fn in (L.cm3d_lift_pass_yaw_fitted, L.cm3d_yaw_fit_boxes):
        assert fn(None, None, None) == -1
        assert fn(ctypes.byref(d), ctypes.byref(y), None) == -1                      # sizes not filled
    d.size, y.size = ctypes.sizeof(d), ctypes.sizeof(y)
    for fn in (L.cm3d_lift_pass_yaw_fitted, L.cm3d_yaw_fit_boxes):
        assert fn(ctypes.byref(d), ctypes.byref(y), None) == -1                      # no tables, no outputs


WAYMO_EVENTS = dict(ev=0x50, K=64, d0="0.1", mn="5,2.5", lmd="1.5", pose="pose_rt", pose_inv="pose_inv", bound=1024)
SEQ_CASES = {
    "plain": dict(first=True),
    "boxes_alone": dict(first=False),
    "waymo_events": dict(first=True, **WAYMO_EVENTS),
    # (lists of the caller's own: cm3d_yaw_fit_boxes alone takes them, a pass fits what it derives -- "own_lists_in_a_pass" below)
    "waymo_events_own_lists": dict(first=False, lists="cl_xyz,cl_off", pos="kept", **WAYMO_EVENTS),
}


def test_yaw_fitted_pass_sequence_under_sanitizers():
    """cm3d_lift_pass_yaw_fitted and cm3d_yaw_fit_boxes over stubs (tests/pass_options_sim.cpp): the plain pass, the fit on the pass's
    lists (cm3d_yaw_fit_boxes alone: or the fit's own), the selection on the pass's lane results, the events around those two, the box
    launch with the yaw table where the lane tables stood and the real lane_dist; a descriptor of another size or a null table or
    output makes no call, nor does a pass that is handed lists it does not derive itself; and whichever call fails, the pass ends there
    with that call's error."""
    got = T.group("yaw")
    refused = ["wrong_size", "wrong_size_boxes", "wrong_pass_size", "wrong_pass_size_boxes", "no_angle_cs", "no_fit_k", "no_fit_rect",
               "no_fit_status", "no_yaw_tab", "no_yaw_idx", "no_yaw_src", "no_tab_off", "no_tab_frame", "null_pass", "null_fit",
               "null_fit_pass", "own_lists_in_a_pass"]
    for name in refused:
        T.assert_refused(got.pop(name), name)
    assert set(got) == set(SEQ_CASES)
    for name, kw in SEQ_CASES.items():
        kw = dict(kw)
        T.assert_pass(got[name], (T.plain_sequence() if kw.pop("first") else []) + T.yaw_sequence(**kw), name)


def test_pipeline_cpp_does_not_know_the_yaw_fitted_pass():
    """The plain pass links without the new entry points (tests/lift_pass_sim.cpp's stubs), and k_box_nms is what it was."""
    src = open(os.path.join(ROOT, "cm3d_amd", "csrc", "pipeline.cpp")).read()
    assert "bev_fit" not in src and "yaw_select" not in src and "yaw_fit" not in src
    boxes = open(os.path.join(ROOT, "cm3d_amd", "csrc", "boxes.hip")).read()
    assert "yaw_tab" not in boxes and "bev_fit" not in boxes
