"""CPU: the box placement (cm3d_amd/boxplace.py, cm3d_box_place, cm3d_lift_pass_placed).  box_place_host against a separately written
plain loop on the case tables, bit for bit; the geometry of the rule on visible-face cars against a derived bound and against the pushed
medoid; what the case tables hold; the flags; the call sequence of the placed pass, traced over stubs by a stand-alone program built with
the address and undefined-behaviour sanitizers (tests/pass_place_sim.cpp) and compared with the sequence include/cm3d_hip.h states; the
ctypes layout of the descriptor; the symbols."""
import argparse
import ctypes
import functools
import itertools
import math
import os
import shutil
import subprocess
import tempfile

import numpy as np
import pytest

from cm3d_amd import bevfit, boxplace
from tests import bev_fit_cases as fc
from tests import box_place_cases as pc
from tests import pass_options_trace as T
from tests.test_pipe_sched_host import SANITIZED

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ------------------------------------------------------------------------------------------------ the rule, once more, as a plain loop
def plain_loop(t, thin, bound):
    """cm3d_box_place as include/cm3d_hip.h states it, mask by mask on Python floats (IEEE doubles: every operation rounds on its own).
    Shares nothing with boxplace.box_place_host."""
    box = [[float(v) for v in row] for row in t["box"]]
    flags = [int(v) for v in t["flags"]]
    M = len(flags)
    rect, src_in = t["fit_rect"], t["yaw_src"]
    prior, group, thr = t["prior_wlh"], t["nms_group"], t["nms_thr"]
    place_src, pushed = [0] * M, [(b[0], b[1]) for b in box]
    fin = math.isfinite
    for f in range(len(t["mask_off"]) - 1):
        m0 = min(max(int(t["mask_off"][f]), 0), M)
        m1 = min(max(int(t["mask_off"][f + 1]), m0), M)
        nm = min(m1 - m0, bound, 1024)
        sx, sy = (0.0, 0.0) if t["ego_xyz"] is None else (float(t["ego_xyz"][f][0]), float(t["ego_xyz"][f][1]))
        cls_of = {}
        for m in range(m0, m0 + nm):
            b8 = box[m][8]
            c = int(b8) if b8 >= 0.0 and b8 < float(len(prior)) else 0
            cls_of[m] = c
            cx, cy, a, b, hc, hs = (float(v) for v in rect[m])
            if not (flags[m] & 1 and int(src_in[m]) == 1 and fin(sx) and fin(sy) and all(fin(v) for v in (cx, cy, a, b, hc, hs))):
                continue
            ln, wd = float(prior[c][1]), float(prior[c][0])
            ex = sx - cx; ey = sy - cy
            pu = (ex * hc) + (ey * hs); pv = (ey * hc) - (ex * hs)
            su = 1.0 if pu >= 0 else -1.0; sv = 1.0 if pv >= 0 else -1.0
            au = b >= thin; av = a >= thin
            du = su * ((a - ln) * 0.5) if au else 0.0
            dv = sv * ((b - wd) * 0.5) if av else 0.0
            box[m][0] = ((du * hc) - (dv * hs)) + cx
            box[m][1] = ((du * hs) + (dv * hc)) + cy
            place_src[m] = 1 if au and av else 2 if au or av else 3
        # the circle NMS again: descending score, ties by descending index
        live = [m for m in range(m0, m0 + nm) if flags[m] & 1]
        live.sort(key=lambda m: (box[m][7], m), reverse=True)
        gone = set()
        for m in range(m0, m1):
            flags[m] &= ~2
        for r, i in enumerate(live):
            if i in gone:
                continue
            flags[i] |= 2
            gi = int(group[cls_of[i]])
            for j in live[r + 1:]:
                gj = int(group[cls_of[j]])
                dx = box[i][0] - box[j][0]; dy = box[i][1] - box[j][1]
                if gj == gi and (dx * dx) + (dy * dy) <= float(thr[gj]):
                    gone.add(j)
        for m in range(m0, m1):
            box[m][9] = float(flags[m])
    return dict(box=np.array(box, np.float64).reshape(M, 10), flags=np.array(flags, np.int32), place_src=np.array(place_src, np.int32),
                place_pushed=np.array(pushed, np.float64).reshape(M, 2))


def host(t, thin=pc.THIN, bound=1024):
    return boxplace.box_place_host(t["box"], t["flags"], t["mask_off"], t["fit_rect"], t["yaw_src"], t["prior_wlh"], t["nms_group"], t["nms_thr"],
                                   t["ego_xyz"], thin, bound)


def same_bits(a, b):
    assert set(a) == set(b)
    for key in a:
        assert a[key].dtype == b[key].dtype and a[key].shape == b[key].shape, key
        assert a[key].tobytes() == b[key].tobytes(), key


@pytest.mark.parametrize("waymo", [False, True], ids=["nusc", "waymo"])
@pytest.mark.parametrize("table", ["rule", "nms"])
def test_host_statement_equals_the_plain_loop_to_the_bit(table, waymo):
    t = pc.rule_table(waymo) if table == "rule" else pc.nms_table(waymo)
    for thin, bound in itertools.product(pc.THINS, pc.BOUNDS):
        got = host(t, thin, bound)
        same_bits(got, plain_loop(t, thin, bound))
        # what every call leaves alone
        assert got["box"][:, 2:9].tobytes() == t["box"][:, 2:9].tobytes() and got["place_pushed"].tobytes() == t["box"][:, :2].tobytes()
        off = got["place_src"] == 0
        assert got["box"][off, :9].tobytes() == t["box"][off, :9].tobytes()
        assert np.array_equal(got["flags"] & 1, t["flags"] & 1) and np.array_equal(got["box"][:, 9], got["flags"].astype(np.float64))


@pytest.mark.parametrize("waymo", [False, True], ids=["nusc", "waymo"])
def test_rule_table_holds_what_it_is_for(waymo):
    t = pc.rule_table(waymo)
    r = host(t)
    name = lambda n: [m for m, v in enumerate(t["names"]) if v.startswith(n)]
    frame = np.repeat(np.arange(len(t["mask_off"]) - 1), np.diff(t["mask_off"]))
    sens = np.zeros((len(frame), 2)) if waymo else t["ego_xyz"][frame, :2]
    rect = t["fit_rect"]
    with np.errstate(invalid="ignore"):
        ex, ey = sens[:, 0] - rect[:, 0], sens[:, 1] - rect[:, 1]
        pu, pv = ex * rect[:, 4] + ey * rect[:, 5], ey * rect[:, 4] - ex * rect[:, 5]
    quad = name("quadrant")
    assert {(bool(pu[m] >= 0), bool(pv[m] >= 0)) for m in quad} == set(itertools.product((False, True), repeat=2))
    assert all(pu[m] == 0.0 and pv[m] != 0.0 for m in name("pu_zero")) and all(pv[m] == 0.0 and pu[m] != 0.0 for m in name("pv_zero"))
    assert len(name("pu_zero")) == 3 and len(name("pv_zero")) == 3
    # the rule does not need the axis' sign: every record with its axis negated gives the same bits (negation is exact, and pu, pv,
    # su, sv change sign together)
    neg = rect.copy()
    neg[:, 4:6] = -neg[:, 4:6]
    rn = host(dict(t, fit_rect=neg))
    rest = np.array([not v.startswith(("pu_zero", "pv_zero")) for v in t["names"]])      # (on pu == 0 the tie goes to +1 either way)
    assert rn["box"][rest, :2].tobytes() == r["box"][rest, :2].tobytes() and np.array_equal(rn["place_src"], r["place_src"])
    assert not np.array_equal(rn["box"][~rest, :2], r["box"][~rest, :2]) and (r["place_src"][quad] == 1).all()
    ext = name("extent_")
    assert {(float(rect[m, 2]), float(rect[m, 3])) for m in ext} == set(itertools.product((0.25, 0.5, 3.0), (0.25, 0.5, 1.5)))
    assert {int(r["place_src"][m]) for m in ext} == {1, 2, 3}
    for m in ext:                                              # on the threshold counts as seen
        assert r["place_src"][m] == {2: 1, 1: 2, 0: 3}[int(rect[m, 2] >= 0.5) + int(rect[m, 3] >= 0.5)]
    assert set(host(t, 0.0)["place_src"][ext]) == {1}
    assert all(rect[m, 2] > 4.5 for m in name("longer_than")) and all(rect[m, 3] > 1.9 for m in name("wider_than"))
    for n in ("lane_yaw_kept", "no_box", "rect_nan", "rect_inf", "nan_sensor"):
        assert (r["place_src"][name(n)] == 0).all(), n
    assert (len(name("nan_sensor")) == 0) == waymo and (t["ego_xyz"] is None) == waymo
    # a class outside the table is class 0: the same offset from the record's centre as the class-0 case with the same extents
    for n in ("class_below", "class_above", "class_nan"):
        for m in name(n):
            assert r["place_src"][m] == 1 and not 0 <= t["box"][m, 8] < len(pc.PRIOR_WLH)
    with np.errstate(invalid="ignore"):
        far, mid = np.isfinite(rect[:, 0]) & (np.abs(rect[:, 0]) > 9000), np.abs(rect[:, 1]) > 1000      # near 10 km; 600 / 1200 m
    assert far.any() == (not waymo) and mid.any() == (not waymo)
    assert np.bincount(r["place_src"], minlength=4).min() >= 3                   # every value, in every frame


@pytest.mark.parametrize("waymo", [False, True], ids=["nusc", "waymo"])
def test_nms_table_holds_what_it_is_for(waymo):
    t = pc.nms_table(waymo)
    assert tuple(np.diff(t["mask_off"])) == pc.FRAME_SIZES == (0, 1, 2, 63, 64, 65, 130)
    r = host(t, bound=1024)
    pushed_only = dict(t, yaw_src=np.zeros_like(t["yaw_src"]))
    q = host(pushed_only, bound=1024)
    assert len(t["pairs"]) == 1 + 4 * 5
    for i, j, goes in t["pairs"]:
        assert t["box"][i, 7] >= t["box"][j, 7] and r["flags"][i] == 3 and r["flags"][j] == (1 if goes else 3), (i, j)
    on = [(i, j) for i, j, _ in t["pairs"] if t["yaw_src"][i] == 0]
    d2 = sorted({float((t["box"][i, 0] - t["box"][j, 0]) ** 2 + (t["box"][i, 1] - t["box"][j, 1]) ** 2) for i, j in on})
    assert len(d2) >= 3 and 4.0 in d2 and d2[0] < 4.0 < d2[-1] and d2[-1] - d2[0] < 1e-11
    # the placement merges one pair the pushed centres kept apart and parts one they merged
    moved = [(i, j, goes) for i, j, goes in t["pairs"] if t["yaw_src"][i] == 1]
    assert len(moved) == 8 and all((q["flags"][j] == 3) == goes for _, j, goes in moved)
    # a frame of 65 / 130: the designed masks straddle or lie beyond the 64th; a bound of 64 takes them out
    r64 = host(t, bound=64)
    for f in (5, 6):
        m0, m1 = int(t["mask_off"][f]), int(t["mask_off"][f + 1])
        assert not (r64["flags"][m0 + 64:m1] & 2).any() and not r64["place_src"][m0 + 64:m1].any() and (r["flags"][m0 + 64:m1] & 2).any()
        assert any(m0 <= i < m0 + 64 <= j for i, j, _ in t["pairs"]) or f == 6
    ties = [np.unique(t["box"][int(a):int(b), 7]).size < b - a for a, b in zip(t["mask_off"][3:-1], t["mask_off"][4:])]
    assert all(ties) and (t["flags"] == 0).sum() >= 20 and (r["flags"] == 1).sum() >= 30


# ------------------------------------------------------------------------------------------------ (c) the geometry of the rule
def _pushed_medoid(orc, xyz, sensor, yaw, prior):
    """The box launch's centre for the list: the medoid of the points, pushed along the view ray (the oracle's box_assemble) with the
    given yaw."""
    p = xyz[:, :3].astype(np.float64)
    d = np.sqrt(((p[:, None, :] - p[None, :, :]) ** 2).sum(2)).sum(1)
    t, _ = orc.box_assemble(xyz[int(np.argmin(d)), :3], prior, yaw, np.array([sensor[0], sensor[1], 0.0]), True)
    return t[:2]


@pytest.mark.parametrize("faces", [2, 1])
def test_placed_centre_of_visible_face_cars(oracle, faces):
    """With the true size as the prior the placed centre lies within (pi / 2K + asin(d0 / CAR_L)) * (CAR_L + CAR_W) of the true one:
    the angle bound of the fit times the lever of the corner.  Derived, not measured: 0.228 / 0.150 / 0.110 m at K = 64 / 128 / 256.
    Seen here: at most 0.029 / 0.027 / 0.027 m with two faces and 0.054 / 0.055 / 0.055 m with one.  The medoid pushed along the ray with
    the same fitted yaw (the oracle's box_assemble) is 0.65 m off in the median with two faces and 1.17 m with one, 1.63 m at worst; at
    least 95 % of the cases must be placed nearer than pushed (seen: all of them)."""
    cases = pc.cars(faces)
    assert pc.N_GEOMETRIES == 984 and len(cases) == pc.CARS_LEFT[faces]
    prior = np.array([[pc.CAR_W, pc.CAR_L, 1.5]])
    assert [round(pc.placed_bound(K), 3) for K in fc.ANGLES] == [0.228, 0.150, 0.110]
    for K in fc.ANGLES:
        tab = bevfit.angle_table(K)
        placed, pushed = [], []
        for xyz, centre, sensor, yaw in cases:
            _, rect, status = bevfit.bev_fit_host(xyz, K, table=tab)
            assert status == bevfit.FITTED
            fitted_yaw = math.atan2(rect[5], rect[4])
            push = _pushed_medoid(oracle, xyz, sensor, fitted_yaw, prior[0])
            box = np.zeros((1, 10))
            box[0, 0:2], box[0, 3], box[0, 7] = push, 1.0, 0.5
            r = boxplace.box_place_host(box, [1], [0, 1], rect[None], [1], prior, [0], [4.0], np.array([[sensor[0], sensor[1], 0.0]]), pc.THIN)
            assert r["place_src"][0] == (1 if faces == 2 else 2) and r["place_pushed"].tobytes() == box[:, :2].tobytes()
            placed.append(math.hypot(*(r["box"][0, :2] - centre)))
            pushed.append(math.hypot(*(push - centre)))
        placed, pushed = np.array(placed), np.array(pushed)
        nearer = float((placed < pushed).mean())
        print(f"{faces} face(s), K={K}: placed max {placed.max():.4f} m (bound {pc.placed_bound(K):.4f}); pushed median {np.median(pushed):.3f} m, "
              f"max {pushed.max():.3f} m; placed nearer than pushed in {100 * nearer:.1f} % of {len(cases)}")
        assert placed.max() <= pc.placed_bound(K)
        assert nearer >= 0.95


# ------------------------------------------------------------------------------------------------ the switches
def test_switches_are_validated():
    assert boxplace.BoxPlace().thin == 0.5 and boxplace.BoxPlace(0).thin == 0.0 and boxplace.BoxPlace().active
    for bad in (-0.1, float("nan"), float("inf")):
        with pytest.raises(ValueError):
            boxplace.BoxPlace(bad)
        with pytest.raises(ValueError):
            boxplace.box_place_host(np.zeros((1, 10)), [0], [0, 1], np.zeros((1, 6)), [0], pc.PRIOR_WLH, pc.NMS_GROUP, pc.NMS_THR, None, bad)
    ap = argparse.ArgumentParser()
    bevfit.add_arguments(ap)
    boxplace.add_arguments(ap)
    ns = ap.parse_args([])
    assert ns.place == "push" and ns.place_thin == 0.5 and boxplace.from_namespace(ns, ap) is None
    assert boxplace.from_namespace(ap.parse_args(["--place", "push", "--place-thin", "2"]), ap) is None
    got = boxplace.from_namespace(ap.parse_args(["--yaw", "fit", "--place", "fit", "--place-thin", "0.25"]), ap)
    assert got == boxplace.BoxPlace(0.25)
    assert boxplace.from_namespace(ap.parse_args(["--yaw", "fit", "--place", "fit"])) == boxplace.BoxPlace()
    with pytest.raises(ValueError):
        boxplace.from_namespace(ap.parse_args(["--place", "fit"]))
    for argv in (["--place", "fit"], ["--yaw", "lane", "--place", "fit"], ["--yaw", "fit", "--place", "fit", "--place-thin", "-1"]):
        with pytest.raises(SystemExit):                        # an error of the command line
            boxplace.from_namespace(ap.parse_args(argv), ap)
    with pytest.raises(SystemExit):
        ap.parse_args(["--place", "corner"])


def test_entry_points_carry_the_flags():
    for rel, want in (("pipeline_nuscenes.py", True), ("pipeline_waymo.py", True), ("pipeline_kitti.py", False)):
        src = open(os.path.join(ROOT, "cm3d_amd", rel)).read()
        assert ("boxplace.add_arguments(ap)" in src) == want and ("boxplace.from_namespace(args, ap)" in src) == want, rel


def test_engine_refuses_a_placement_without_a_yaw_fit(monkeypatch):
    from cm3d_amd import lifting
    monkeypatch.setattr(lifting.torch.cuda, "is_available", lambda: True)
    with pytest.raises(ValueError, match="needs yaw=YawFit"):
        lifting.LiftEngine("cpu", place=boxplace.BoxPlace())


# ------------------------------------------------------------------------------------------------ the placed pass over stubs
CODE = dict(T.CODE, cm3d_box_place=-3)


@functools.lru_cache(maxsize=None)
def _run_sim():
    tmp = tempfile.mkdtemp(prefix="pass_place_sim")
    try:
        exe = os.path.join(tmp, "pass_place_sim")
        rocm = os.environ.get("ROCM_PATH", "/opt/rocm")
        csrc = os.path.join(ROOT, "cm3d_amd", "csrc")
        r = subprocess.run(SANITIZED + ["-D__HIP_PLATFORM_AMD__", "-isystem", os.path.join(rocm, "include"), os.path.join(ROOT, "tests", "pass_place_sim.cpp"),
                                        os.path.join(csrc, "pass_compose.cpp"), os.path.join(csrc, "pass_options.cpp"), "-o", exe],
                           capture_output=True, text=True)
        assert r.returncode == 0, r.stderr
        r = subprocess.run([exe], capture_output=True, text=True)            # its own executable: the sanitizers' runtimes are linked in
        assert r.returncode == 0 and r.stdout.endswith("pass_place_sim done\n"), r.stdout + r.stderr
    finally:
        shutil.rmtree(tmp, ignore_errors=True)
    got = {}
    for line in r.stdout.splitlines()[:-1]:
        if line.startswith("case "):
            assert line[5:] not in got, line
            calls, rc, fails = got[line[5:]] = ([], [], [])
        elif line.startswith("rc "):
            rc.append(int(line[3:]))
        elif line.startswith("fail "):
            fails.append(tuple(int(x) for x in line.split()[1:]))
        else:
            calls.append(line)
    return got


def sim():
    rocm = os.environ.get("ROCM_PATH", "/opt/rocm")
    if shutil.which("g++") is None or not os.path.exists(os.path.join(rocm, "include", "hip", "hip_runtime_api.h")):
        pytest.skip("no g++ or no HIP headers")
    return _run_sim()


def placed_sequence(cluster, filt, nms, waymo=False, ev=0x70, thin="0.5"):
    """include/cm3d_hip.h's statement of cm3d_lift_pass_placed: the composed pass without its rotated NMS, the placement between its
    events, the rotated NMS."""
    bound = 1024 if waymo else 96
    return (T.composed_sequence(cluster, filt, True, False, waymo=waymo) + T.records(ev, 0)
            + [f"cm3d_box_place io=box,flags off=mask_off rest=set n=3,7,10 waymo={int(waymo)} thin={thin} bound={bound} out=set,set"]
            + T.records(ev, 1) + (T.nms_sequence(int(waymo), bound) if nms else []))


def assert_pass(trace, want, name):
    calls, rc, fails = trace
    assert calls == want, name
    assert rc == [0], name
    assert fails == [(k, CODE[c.split()[0]], k + 1) for k, c in enumerate(calls)], name       # ends at the first error, with its code


@pytest.mark.parametrize("waymo", [False, True], ids=["nusc", "waymo"])
def test_placed_pass_makes_the_headers_calls_and_ends_at_the_first_error(waymo):
    got = sim()
    for c, f, n in itertools.product((False, True), repeat=3):
        which = ("c" if c else "-") + ("f" if f else "-") + "y" + ("n" if n else "-")
        assert_pass(got[("combo_waymo." if waymo else "combo.") + which], placed_sequence(c, f, n, waymo), which)
    assert_pass(got["ok.no_events_thin_0"], placed_sequence(False, False, True, ev=0, thin="0"), "no events")


def test_every_refusal_of_the_placed_pass_makes_no_call():
    got = sim()
    bad = {name: t for name, t in got.items() if name.startswith("bad.")}
    assert set(bad) == {"bad." + n for n in ("no_yaw", "no_member", "place_size", "opt_size", "pass_size", "yaw_size", "nms_size", "nms_no_thr", "cluster_size",
                                             "filter_no_on_road", "no_place_src", "no_place_pushed", "yaw_no_fit_rect", "yaw_no_yaw_src", "yaw_no_tab_off",
                                             "thin_negative", "thin_nan", "thin_inf", "null_place", "null_opt", "null_pass")}
    for name, trace in bad.items():
        T.assert_refused(trace, name)


def test_placed_pass_writes_to_no_descriptor_of_the_callers():
    got = sim()
    assert len(got) == 16 + 1 + 21
    assert not [name for name, (calls, _, _) in got.items() if any("descriptor was changed" in c for c in calls)]


def test_pass_options_cpp_does_not_know_the_placement():
    csrc = os.path.join(ROOT, "cm3d_amd", "csrc")
    for rel in ("pass_options.cpp", "pipeline.cpp"):
        src = open(os.path.join(csrc, rel)).read()
        assert "box_place" not in src and "pass_placed" not in src and "pass_place" not in src, rel
        assert "ground_strip" not in src and "point_owner" not in src and "pass_compose" not in src, rel
    src = open(os.path.join(csrc, "pass_compose.cpp")).read()
    assert src.count("cm3d_pass_seam_run(") == 1 and "cm3d_box_nms_bounded(" not in src


# ------------------------------------------------------------------------------------------------ the C ABI
def test_descriptor_layout_matches_the_header(tmp_path):
    if shutil.which("gcc") is None:
        pytest.skip("no gcc")
    from cm3d_amd import _lib
    S = _lib.BoxPlaceDesc
    names = [n for n, _ in S._fields_]
    assert names == ["size", "place_src", "place_pushed", "ev", "thin"]
    src = tmp_path / "t.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "cm3d_hip.h"\nint main(void) {\n'
                   + "".join(f'printf("%zu\\n", offsetof(cm3d_box_place_desc, {n}));\n' for n in names)
                   + 'printf("%zu\\n", sizeof(cm3d_box_place_desc)); printf("%zu\\n", sizeof(cm3d_lift_pass_options)); return 0; }\n')
    exe = tmp_path / "t"
    r = subprocess.run(["gcc", "-std=c99", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    got = [int(x) for x in subprocess.run([str(exe)], capture_output=True, text=True).stdout.split()]
    assert got[:-1] == [getattr(S, n).offset for n in names] + [ctypes.sizeof(S)]
    assert got[-1] == ctypes.sizeof(_lib.LiftPassOptions) == 40                  # the options did not grow


def test_new_symbols_within_abi_5_and_bad_arguments_never_launch():
    from cm3d_amd import _lib
    L = _lib.lib()
    assert _lib.ABI_VERSION == 5 and L.cm3d_abi_version() == 5
    assert L.cm3d_box_place.argtypes == _lib.SIGNATURES["cm3d_box_place"][1] and len(L.cm3d_box_place.argtypes) == 18
    assert L.cm3d_lift_pass_placed.argtypes == _lib.SIGNATURES["cm3d_lift_pass_placed"][1]
    ref = ctypes.byref
    d, o, y, p = _lib.LiftPassDesc(), _lib.LiftPassOptions(), _lib.YawFitDesc(), _lib.BoxPlaceDesc()
    assert L.cm3d_lift_pass_placed(None, None, None, None) == -1
    d.size, o.size, y.size = ctypes.sizeof(d), ctypes.sizeof(o), ctypes.sizeof(y)
    o.yaw = ctypes.addressof(y)
    assert L.cm3d_lift_pass_placed(ref(d), ref(o), ref(p), None) == -1               # a placement of size 0
    p.size = ctypes.sizeof(p)
    assert L.cm3d_lift_pass_placed(ref(d), ref(o), ref(p), None) == -1               # no outputs
    # cm3d_box_place: a null array, a non-positive size, a bad thin (host memory stands in: nothing may be launched on it)
    a = np.zeros(64)
    q = a.ctypes.data
    ok = [q, q, q, 1, 1, q, q, q, q, q, 1, q, 0, 0.5, 64, q, q, None]
    for k in (0, 1, 2, 5, 6, 7, 8, 9, 11, 15, 16):
        assert L.cm3d_box_place(*[None if i == k else v for i, v in enumerate(ok)]) == -1, k
    for k in (3, 4, 10, 14):
        for v in (0, -1):
            assert L.cm3d_box_place(*[v if i == k else w for i, w in enumerate(ok)]) == -1, k
    for thin in (float("nan"), -1e-300, -1.0, float("inf")):
        assert L.cm3d_box_place(*[thin if i == 13 else w for i, w in enumerate(ok)]) == -1, thin
