"""CPU: the ground strip (cm3d_amd/groundstrip.py, cm3d_ground_grid, cm3d_ground_strip, cm3d_lift_pass_stripped).  The host statements
against a separately written scalar loop on the case tables, bit for bit; what the case tables hold; argument validation and the flags;
two properties of the rule (an in-mask point is a member of its own cell; without estimates the strip is the identity); the geometry of
the rule on a sloped plane against a derived bound; the call sequence of the stripped pass, traced over stubs by a stand-alone program
built with the address and undefined-behaviour sanitizers (tests/pass_strip_sim.cpp) and compared with the sequence include/cm3d_hip.h
states; the ctypes layout of the descriptor."""
import argparse
import ctypes
import functools
import math
import os
import shutil
import subprocess
import tempfile

import numpy as np
import pytest

from cm3d_amd import _lib, groundstrip as gs
from tests import ground_strip_cases as gc
from tests.test_pipe_sched_host import SANITIZED

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def orc():
    from oracle import oracle
    return oracle


@functools.lru_cache(maxsize=None)
def _cases():
    from oracle import oracle
    out = {}
    for case in gc.all_cases():
        out[case["name"]] = (case,) + gc.cloud(oracle, case)
    return out


@pytest.mark.parametrize("name", ["edges", "many"])
def test_host_statement_equals_the_scalar_loop(name):
    case, points, pt_off = _cases()[name]
    xyz, idx, off, mf = gc.lists(case, points)
    for run in case["runs"]:
        e = gc.expected(case, points, pt_off, run)
        lz, ln = gc.loop_grid(points, pt_off, case["origin"], **gc.grid_params(run))
        assert np.array_equal(e["grid_n"], ln) and e["grid_n"].dtype == np.int32, run
        assert np.array_equal(gc.bits(e["grid_z"]), gc.bits(lz)), run
        keep, status, dropped = gc.loop_strip(xyz, off, mf, case["origin"], lz, **gc.strip_params(run))
        assert np.array_equal(e["keep"], keep) and np.array_equal(e["gs_status"], status) and np.array_equal(e["gs_dropped"], dropped), run
        cnt = np.array([keep[off[m]:off[m + 1]].sum() for m in range(len(off) - 1)])
        assert np.array_equal(np.diff(e["gs_off"]), cnt) and np.array_equal(np.diff(e["gs_tile_off"]), (cnt + 63) // 64)
        assert e["gs_off"].dtype == np.int32 and e["gs_status"].dtype == np.int32 and e["gs_dropped"].dtype == np.int32


def test_edges_case_reaches_what_it_is_built_for():
    case, points, pt_off = _cases()["edges"]
    e = gc.expected(case, points, pt_off, {})
    gz, gn = e["grid_z"], e["grid_n"]
    # the identity transform: the cloud is the rows to the bit, the dropped rows NaN
    rows = np.concatenate([s[0] for s in case["sweeps"]], 0)
    fin = np.isfinite(points[:, :3]).all(1)
    assert np.array_equal(points[fin, :3], rows[fin, :3]) and int((~fin).sum()) > 5
    named = 0
    for name, (cell, n, b_star) in case["cells"].items():
        assert gn[0, cell] == n, name
        if b_star is None:
            assert np.isnan(gz[0, cell]), name
        else:
            assert gz[0, cell] == -3.0 + (b_star + 0.5) * gc.DZ, name
        named += n
    assert int(gn[0].sum()) == named                                   # the points at iu, iv = -33 and 32, below and above the window: nowhere
    assert case["cells"]["few_7"][1] == gc.DEFAULTS["min_points"] - 1 and case["cells"]["enough_8"][1] == gc.DEFAULTS["min_points"]
    for name, (cell, n, b_star) in case["frame1_cells"].items():
        assert gn[1, cell] == n and gz[1, cell] == -3.5 + (b_star + 0.5) * gc.DZ, name
    assert int(gn[1].sum()) == 17
    assert not gn[2].any() and np.isnan(gz[2]).all() and not gn[6].any() and np.isnan(gz[6]).all()           # non-finite origins
    f, cell, n, b_star = case["same_xy_frame"]
    assert gn[f, cell] == n and gz[f, cell] == -3.0 + (b_star + 0.5) * gc.DZ and gz[0, cell] != gz[f, cell]
    assert not gn[4].any() and not gn[5].any()                         # no sweep; a sweep without rows
    # the seams of the kernel's tiles lie between cells the case occupies
    occupied = set(np.flatnonzero(gn[0]))
    for i in (15, 31, 47):
        assert gc.cell_index(i - 32, 12) in occupied and gc.cell_index(i + 1 - 32, 12) in occupied
        assert gc.cell_index(13, i - 32) in occupied and gc.cell_index(13, i + 1 - 32) in occupied
    # the lists
    st = dict(zip(case["names"], zip(e["gs_status"].tolist(), e["gs_dropped"].tolist())))
    for name, want in case["lists_expect"].items():
        if want is not None:
            assert st[name] == want, name
    assert st["threshold_03"][0] == 0 and st["threshold_03"][1] in (1, 2)
    e25 = gc.expected(case, points, pt_off, dict(margin=0.25))
    st25 = dict(zip(case["names"], zip(e25["gs_status"].tolist(), e25["gs_dropped"].tolist())))
    assert st25["threshold_025"] == (0, 1)                             # one float32 below g + MARGIN is ground; on it and above it are not
    m = case["names"].index("threshold_025")
    assert np.array_equal(e25["keep"][case["hit_off"][m]:case["hit_off"][m] + 3], [False, True, True])
    lens = {n: int(case["hit_off"][i + 1] - case["hit_off"][i]) for i, n in enumerate(case["names"])}
    assert [lens[f"len_{n}"] for n in (1, 63, 64, 65, 257, 300)] == [1, 63, 64, 65, 257, 300] and lens["empty"] == 0
    for n in (63, 64, 65, 257, 300):
        assert st[f"len_{n}"][0] == 0 and 0 < st[f"len_{n}"][1] < n
    assert set(e["gs_status"].tolist()) == {0, 1, 2}
    assert set(case["mask_frame"].tolist()) >= {-1, 99} and 3 not in set(case["mask_frame"].tolist())      # frame 3 has no list
    # every run changes something
    base = (gc.bits(gz).tobytes(), gn.tobytes(), e["keep"].tobytes(), e["gs_status"].tobytes())
    for run in case["runs"][1:]:
        r = gc.expected(case, points, pt_off, run)
        assert (gc.bits(r["grid_z"]).tobytes(), r["grid_n"].tobytes(), r["keep"].tobytes(), r["gs_status"].tobytes()) != base, run


def test_many_case_reaches_what_it_is_built_for():
    case, points, pt_off = _cases()["many"]
    e = gc.expected(case, points, pt_off, {})
    assert len(case["sweeps"]) == 4 and case["frame_sweep_off"].tolist() == [0, 2, 3, 4]
    assert not np.array_equal(case["sweeps"][0][1], case["sweeps"][1][1])                  # two sweeps, transforms of their own
    assert int((~np.isfinite(points[:, :3]).all(1)).sum()) > 10                            # ego-box rows and padding
    est = np.isfinite(e["grid_z"])
    assert est[0].sum() > 100 and est[1].sum() > 30 and (e["grid_n"][0] > 0).sum() > est[0].sum()
    rows = np.flatnonzero(est[0]) // 64
    cols = np.flatnonzero(est[0]) % 64
    assert rows.min() < 31 and rows.max() > 32 and cols.min() < 31 and cols.max() > 32      # estimates on all four sides of the middle seams
    assert (e["gs_status"] == 0).sum() > 20 and (e["gs_dropped"] > 0).sum() > 20 and int(np.diff(case["hit_off"]).max()) > 256


@pytest.mark.parametrize("name", ["edges", "many"])
def test_an_in_mask_point_is_a_member_of_its_own_cell(name):
    """Every list point that lies inside the grid and the window is a row of its frame's cloud: grid_n >= 1 in its cell."""
    case, points, pt_off = _cases()[name]
    if name == "edges":                                                  # (its lists are not rows of the cloud: the cloud's own rows as one list per frame)
        xyz, mf = points, np.repeat(np.arange(len(pt_off) - 1), np.diff(pt_off))
    else:
        xyz, _, off, m_frame = gc.lists(case, points)
        mf = np.repeat(m_frame, np.diff(off))
    _, gn = gs.ground_grid_host(points, pt_off, case["origin"])
    checked = 0
    for f in range(len(pt_off) - 1):
        o = case["origin"][f]
        if not np.isfinite(o).all():
            continue
        p = xyz[mf == f]
        p = p[np.isfinite(p[:, :3]).all(1)]
        inside, idx = gs.cells(p[:, 0], p[:, 1], o, 2.0)
        t = (p[:, 2].astype(np.float64) - (o[2] - 4.0)) / 0.125
        sel = inside & (t >= 0) & (t < 64)
        assert (gn[f, idx[sel]] >= 1).all()
        checked += int(sel.sum())
    assert checked > 300


@pytest.mark.parametrize("name", ["edges", "many"])
def test_without_estimates_the_strip_is_the_identity(name):
    case, points, pt_off = _cases()[name]
    xyz, idx, off, mf = gc.lists(case, points)
    e = gc.expected(case, points, pt_off, dict(min_points=10 ** 6, min_keep=1))
    assert np.isnan(e["grid_z"]).all() and e["grid_n"].any()
    assert e["gs_off"].tobytes() == off.tobytes() and e["gs_xyz"].tobytes() == xyz.tobytes() and e["gs_idx"].tobytes() == idx.tobytes()
    assert not e["gs_dropped"].any() and np.array_equal(e["gs_status"], np.where(np.diff(off) == 0, 2, 0))


# ------------------------------------------------------------------------------------------------ arguments and flags
def test_argument_validation():
    nan, inf = float("nan"), float("inf")
    bad = [dict(cell=0.0), dict(cell=-1.0), dict(cell=nan), dict(cell=inf), dict(down=0.0), dict(down=nan), dict(down=inf), dict(up=0.0),
           dict(up=-1.0), dict(up=nan), dict(quantile=-0.1), dict(quantile=1.1), dict(quantile=nan), dict(min_points=0), dict(min_points=2.5),
           dict(margin=nan), dict(margin=inf), dict(margin=-inf), dict(min_keep=0), dict(min_keep=1.5)]
    for kw in bad:
        with pytest.raises(ValueError):
            gs.GroundStrip(**kw)
    g = gs.GroundStrip()
    assert g.active and g.params() == gc.DEFAULTS
    assert gs.GroundStrip(margin=-0.2, quantile=0.0, min_points=1, min_keep=1).margin == -0.2
    with pytest.raises(ValueError):
        gs.ground_grid_host(np.zeros((4, 4), np.float32), [0, 4], np.zeros((1, 3)), cell=0.0)
    with pytest.raises(ValueError):
        gs.ground_grid_host(np.zeros((4, 4), np.float32), [0, 4], np.zeros((2, 3)))
    with pytest.raises(ValueError):
        gs.ground_strip_host(np.zeros((4, 3), np.float32), np.zeros(3), None, min_keep=0)
    assert _lib.GROUND_GRID_CELLS == gc.CELLS == 64 and _lib.GROUND_GRID_BINS == gc.BINS == 64
    header = open(os.path.join(ROOT, "include", "cm3d_hip.h")).read()
    assert "#define CM3D_GROUND_GRID_CELLS 64" in header and "#define CM3D_GROUND_GRID_BINS 64" in header
    assert "#define CM3D_ABI_VERSION 5" in header


def _parser():
    ap = argparse.ArgumentParser()
    gs.add_arguments(ap)
    return ap


def test_flags():
    ap = _parser()
    assert gs.from_namespace(ap.parse_args([]), ap) is None
    assert gs.from_namespace(ap.parse_args(["--ground-strip", "off"]), ap) is None
    assert gs.from_namespace(ap.parse_args(["--ground-strip", "grid"]), ap) == gs.GroundStrip()
    g = gs.from_namespace(ap.parse_args(["--ground-strip", "grid", "--ground-strip-cell", "1.5", "--ground-strip-window", "3,2.5",
                                         "--ground-strip-quantile", "0.2", "--ground-strip-min-points", "4", "--ground-strip-margin", "0.1",
                                         "--ground-strip-min-keep", "9"]), ap)
    assert g == gs.GroundStrip(1.5, 3.0, 2.5, 0.2, 4, 0.1, 9)
    for flag, value in (("--ground-strip-cell", "1"), ("--ground-strip-window", "1,1"), ("--ground-strip-quantile", "0.5"),
                        ("--ground-strip-min-points", "3"), ("--ground-strip-margin", "0.2"), ("--ground-strip-min-keep", "2")):
        with pytest.raises(SystemExit):
            gs.from_namespace(ap.parse_args([flag, value]), ap)                 # a --ground-strip-* flag without --ground-strip grid
        with pytest.raises(ValueError):
            gs.from_namespace(ap.parse_args(["--ground-strip", "off", flag, value]))
    for args in (["--ground-strip-window", "3"], ["--ground-strip-window", "a,b"], ["--ground-strip-cell", "0"], ["--ground-strip-min-keep", "0"]):
        with pytest.raises(SystemExit):
            gs.from_namespace(ap.parse_args(["--ground-strip", "grid"] + args), ap)
    with pytest.raises(SystemExit):
        ap.parse_args(["--ground-strip", "fit"])


def test_entry_points_take_the_flags():
    """Both nuScenes scripts run pipeline_nuscenes.main and the Waymo script pipeline_waymo.main: those take the flags; KITTI does not."""
    read = lambda *parts: open(os.path.join(ROOT, *parts)).read()
    assert "pipeline_nuscenes import main" in read("src", "nuscenes", "2d_to_3d.py") and "pipeline_nuscenes import main" in read("src", "nuscenes", "2d_to_3d_new.py")
    assert "pipeline_waymo import main" in read("src", "waymo", "2d_to_3d.py")
    for mod in ("pipeline_nuscenes.py", "pipeline_waymo.py"):
        text = read("cm3d_amd", mod)
        assert "gsmod.add_arguments(ap)" in text and "gsmod.from_namespace(args, ap)" in text and "strip=strip" in text, mod
    assert "groundstrip" not in read("cm3d_amd", "pipeline_kitti.py") and "ground-strip" not in read("cm3d_amd", "pipeline_kitti.py")


def test_descriptor_layout():
    d = _lib.GroundStripDesc
    assert ctypes.sizeof(d) == 160 and d.size.offset == 0 and d.origin.offset == 8 and d.ws_bytes.offset == 88 and d.ev.offset == 96
    assert d.cell.offset == 112 and d.margin.offset == 144 and d.min_points.offset == 152 and d.min_keep.offset == 156
    for name in ("cm3d_ground_strip_check", "cm3d_ground_grid", "cm3d_ground_strip_workspace_bytes", "cm3d_ground_strip", "cm3d_lift_pass_stripped"):
        assert name in _lib.SIGNATURES


# ------------------------------------------------------------------------------------------------ the geometry of the rule
SLOPES = [(0.0, (1.0, 0.0)), (0.03, (1.0, 0.0)), (0.03, (0.0, 1.0)), (0.03, (math.sqrt(0.5), math.sqrt(0.5))), (0.1, (1.0, 0.0)),
          (0.1, (0.0, 1.0)), (0.1, (math.sqrt(0.5), math.sqrt(0.5)))]


@pytest.mark.parametrize("s,d", SLOPES)
def test_geometry_on_a_sloped_plane(s, d):
    """A noise-free ring pattern on the plane z = -1.84 + s d . (x, y) (d a unit vector) around the origin 0, 0, 0, and a box-shaped
    object of 4 x 2 x 1.6 m standing on it (the plane's points under it stay: the rule is under test, not the occlusion, and so no cell is
    the object's alone); one list: the object's points and the plane's points within a metre of its footprint.

    The bound.  Take a cell with an estimate g, C its side.  Its plane members have heights in [lo, hi] with hi - lo <= s C (|d_x| + |d_y|)
    <= sqrt(2) s C, and every member, the object's included, lies at or above the plane at its own x, y, so at or above lo.  Let n_p be
    the plane members.  k = (int)(Q (n - 1)) < n_p whenever the object's share of the n members is below 1 - Q (asserted), so the member
    of rank k lies in [lo, hi], and g, the centre of its bin, in [lo - dz / 2, hi + dz / 2].  A plane point of the cell, at most hi high,
    is dropped iff its z < g + MARGIN; g + MARGIN >= lo - dz / 2 + MARGIN, so MARGIN > sqrt(2) s C + dz / 2 drops every one.  An object point
    h above the plane stands at least lo + h high and is kept iff its z >= g + MARGIN, which h >= MARGIN + sqrt(2) s C + dz / 2 guarantees.
    The coordinates are float32 roundings of these (relative 2^-24 of some ten metres): 1e-4 m is added to both bounds."""
    C, dz, Q = 2.0, 0.125, 0.1
    bound = math.sqrt(2.0) * s * C + dz / 2 + 1e-4
    margin = max(0.3, bound + 0.02)
    plane = lambda x, y: -1.84 + s * (d[0] * x + d[1] * y)
    a = np.linspace(-np.pi, np.pi, 720, endpoint=False)
    radii = np.arange(3.0, 24.0, 0.25)
    x = np.concatenate([r * np.cos(a + 0.003 * i) for i, r in enumerate(radii)])
    y = np.concatenate([r * np.sin(a + 0.003 * i) for i, r in enumerate(radii)])
    cx, cy, L, W, H = 10.3, 3.1, 4.0, 2.0, 1.6
    ground = np.stack([x, y, plane(x, y)], 1)
    u, v, h = np.arange(-L / 2, L / 2 + 1e-9, 0.2), np.arange(-W / 2, W / 2 + 1e-9, 0.2), np.arange(0.05, H + 1e-9, 0.1)
    face_a = np.array([(cx + uu, cy - W / 2, hh) for uu in u for hh in h])
    face_b = np.array([(cx - L / 2, cy + vv, hh) for vv in v for hh in h])
    top = np.array([(cx + uu, cy + vv, H) for uu in u for vv in v])
    obj = np.concatenate([face_a, face_b, top], 0)
    obj_h = obj[:, 2].copy()
    obj[:, 2] += plane(obj[:, 0], obj[:, 1])
    pts = np.zeros((len(ground) + len(obj), 4), np.float32)
    pts[:, :3] = np.concatenate([ground, obj], 0)
    is_obj = np.arange(len(pts)) >= len(ground)
    origin = np.zeros((1, 3))
    gz, gn = gs.ground_grid_host(pts, [0, len(pts)], origin)
    inside, cell = gs.cells(pts[:, 0], pts[:, 1], origin[0], C)
    assert inside.all()
    share = np.bincount(cell[is_obj], minlength=gs.N_CELLS) / np.maximum(gn[0], 1)
    assert share.max() < 1.0 - Q and share.max() > 0.2                  # the object's share of every occupied cell's members
    foot = (np.abs(pts[:, 0] - cx) < L / 2 + 1.0) & (np.abs(pts[:, 1] - cy) < W / 2 + 1.0)
    sel = np.flatnonzero(is_obj | foot)
    assert np.isfinite(gz[0, cell[sel]]).all() and 100 < int((~is_obj[sel]).sum())          # every cell of the list has an estimate
    keep, status, dropped = gs.ground_strip_host(pts[sel, :3], origin[0], gz[0], C, margin, 5)
    assert status == gs.ST_STRIPPED and dropped == int((~keep).sum())
    assert margin > bound and not keep[~is_obj[sel]].any()              # every plane point of the list is dropped
    high = obj_h[sel[is_obj[sel]] - len(ground)] >= margin + bound
    assert high.sum() > 100 and keep[is_obj[sel]][high].all()           # every object point that high above the plane is kept
    assert not keep[is_obj[sel]].all() or margin + bound < 0.05         # (the object's lowest points go with the road)


# ------------------------------------------------------------------------------------------------ the stripped pass's sequence
CODE = {"cm3d_lift_pass_head": -2, "cm3d_lift_pass_tail": -2, "record": -2, "cm3d_ground_grid": -3, "cm3d_ground_strip": -3, "cm3d_depth_cluster": -3,
        "cm3d_stage2_filter": -2, "cm3d_bev_fit": -1, "cm3d_yaw_select": -3, "cm3d_box_nms_bounded": -2, "cm3d_box_place": -3,
        "cm3d_box_rotated_nms": -3}


@functools.lru_cache(maxsize=None)
def _run_sim():
    tmp = tempfile.mkdtemp(prefix="pass_strip_sim")
    try:
        exe = os.path.join(tmp, "pass_strip_sim")
        rocm = os.environ.get("ROCM_PATH", "/opt/rocm")
        r = subprocess.run(SANITIZED + ["-D__HIP_PLATFORM_AMD__", "-isystem", os.path.join(rocm, "include"), os.path.join(ROOT, "tests", "pass_strip_sim.cpp"),
                                        os.path.join(ROOT, "cm3d_amd", "csrc", "pass_compose.cpp"), os.path.join(ROOT, "cm3d_amd", "csrc", "pass_options.cpp"),
                                        "-o", exe], capture_output=True, text=True)
        assert r.returncode == 0, r.stderr
        r = subprocess.run([exe], capture_output=True, text=True)            # its own executable: the sanitizers' runtimes are linked in
        assert r.returncode == 0 and r.stdout.endswith("pass_strip_sim done\n"), r.stdout + r.stderr
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


def stripped_sequence(c, f, y, p, n, waymo=False, idx=True, cloud=False, ev=True):
    """include/cm3d_hip.h's statement of cm3d_lift_pass_stripped for one presence combination."""
    rec = lambda e: [f"record {e:#x}"]
    hi, gi, ci = ("hit_idx", "gs_idx", "cl_idx") if idx else ("null", "null", "null")
    part = lambda name, off, tile, i, xyz, work: f"{name} hit_off={off} tile_off={tile} hit_idx={i} hit_xyz={xyz} tile_work={work}"
    out = [part("cm3d_lift_pass_head", "hit_off", "tile_off", hi, "hit_xyz", "tile_work")] + (rec(0x30) if ev else [])
    out += [f"cm3d_ground_grid cloud={'points,pt_off' if cloud else 'null,null'} raw=raw,5 rest=set n=6,5000,3 halfw=1.5 origin=ego par=2,4,3,0.1,8 "
            "out=grid_z,grid_n",
            f"cm3d_ground_strip in=hit_xyz,{hi},hit_off frame=set n=7,4096,3 origin=ego grid=grid_z par=2,0.3,5 "
            f"out=gs_off,gs_tile_off,{gi},gs_xyz,gs_status,gs_dropped ws=gs_ws,16"] + (rec(0x31) if ev else [])
    lists = "gs_xyz,gs_off"
    if c:
        out += rec(0x50) + [f"cm3d_depth_cluster in=gs_xyz,{gi},gs_off origin=origin out=cl_off,cl_tile_off,{ci},cl_xyz,cl_status ws=cl_ws"] + rec(0x51)
        out += [part("cm3d_lift_pass_tail", "cl_off", "cl_tile_off", "cl_idx", "cl_xyz", "null")]
        lists = "cl_xyz,cl_off"
    else:
        out += [part("cm3d_lift_pass_tail", "gs_off", "gs_tile_off", gi, "gs_xyz", "null")]
    pos = "kept" if f else "medoid_pos"
    if f:
        out += rec(0x40) + ["cm3d_stage2_filter pos=medoid_pos out=kept"] + rec(0x41) + ["cm3d_box_nms_bounded pos=kept lane=lane out=box,flags"]
    if y:
        out += rec(0x60) + [f"cm3d_bev_fit in={lists} out=fit_rect", f"cm3d_yaw_select pos={pos} out=yaw_tab"] + rec(0x61)
        out += [f"cm3d_box_nms_bounded pos={pos} lane=yaw_tab out=box,flags"]
    if p:
        out += rec(0x70) + [f"cm3d_box_place io=box,flags in=fit_rect,yaw_src waymo={int(waymo)} thin=0.5 out=place_src,place_pushed"] + rec(0x71)
    if n:
        out += [f"cm3d_box_rotated_nms io=box,flags waymo={int(waymo)}"]
    return out


def assert_pass(trace, want, name):
    calls, rc, fails = trace
    assert calls == want, (name, calls, want)
    assert rc == [0], name
    assert fails == [(k, CODE[c.split()[0]], k + 1) for k, c in enumerate(calls)], name


def test_stripped_pass_sequence():
    got = sim()
    seen = 0
    for m in range(32):
        c, f, y, p, n = bool(m & 1), bool(m & 2), bool(m & 4), bool(m & 8), bool(m & 16)
        if p and not y:
            continue
        name = "combo." + "".join(ch if on else "-" for ch, on in zip("cfypn", (c, f, y, p, n)))
        assert_pass(got[name], stripped_sequence(c, f, y, p, n), name)
        seen += 1
    assert seen == 24
    assert_pass(got["combo_waymo.cfypn"], stripped_sequence(True, True, True, True, True, waymo=True), "waymo")
    assert_pass(got["ok.null_opt"], stripped_sequence(False, False, False, False, False), "null opt")
    assert_pass(got["ok.cloud"], stripped_sequence(False, False, False, False, False, cloud=True), "cloud")
    assert_pass(got["ok.no_events"], stripped_sequence(True, False, False, False, False, ev=False), "no events of the strip's")
    want = stripped_sequence(True, False, False, False, False, idx=False)
    want[-1] = want[-1].replace("hit_idx=cl_idx", "hit_idx=null")
    assert_pass(got["ok.without_idx"], want, "without idx")
    assert_pass(got["rule.gs_lists"], stripped_sequence(False, False, True, False, False), "the fit's own statement of the stripped lists")
    assert_pass(got["rule.cl_lists"], stripped_sequence(True, True, True, False, False), "the fit's own statement of the clustered lists")


def test_stripped_pass_makes_no_call_on_a_bad_descriptor():
    got = sim()
    bad = {k: v for k, v in got.items() if k.startswith("bad.") or k in ("rule.raw_xyz_behind_strip", "rule.gs_off_behind_cluster")}
    assert len(bad) == 14 + 10 + 12 + 2
    for name, trace in bad.items():
        assert trace == ([], [-1], []), name                             # CM3D_ERR_ARG and no call at all
    assert not any("descriptor was changed" in line for t in got.values() for line in t[0])
