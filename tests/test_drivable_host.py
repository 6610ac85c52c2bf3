"""CPU: the host side of the drivable-area test and of the stage-2 filters (cm3d_amd/drivable.py, csrc/pass_options.cpp).  The y-slab
index and the walk the kernel makes through it, restated in numpy, against eval_detection.point_in_polygons on the cases of
tests/drivable_cases.py; the index invariant; the filter rule on hand-written rows; the new descriptor's layout; and the call sequence
of cm3d_lift_pass_filtered, traced over stubs by a stand-alone program built with the address and undefined-behaviour sanitizers."""
import ctypes
import os
import shutil
import subprocess

import numpy as np
import pytest

from cm3d_amd import drivable, eval_detection as ev
from cm3d_amd.lifting import ClassTable
from tests import drivable_cases as dc
from tests import pass_options_trace as T

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.parametrize("name", dc.CASE_NAMES)
def test_query_through_the_index_equals_brute_force(name):
    c = dc.all_cases()[name]
    exp = dc.expected(name)
    got = drivable.query_index(drivable.build_index(c["tables"]), c["xy"], c["table"])
    assert np.array_equal(got, exp), f"{name}: {np.flatnonzero(got != exp)[:8]}"
    if name != "H_slab_edges":
        assert exp.any() and not exp.all(), name            # the case says something about both answers


def test_cases_are_what_they_claim():
    cases = dc.all_cases()
    assert list(cases) == dc.CASE_NAMES
    for c in cases.values():
        assert c["xy"].dtype == np.float64 and c["table"].dtype == np.int32 and c["xy"].shape == (c["table"].size, 2)
        assert np.abs(c["xy"]).max() > 600 and np.any(c["xy"] != np.round(c["xy"]))
    # F: a ray through the teeth crosses 2 T edges of ONE ring inside one slab, and ring boundaries fall on lanes 63 / 64 of a chunk
    for t in dc.COMB_TEETH:
        c = cases[f"F_comb_{t}"]
        ix = drivable.build_index(c["tables"])
        ymin, ymax, per_y = ix["tab_y"][0]
        s = int(drivable.slab_of(dc.COMB_RAY_Y, ymin, per_y, int(ix["tab_slab"][0, 1])))
        rings = ix["ent_ring"][ix["slab_off"][s]:ix["slab_off"][s + 1]]
        e = ix["edge"][ix["ent_edge"][ix["slab_off"][s]:ix["slab_off"][s + 1]]]
        crossing = (e[:, 1] > dc.COMB_RAY_Y) != (e[:, 3] > dc.COMB_RAY_Y)
        assert np.bincount(rings[crossing]).max() == 2 * t
        assert np.any(dc.comb_ring_seams(c["tables"][0]) % 64 == 0), t
        assert np.any(c["xy"][:, 1] == dc.COMB_RAY_Y)
    j = cases["J_city"]
    ext, holes = j["tables"][0][0]
    assert 19000 <= ext.shape[0] <= 21000 and len(holes) == 50 and j["xy"].shape[0] == 4096
    assert len(cases["I_three_tables"]["tables"]) == 3 and cases["I_three_tables"]["tables"][1] == []
    # G: the big rectangle's two long edges are listed in every slab
    ix = drivable.build_index(cases["G_big_rectangle"]["tables"])
    n = int(ix["tab_slab"][0, 1])
    for k in (1, 3):
        assert np.array_equal(np.unique(np.repeat(np.arange(n), np.diff(ix["slab_off"][:n + 1]))[ix["ent_edge"] == k]), np.arange(n))


@pytest.mark.parametrize("name", dc.CASE_NAMES)
def test_every_edge_is_listed_in_every_slab_its_y_interval_touches(name):
    c = dc.all_cases()[name]
    ix = drivable.build_index(c["tables"])
    assert ix["slab_off"][0] == 0 and np.all(np.diff(ix["slab_off"]) >= 0) and ix["slab_off"][-1] == ix["ent_edge"].size
    e0 = r0 = 0
    for t, polygons in enumerate(c["tables"]):
        rings = drivable.table_rings(polygons)
        s0, n = (int(v) for v in ix["tab_slab"][t])
        if not rings:
            assert n == 0
            continue
        E = sum(r.shape[0] for r, _ in rings)
        edges = ix["edge"][e0:e0 + E]
        ymin, ymax, per_y = ix["tab_y"][t]
        assert ymin == min(r[:, 1].min() for r, _ in rings) and ymax == max(r[:, 1].max() for r, _ in rings)
        listed = np.zeros((n, E), bool)
        slab = np.repeat(np.arange(n), np.diff(ix["slab_off"][s0:s0 + n + 1]))
        sl = slice(int(ix["slab_off"][s0]), int(ix["slab_off"][s0 + n]))
        listed[slab, ix["ent_edge"][sl] - e0] = True
        # inside a slab: ascending edges (so rings, and the rings of a polygon, are neighbours), the ring of an entry is its edge's
        ring_of_edge = np.repeat(np.arange(len(rings)), [r.shape[0] for r, _ in rings]) + r0
        assert np.array_equal(ix["ent_ring"][sl], ring_of_edge[ix["ent_edge"][sl] - e0])
        same_slab = np.diff(slab) == 0
        assert np.all(np.diff(ix["ent_edge"][sl])[same_slab] > 0)
        assert np.array_equal(ix["ring_info"][r0:r0 + len(rings)], [info for _, info in rings])
        # the slabs as real intervals [ymin + k / per_y, ymin + (k + 1) / per_y], and the slab the kernel's expression gives
        lo, hi = np.minimum(edges[:, 1], edges[:, 3]), np.maximum(edges[:, 1], edges[:, 3])
        for k in range(n):
            a = ymin + k / per_y if per_y else ymin
            b = ymin + (k + 1) / per_y if per_y else ymax
            touches = (hi >= a) & (lo <= b)
            assert np.all(listed[k][touches]), (name, t, k)
        for y in (lo, hi, (lo + hi) / 2):
            assert np.all(listed[drivable.slab_of(y, ymin, per_y, n), np.arange(E)])
        e0, r0 = e0 + E, r0 + len(rings)


def test_index_sizes_are_checked_on_the_host():
    ring = dc._rect(0.5, 0.5, 10.5, 1e6)
    with pytest.raises(ValueError, match="2\\^31"):       # 4 edges, two of them over 65536 slabs, forced a few 10^4 times over
        drivable.build_index([[(np.tile(ring, (20000, 1)), [])]], edges_per_slab=1)
    with pytest.raises(ValueError, match="finite"):
        drivable.build_index([[(np.array([(0, 0), (1, np.inf), (2, 0)], np.float64), [])]])
    empty = drivable.build_index([])
    assert empty["n_tables"] == 0 and empty["slab_off"].tolist() == [0]
    flat = drivable.build_index([[(np.array([(0, 5.5), (1, 5.5), (2, 5.5)], np.float64), [])]])
    assert flat["tab_slab"].tolist() == [[0, 1]] and flat["tab_y"][0, 2] == 0.0
    assert drivable.query_index(flat, [(1.0, 5.5), (1.0, 5.6)], [0, 0]).tolist() == [0, 0]


def test_filter_rule_rows():
    cls = ClassTable.nuscenes()
    assert [n for n, r in zip(cls.names, cls.needs_road) if r] == ["car", "truck", "bus"]
    assert ClassTable.waymo().needs_road.tolist() == cls.needs_road.tolist()
    ci = cls.index
    rows = [   # class, medoid_pos, lane_dist, on_road -> kept with (drivable, lane 20, vehicle 4)
        ("car", 5, 1.0, 1, 5), ("car", 5, 1.0, 0, -1), ("truck", 0, 3.9, 0, -1), ("bus", 2, 0.0, 0, -1),
        ("construction_vehicle", 3, 1.0, 0, 3), ("trailer", 3, 1.0, 0, 3), ("barrier", 3, 1.0, 0, 3), ("pedestrian", 7, 19.0, 0, 7),
        ("car", 5, 4.0, 1, 5), ("car", 5, np.nextafter(4.0, 5.0), 1, -1), ("barrier", 1, 4.5, 1, -1), ("trailer", 1, 4.0, 1, 1),
        ("pedestrian", 1, 20.0, 1, 1), ("pedestrian", 1, np.nextafter(20.0, 21.0), 1, -1), ("bicycle", 4, 25.0, 1, -1),
        ("traffic_cone", 4, 4.5, 0, 4), ("car", -1, np.inf, 0, -1), ("pedestrian", -1, np.inf, 0, -1), ("motorcycle", 0, np.nan, 0, 0),
    ]
    c = np.array([ci(r[0]) for r in rows])
    med, ld, on, want = (np.array([r[k] for r in rows]) for k in (1, 2, 3, 4))
    got = drivable.filter_rule(med, c, ld, on, cls.is_vehicle, cls.needs_road, 20.0, 4.0)
    assert got.dtype == np.int32 and got.tolist() == want.tolist()
    # no polygons: no road test; thresholds at +inf: off
    assert drivable.filter_rule(med, c, ld, None, cls.is_vehicle, cls.needs_road).tolist() == med.tolist()
    only_lane = drivable.filter_rule(med, c, ld, None, cls.is_vehicle, cls.needs_road, 20.0)
    assert np.array_equal(only_lane == -1, (med < 0) | (ld > 20.0))
    only_road = drivable.filter_rule(med, c, ld, on, cls.is_vehicle, cls.needs_road)
    assert np.array_equal(only_road == -1, (med < 0) | (np.isin(c, [ci("car"), ci("truck"), ci("bus")]) & (on == 0)))
    f = drivable.Stage2Filters
    assert not f().active and f(drivable=True).active and f(lane_max_dist=20).active and f(vehicle_lane_max_dist=4).active
    assert f.from_args(False, None, None) is None and f.from_args(False, None, 4).vehicle_lane_max_dist == 4.0
    with pytest.raises(ValueError):
        f(lane_max_dist=float("nan"))


def test_point_in_polygons_reference_is_per_ring_and_per_polygon():
    """What the cases rest on: the host reference itself gives the answers a sum of parities would not."""
    c = dc.all_cases()["C_overlap"]
    a = c["tables"][0][0][0]
    mid = a.mean(0)
    assert ev.point_in_polygons(c["tables"][0], *mid) and ev.point_in_polygons(c["tables"][0][:1], *mid)


def test_filter_descriptor_layout_matches_the_header(tmp_path):
    if shutil.which("gcc") is None:
        pytest.skip("no gcc")
    from cm3d_amd import _lib
    names = [n for n, _ in _lib.Stage2FilterDesc._fields_]
    src = tmp_path / "t.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "cm3d_hip.h"\nint main(void) {\n'
                   + "".join(f'printf("%zu\\n", offsetof(cm3d_stage2_filter_desc, {n}));\n' for n in names)
                   + 'printf("%zu\\n", sizeof(cm3d_stage2_filter_desc)); return 0; }\n')
    exe = tmp_path / "t"
    r = subprocess.run(["gcc", "-std=c99", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    got = [int(x) for x in subprocess.run([str(exe)], capture_output=True, text=True).stdout.split()]
    assert got == [getattr(_lib.Stage2FilterDesc, n).offset for n in names] + [ctypes.sizeof(_lib.Stage2FilterDesc)]
    assert tuple(names[1:8]) == _lib.POLY_INDEX_ARRAYS == drivable.INDEX_ARRAYS


def test_new_symbols_within_abi_5_and_bad_arguments_never_launch():
    from cm3d_amd import _lib
    L = _lib.lib()
    assert _lib.ABI_VERSION == 5 and L.cm3d_abi_version() == 5
    f = _lib.Stage2FilterDesc()
    d = _lib.LiftPassDesc()
    assert L.cm3d_lift_pass_filtered(None, None, None) == -1
    assert L.cm3d_lift_pass_filtered(ctypes.byref(d), ctypes.byref(f), None) == -1          # size not filled
    f.size = ctypes.sizeof(f)
    assert L.cm3d_lift_pass_filtered(ctypes.byref(d), ctypes.byref(f), None) == -1          # no outputs
    assert L.cm3d_points_in_polygons(None, None, 5, None, None, None, None, None, None, None, 1, None, None) == -1
    assert L.cm3d_points_in_polygons(None, None, -1, None, None, None, None, None, None, None, 1, None, None) == -1
    assert L.cm3d_stage2_filter(*([None] * 6), 4, 1, *([None] * 7), 0, None, None, 10, 20.0, 4.0, None, None, None) == -1


FILTERED_CASES = {"lanes_only": dict(bound=32), "polygons": dict(polygons=True, tables=2, bound=32), "events": dict(ev=0x40, bound=32),
                  "pose_planes": dict(bound=96, pose_inv="pose_inv"), "planes_32": dict(bound=1024, pose_inv="pose_inv")}


def test_filtered_pass_sequence_under_sanitizers():
    """cm3d_lift_pass_filtered over stubs (tests/pass_options_sim.cpp): the plain pass, the filter on the pass's medoid positions, the
    boxes again on the kept ones, in that order and with the events around the filter; a descriptor of another size, one without
    outputs or a null pointer makes no call; and whichever call fails, the pass ends there with that call's error."""
    got = T.group("filter")
    for name in ("wrong_size", "no_output", "no_on_road", "null_pass", "null_filter"):
        T.assert_refused(got.pop(name), name)
    assert set(got) == set(FILTERED_CASES)
    for name, kw in FILTERED_CASES.items():
        T.assert_pass(got[name], T.plain_sequence() + T.filter_sequence(**kw), name)


def test_pipeline_cpp_and_the_kernels_do_not_know_the_filtered_pass():
    """The hard constraint of the design: the plain pass links without the new entry points (tests/lift_pass_sim.cpp's stubs)."""
    src = open(os.path.join(ROOT, "cm3d_amd", "csrc", "pipeline.cpp")).read()
    assert "stage2_filter" not in src and "lift_pass_filtered" not in src and "points_in_polygons" not in src
