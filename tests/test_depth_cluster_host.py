"""CPU: the host side of the depth clustering (cm3d_amd/cluster.py, csrc/pass_options.cpp).  The host statement -- sort by (range,
position), boundaries where neighbours lie more than eps apart -- against the O(n^2) connected components of "|ri - rj| <= eps" on the
hand-written rows and the random recipe of tests/depth_cluster_cases.py; DepthCluster's argument checks; the new descriptor's layout;
and the call sequence of cm3d_lift_pass_clustered, traced over stubs by a stand-alone program built with the address and
undefined-behaviour sanitizers."""
import ctypes
import os
import shutil
import subprocess

import numpy as np
import pytest

from cm3d_amd import cluster
from tests import depth_cluster_cases as cases
from tests import pass_options_trace as T

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.parametrize("name", list(cases.crafted()))
def test_crafted_rows(name):
    xyz, o, eps, mp, want = cases.crafted()[name]
    for pick in cluster.PICKS:
        keep, st = cluster.depth_cluster_host(xyz, cases.ORIGINS[o], eps, mp, pick)
        bkeep, bst = cases.brute_force(xyz, cases.ORIGINS[o], eps, mp, pick)
        assert keep.dtype == bool and np.array_equal(keep, bkeep) and st == bst, (name, pick)
        if want is not None and pick in want:
            assert (np.flatnonzero(keep).tolist(), st) == want[pick], (name, pick)
        assert keep.any()                                    # a non-empty list never becomes empty


def test_crafted_rows_are_what_they_claim():
    rows = cases.crafted()
    h = lambda name, pick: cluster.depth_cluster_host(rows[name][0], cases.ORIGINS[rows[name][1]], rows[name][2], rows[name][3], pick)
    r = lambda name: cluster.ranges(rows[name][0], cases.ORIGINS[rows[name][1]])
    # the same four ranges up to one point: joined at a gap of exactly eps, split when the gap is eps plus one ulp
    assert rows["gap_eps_plus_ulp_splits"][2] < 1.0 and np.nextafter(rows["gap_eps_plus_ulp_splits"][2], 2.0) == 1.0
    assert 1.0 in np.diff(np.sort(r("gap_equals_eps_joins"))) and 1.0 in np.diff(np.sort(r("gap_eps_plus_ulp_splits")))
    assert np.unique(r("duplicates")).size == 2
    # the tie: two clusters of 25, the nearer one kept by both picks
    keep, _ = h("size_tie_goes_to_nearest", "largest")
    rr = r("size_tie_goes_to_nearest")
    assert keep.sum() == 25 and rr[keep].max() < 13 and (rr > 25).sum() == 25
    # the largest lies farthest: the picks differ
    kl, kn = h("largest_is_last_in_range", "largest")[0], h("largest_is_last_in_range", "nearest")[0]
    rr = r("largest_is_last_in_range")
    assert kl.sum() == 30 and rr[kl].min() > 40 and kn.sum() == 21 and rr[kn].max() < 9
    assert h("no_cluster_qualifies", "largest")[1] == cluster.KEPT_WHOLE
    sizes = {k: int(h(f"cluster_of_{k}", "largest")[0].sum()) for k in (19, 20, 21)}
    stat = {k: h(f"cluster_of_{k}", "nearest")[1] for k in (19, 20, 21)}
    assert sizes == {19: 24, 20: 20, 21: 21} and stat == {19: 1, 20: 0, 21: 0}
    keep, st = h("far_origin", "largest")
    assert st == 0 and keep.sum() == 24 and np.abs(rows["far_origin"][0]).max() >= 1600
    assert cluster.depth_cluster_host(np.zeros((0, 3), np.float32), [0, 0, 0], 1.0)[1] == cluster.EMPTY


@pytest.mark.parametrize("pick", cluster.PICKS)
def test_random_lists_equal_brute_force(pick):
    lists = cases.random_lists(11, 400)
    subset = whole = 0
    for xyz, o in lists:
        keep, st = cluster.depth_cluster_host(xyz, cases.ORIGINS[o], cases.EPS, cases.MIN_POINTS, pick)
        bkeep, bst = cases.brute_force(xyz, cases.ORIGINS[o], cases.EPS, cases.MIN_POINTS, pick)
        assert np.array_equal(keep, bkeep) and st == bst
        subset += int(st == 0 and not keep.all())
        whole += int(st == 1)
    print(f"{pick}: strict subsets {subset / len(lists):.2f}, kept whole {whole / len(lists):.2f}")
    assert subset >= 0.25 * len(lists) and whole >= 0.10 * len(lists)         # otherwise the recipe shows nothing


def test_depth_cluster_arguments():
    D = cluster.DepthCluster
    d = D(1)
    assert (d.eps, d.min_points, d.pick, d.pick_index, d.active) == (1.0, 20, "largest", 0, True)
    assert D(float("inf"), 1, "nearest").pick_index == 1 and D(0.5, pick=1).pick == "nearest"
    for bad in (dict(eps=0), dict(eps=-1), dict(eps=float("nan")), dict(eps=1, min_points=0), dict(eps=1, min_points=2.5),
                dict(eps=1, pick="middle"), dict(eps=1, pick=2)):
        with pytest.raises(ValueError):
            D(**bad)
    assert D.from_args(None, 20, "largest") is None
    got = D.from_args(2.0, 5, "nearest")
    assert (got.eps, got.min_points, got.pick) == (2.0, 5, "nearest")
    import argparse
    ap = argparse.ArgumentParser()
    cluster.add_arguments(ap)
    assert cluster.from_namespace(ap.parse_args([])) is None
    c = cluster.from_namespace(ap.parse_args(["--depth-cluster", "1", "--depth-cluster-min-points", "7", "--depth-cluster-pick", "nearest"]))
    assert (c.eps, c.min_points, c.pick) == (1.0, 7, "nearest")
    for bad in (dict(eps=0.0), dict(eps=float("nan")), dict(min_points=0)):
        with pytest.raises(ValueError):
            cluster.depth_cluster_host(np.zeros((2, 3), np.float32), [0, 0, 0], **{"eps": 1.0, **bad})


def test_cluster_descriptor_layout_matches_the_header(tmp_path):
    if shutil.which("gcc") is None:
        pytest.skip("no gcc")
    from cm3d_amd import _lib
    names = [n for n, _ in _lib.DepthClusterDesc._fields_]
    assert names == ["size", "origin", "cl_off", "cl_tile_off", "cl_idx", "cl_xyz", "cl_status", "ws", "ws_bytes", "ev", "eps", "min_points", "pick"]
    src = tmp_path / "t.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "cm3d_hip.h"\nint main(void) {\n'
                   + "".join(f'printf("%zu\\n", offsetof(cm3d_depth_cluster_desc, {n}));\n' for n in names)
                   + 'printf("%zu\\n%d\\n", sizeof(cm3d_depth_cluster_desc), CM3D_DEPTH_CLUSTER_LDS_POINTS); return 0; }\n')
    exe = tmp_path / "t"
    r = subprocess.run(["gcc", "-std=c99", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    got = [int(x) for x in subprocess.run([str(exe)], capture_output=True, text=True).stdout.split()]
    assert got == ([getattr(_lib.DepthClusterDesc, n).offset for n in names] + [ctypes.sizeof(_lib.DepthClusterDesc)]
                   + [_lib.DEPTH_CLUSTER_LDS_POINTS])
    # at least two workgroups of the sorting kernel fit a CU's 160 KiB of LDS (12 bytes per point)
    assert 2 * 12 * _lib.DEPTH_CLUSTER_LDS_POINTS <= 160 * 1024


def test_new_symbols_within_abi_5_and_bad_arguments_never_launch():
    from cm3d_amd import _lib
    L = _lib.lib()
    assert _lib.ABI_VERSION == 5 and L.cm3d_abi_version() == 5
    d, c = _lib.LiftPassDesc(), _lib.DepthClusterDesc()
    assert L.cm3d_lift_pass_clustered(None, None, None) == -1
    assert L.cm3d_lift_pass_clustered(ctypes.byref(d), ctypes.byref(c), None) == -1          # size not filled
    c.size = ctypes.sizeof(c)
    assert L.cm3d_lift_pass_clustered(ctypes.byref(d), ctypes.byref(c), None) == -1          # no outputs
    assert L.cm3d_lift_pass_head(ctypes.byref(d), None) == -1 and L.cm3d_lift_pass_tail(ctypes.byref(d), None) == -1
    assert L.cm3d_lift_pass_head(None, None) == -1 and L.cm3d_lift_pass_tail(None, None) == -1
    assert L.cm3d_depth_cluster_workspace_bytes(7, 1000) == 13 * 1000 + 4 * 7 and L.cm3d_depth_cluster_workspace_bytes(0, 5) == 0
    # (every pointer a non-null dummy, so that each call is refused for the one argument it names)
    buf = (ctypes.c_uint8 * 64)()
    p = ctypes.addressof(buf)

    def call(eps=1.0, min_points=20, pick=0, n_masks=3, idx_cap=8, n_frames=1, hit_idx=p, cl_idx=p, ws_bytes=1 << 20, cl_off=p):
        return L.cm3d_depth_cluster(p, hit_idx, p, p, n_masks, idx_cap, p, n_frames, eps, min_points, pick, cl_off, p, cl_idx, p, p, p, ws_bytes, None)
    for kw in (dict(eps=0.0), dict(eps=-1.0), dict(eps=float("nan")), dict(min_points=0), dict(pick=2), dict(pick=-1), dict(n_masks=0),
               dict(idx_cap=0), dict(n_frames=0), dict(hit_idx=None), dict(cl_idx=None), dict(cl_off=None)):
        assert call(**kw) == -1, kw
    assert call(ws_bytes=13 * 8 + 4 * 3 - 1) == -3


CLUSTERED_CASES = {
    "plain": dict(eps="1", mp=20, pick=0),
    "events": dict(ev=0x50, eps="0.5", mp=3, pick=1),
}


def test_clustered_pass_sequence_under_sanitizers():
    """cm3d_lift_pass_clustered over stubs (tests/pass_options_sim.cpp): the head on the raw lists, the clustering from the raw lists into
    the cl_* arrays, the tail on the cl_* arrays with a null tile_work, the events around the clustering; a descriptor of another size,
    a null output or a null pointer makes no call; and whichever call fails, the pass ends there with that call's error (the stubs
    answer -2 for head, tail and events, -3 for the clustering)."""
    got = T.group("cluster")
    for name in ("wrong_size", "no_cl_off", "no_cl_tile_off", "no_cl_idx", "no_cl_xyz", "no_cl_status", "null_pass", "null_cluster"):
        T.assert_refused(got.pop(name), name)
    assert set(got) == set(CLUSTERED_CASES)
    for name, kw in CLUSTERED_CASES.items():
        T.assert_pass(got[name], T.cluster_sequence(**kw), name)


def test_pipeline_cpp_does_not_know_the_clustered_pass():
    """The plain pass links without the new entry points (tests/lift_pass_sim.cpp's stubs)."""
    src = open(os.path.join(ROOT, "cm3d_amd", "csrc", "pipeline.cpp")).read()
    assert "depth_cluster" not in src and "lift_pass_clustered" not in src
    assert "cm3d_lift_pass_head" in src and "cm3d_lift_pass_tail" in src
