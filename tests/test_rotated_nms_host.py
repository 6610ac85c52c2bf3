"""CPU: the host statement of the rotated-box NMS (cm3d_amd.nms.rotated_nms_host, records_from_boxes) against the exact greedy NMS
of tests/rotated_nms_cases.py, and the switches around it (RotatedNms, the entry points' flags, LiftEngine's default)."""
import argparse
import inspect
import math

import numpy as np
import pytest

from cm3d_amd import nms
from tests import box_iou_exact as X
from tests import rotated_nms_cases as rc


def test_measures_are_the_scalar_float64_restatement():
    """nms.measures on every pair of iou_cases.pairs(): the bits of box_iou_exact's scalar restatement of bev_iou.h."""
    for c in rc.pair_cases():
        a, b = c["rec"]
        assert nms.measures(a, b[None], "iou")[0] == X.bev_iou_f64(a, b), c["name"]
        want = min(X.bev_inter_area_f64(a, b) / (b[2] * b[3]), 1.0)
        assert nms.measures(a, b[None], "cover")[0] == want, c["name"]


def test_every_exact_case_is_decidable_in_float64():
    """The exact-geometry condition: no pair the rule could compare lies within its float64 error bound of its threshold.  Nothing
    is filtered: the crowds were drawn so that it holds."""
    n_pairs = 0
    for c in rc.all_cases():
        if c["exact"]:
            assert rc.undecidable_pairs(c["rec"], c["group"], c["thr"], c["agnostic"], c["measures"]) == [], c["name"]
            n_pairs += sum(len(v) for v in rc.neighbours(c["rec"][:rc.MAX_BOXES]))
    assert n_pairs > 5000


def test_cover_straddlers_straddle():
    rows = rc.cover_straddlers()
    assert len(rows) == 144
    for thr, d, a, b in rows:
        v, bound = rc.exact_measure(a, b, "cover")
        assert (v > thr) == (d > 0) and abs(float(v) - (thr + d)) < 1e-12 and bound < 1e-12 < abs(d) / 2, (thr, d)
        assert (nms.measures(np.array(a[:6]), np.array([b[:6]]), "cover")[0] > thr) == (d > 0)


@pytest.mark.parametrize("measure", rc.MEASURES)
def test_host_equals_the_exact_greedy_nms(measure):
    exact = rc.exact_results()
    shares = []
    for c in rc.all_cases():
        if measure not in c["measures"]:
            continue
        got = nms.rotated_nms_host(c["rec"], c["score"], c["group"], [0, len(c["rec"])], c["thr"], measure, c["agnostic"])
        assert got.dtype == np.int32
        if c["want"] is not None:
            assert got.tolist() == c["want"].tolist(), c["name"]
        if c["exact"]:
            assert np.array_equal(got, exact[c["name"], measure]), c["name"]
        if c["name"].startswith("crowd") and len(got) >= 63:
            shares.append(1.0 - got.mean())
            assert shares[-1] >= 1.0 / 3.0, (c["name"], shares[-1])      # otherwise the frame shows nothing
    assert len(shares) >= 25
    last = [c for c in rc.all_cases() if c["name"] == "beyond_the_frame_limit"][0]
    got = nms.rotated_nms_host(last["rec"], last["score"], last["group"], [0, 1030], last["thr"], measure)
    assert got[1024:].tolist() == [0] * 6 and got[np.argsort(-last["score"][:1024])[:6]].tolist() == [1] * 6


def test_degenerate_boxes_neither_suppress_nor_go():
    c = [c for c in rc.all_cases() if c["name"] == "degenerate_in_crowd/agnostic"][0]
    for m in rc.MEASURES:
        got = nms.rotated_nms_host(c["rec"], c["score"], c["group"], [0, 65], c["thr"], m, True)
        assert got[[10, 20, 30, 40, 50]].tolist() == [1] * 5
        rest = np.delete(np.arange(65), [10, 20, 30, 40, 50])
        alone = nms.rotated_nms_host(c["rec"][rest], c["score"][rest], c["group"][rest], [0, 60], c["thr"], m, True)
        assert np.array_equal(got[rest], alone) and alone.sum() < 60


def test_frames_and_take():
    """Several frames in one call (an empty one between them); `take` removes boxes from the pass altogether."""
    a = [c for c in rc.crafted_cases() if c["name"] == "chain@0"][0]
    rec = np.concatenate([a["rec"], a["rec"]])
    score = np.concatenate([a["score"], a["score"]])
    got = nms.rotated_nms_host(rec, score, np.zeros(6, int), [0, 3, 3, 6], [0.4])
    assert got.tolist() == [1, 0, 1, 1, 0, 1]
    got = nms.rotated_nms_host(rec, score, np.zeros(6, int), [0, 3, 3, 6], [0.4], take=[True, True, True, False, True, True])
    assert got.tolist() == [1, 0, 1, 0, 1, 0]                           # without A, B is kept and suppresses C


def test_records_from_boxes():
    prior = np.array([[2.0, 4.5, 1.6], [0.7, 0.8, 1.7], [2.9, 12.0, 3.5]])            # w, l, h
    yaw = 0.7
    qw, qz = math.cos(yaw / 2), math.sin(yaw / 2)
    box = np.zeros((4, 10))
    box[0] = [10.5, -3.25, 1.0, qw, qz, yaw, 0.4, 0.9, 0, 3]             # a vehicle row
    box[1] = [1.0, 2.0, 0.5, 1.0, 0.0, 0.1, 0.2, 0.8, 1, 3]              # identity rotation: axis-aligned
    box[2] = [5.0, 6.0, 0.0, -qw, -qz, 0.0, 0.0, 0.7, 2, 1]              # the quaternion's other sign: the same axis
    box[3] = [7.0, 8.0, 0.0, 1.0, 0.0, 0.0, 0.0, 0.6, 99, 0]             # class out of range: class 0
    r = nms.records_from_boxes(box, prior, waymo=False)
    assert r.shape == (4, 6) and r.dtype == np.float64
    assert r[0].tolist() == [10.5, -3.25, 4.5, 2.0, qw * qw - qz * qz, 2.0 * qw * qz]
    assert abs(r[0, 4] - math.cos(yaw)) < 1e-15 and abs(r[0, 5] - math.sin(yaw)) < 1e-15
    assert r[1].tolist() == [1.0, 2.0, 0.8, 0.7, 1.0, 0.0]
    assert r[2].tolist() == [5.0, 6.0, 12.0, 2.9, r[0, 4], r[0, 5]]
    assert r[3, 2:4].tolist() == [4.5, 2.0]
    w = box.copy()
    w[:, 3] = [yaw, 0.0, math.pi, -math.pi]
    w[:, 4] = 0.0
    rw = nms.records_from_boxes(w, prior, waymo=True)
    assert np.array_equal(rw[:, :4], r[:, :4])
    assert rw[:, 4].tolist() == [math.cos(yaw), 1.0, math.cos(math.pi), math.cos(-math.pi)]
    assert rw[:, 5].tolist() == [math.sin(yaw), 0.0, math.sin(math.pi), math.sin(-math.pi)]
    assert nms.live(r).all() and not nms.live(np.array([[np.nan, 0, 1, 1, 1, 0], [0, 0, 0, 1, 1, 0], [0, np.inf, 1, 1, 1, 0], [0, 0, np.nan, 1, 1, 0]])).any()


def test_flags_and_their_defaults():
    ap = argparse.ArgumentParser()
    nms.add_arguments(ap)
    d = ap.parse_args([])
    assert (d.nms, d.nms_overlap, d.nms_thr, d.nms_class_agnostic) == ("circle", "iou", 0.4, False)
    assert nms.from_args(d) is None
    a = ap.parse_args(["--nms", "rotated"])
    assert nms.from_args(a) == nms.RotatedNms("iou", 0.4, False)
    a = ap.parse_args(["--nms", "rotated", "--nms-overlap", "cover", "--nms-thr", "0.25", "--nms-class-agnostic"])
    assert nms.from_args(a) == nms.RotatedNms("cover", 0.25, True) and nms.from_args(a).measure_index == 1
    assert nms.from_args(ap.parse_args(["--nms-overlap", "cover", "--nms-class-agnostic"])) is None      # circle: the others are not read
    for bad in (["--nms", "square"], ["--nms-overlap", "giou"]):
        with pytest.raises(SystemExit):
            ap.parse_args(bad)


def test_entry_points_carry_the_flags():
    from cm3d_amd import pipeline_nuscenes, pipeline_waymo, pipeline_kitti
    for mod, has in ((pipeline_nuscenes, True), (pipeline_waymo, True), (pipeline_kitti, False)):
        assert ("nmsmod.add_arguments(ap)" in inspect.getsource(mod.main)) == has, mod.__name__


def test_thresholds_from_a_mapping():
    from cm3d_amd.lifting import ClassTable
    n = ClassTable.nuscenes()
    r = nms.RotatedNms(thr={"car": 0.5, "bus": 0.3})
    t = r.thr_by_group(n)
    assert t.dtype == np.float64 and t.shape == n.nms_thr.shape
    assert t[n.index("car")] == 0.5 and t[n.index("bus")] == 0.3 and t[n.index("pedestrian")] == 0.4
    assert nms.RotatedNms(thr=0.25).thr_by_group(n).tolist() == [0.25] * len(n.names)
    w = ClassTable.waymo()                                       # several classes share a Waymo type: one threshold per type
    veh = [k for k in w.names if w.nms_group[w.index(k)] == w.nms_group[w.index("car")]]
    assert len(veh) > 1
    t = nms.RotatedNms(thr={"car": 0.6}).thr_by_group(w)
    assert t.shape == w.nms_thr.shape and t[w.nms_group[w.index("car")]] == 0.6 and t[w.nms_group[w.index("pedestrian")]] == 0.4
    assert nms.RotatedNms(thr={veh[0]: 0.6, veh[1]: 0.6}).thr_by_group(w)[w.nms_group[w.index("car")]] == 0.6
    with pytest.raises(ValueError):
        nms.RotatedNms(thr={veh[0]: 0.6, veh[1]: 0.5}).thr_by_group(w)
    with pytest.raises(ValueError):
        nms.RotatedNms(thr={"unicorn": 0.5}).thr_by_group(n)
    with pytest.raises(ValueError):
        nms.RotatedNms(measure="giou")
    with pytest.raises(ValueError):
        nms.RotatedNms(thr=float("nan"))


def test_engine_default_is_no_rotated_nms():
    from cm3d_amd import lifting
    p = inspect.signature(lifting.LiftEngine.__init__).parameters["nms"]
    assert p.default is None and lifting.RotatedNms is nms.RotatedNms
