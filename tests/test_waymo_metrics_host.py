"""CPU: the Waymo detection metrics restated on the host (cm3d_amd/waymo_eval.py) against the printed output of the
reference's evaluator binary (golden G11), the ground-truth decoder, the text format and the entry point's arguments."""
import os
import subprocess
import sys

import numpy as np
import pytest

from cm3d_amd import fusion, waymo as wm, waymo_eval as we
from tests.waymo_metrics_cases import blob, fixtures, generator

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CASES = sorted(fixtures()["cases"])


def test_gt_fields_decode():
    b = wm.encode_objects([we.encode_gt_object([1.0, 2.0, 3.0], 4.5, 2.0, 1.6, 0.25, 1, "seg", 77, 6, difficulty=2),
                           we.encode_gt_object([5.0, 6.0, 0.5], 0.9, 0.8, 1.8, -1.0, 2, "seg", 78, 0),
                           wm.encode_object([1.0, 2.0, 3.0], 4.5, 2.0, 1.6, 0.25, 4, 0.75, "seg", 77)])
    a, g, p = we.decode_objects(b)
    assert a["center"] == [1.0, 2.0, 3.0] and (a["length"], a["width"], a["height"], a["heading"]) == (4.5, 2.0, 1.6, 0.25)
    assert (a["type"], a["context_name"], a["timestamp_micros"]) == (1, "seg", 77)
    assert (a["num_lidar_points_in_box"], a["detection_difficulty_level"], a["score"]) == (6, 2, 0.0)
    assert (g["num_lidar_points_in_box"], g["detection_difficulty_level"]) == (0, 0)
    assert (p["type"], p["score"], p["num_lidar_points_in_box"]) == (4, 0.75, 0)
    old = wm.decode_objects(wm.encode_objects([wm.encode_object([1.0, 2.0, 3.0], 4.5, 2.0, 1.6, 0.25, 4, 0.75, "seg", 77)]))[0]
    assert {k: p[k] for k in old} == old                         # the new decoder agrees with the writer's own on its fields


def test_difficulty_levels():
    o = dict(num_lidar_points_in_box=0, detection_difficulty_level=0)
    for pts, lv, want in ((1, 0, 2), (5, 0, 2), (6, 0, 1), (200, 0, 1), (200, 2, 2), (3, 1, 1)):
        assert we.gt_level(dict(o, num_lidar_points_in_box=pts, detection_difficulty_level=lv)) == want


@pytest.mark.parametrize("name", CASES)
def test_host_equals_reference_binary(name):
    c = fixtures()["cases"][name]
    _, text = we.evaluate_host(we.decode_objects(blob(c["pred"])), we.decode_objects(blob(c["gt"])))
    assert text == c["text"]


def test_text_round_trips_through_parse():
    c = fixtures()["cases"]["random"]
    ap, text = we.evaluate_host(we.decode_objects(blob(c["pred"])), we.decode_objects(blob(c["gt"])))
    ref, score = fusion.parse_waymo_metrics(c["text"])
    assert ap == ref and ap["Overall/L2 mAP"] == score
    assert len(text.splitlines()) == 32 and fusion.parse_waymo_metrics(text)[0] == ap


def test_ap_rule_known_answers():
    # one TP at recall 1 after a gap: trapezoids over points every 0.05 recall with the running maximum precision
    p = np.array([2 / 3, 0.5, 1.0, 0.0], np.float32)
    r = np.array([1.0, 0.5, 0.5, 0.0], np.float32)
    assert abs(we.mean_average_precision(p, r) - 0.841667) < 1e-6
    assert abs(we.mean_average_precision([0.5, 0.0], [1.0, 0.0]) - 0.5) < 1e-6       # recall 0 takes its neighbour's precision
    assert we.mean_average_precision([1.0], [0.0]) == 0.0


def test_unknown_type_is_an_error():
    P = we.decode_objects(wm.encode_objects([wm.encode_object([1, 2, 0], 4, 2, 1.5, 0, 0, 0.5, "c", 1)]))
    with pytest.raises(ValueError):
        we.evaluate_host(P, [])


def test_generator_cases_are_the_fixture_inputs():
    gen = generator()
    P, G = gen.case_headings()
    c = fixtures()["cases"]["headings"]
    assert wm.encode_objects(P) == blob(c["pred"]) and wm.encode_objects(G) == blob(c["gt"])


def test_entry_point_arguments(tmp_path):
    script = os.path.join(ROOT, "src", "waymo", "compute_detection_metrics.py")
    r = subprocess.run([sys.executable, script], capture_output=True, text=True)
    assert r.returncode == 2 and "usage" in r.stderr
    r = subprocess.run([sys.executable, script, str(tmp_path / "missing.bin"), str(tmp_path / "gt.bin")], capture_output=True, text=True)
    assert r.returncode == 2 and "no such file" in r.stderr
    c = fixtures()["cases"]["scores"]
    (tmp_path / "p.bin").write_bytes(blob(c["pred"]))
    (tmp_path / "g.bin").write_bytes(blob(c["gt"]))
    r = subprocess.run([sys.executable, script, str(tmp_path / "p.bin"), str(tmp_path / "g.bin"), "--host"], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    assert r.stdout == c["text"]


def test_fixture_matches_its_report():
    import hashlib
    import json
    golden = os.path.join(ROOT, "tests", "golden")
    report = json.load(open(os.path.join(golden, "g11_waymo_metrics_report.json")))
    with open(os.path.join(golden, "g11_waymo_metrics.json.gz"), "rb") as f:
        assert hashlib.sha256(f.read()).hexdigest() == report["G11 g11_waymo_metrics.json.gz sha256"]
    assert sorted(n for n, _, _ in report["G11 cases: name / predictions / ground truth"]) == CASES
    assert report["G11 fusion: alphas / best alpha / best Overall L2 mAP"][1] == fixtures()["fusion"]["best_alpha"]
