"""tools/wedge_hull_sim.py (the CPU model of the camera visits per wave-chunk) on two `tiny` frames.  No GPU."""
import importlib.util
import os

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _tool():
    spec = importlib.util.spec_from_file_location("wedge_hull_sim", os.path.join(ROOT, "tools", "wedge_hull_sim.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def test_hull_visits_lie_between_candidate_and_image_visits():
    r = _tool().simulate("tiny", 2, 2)
    assert r["chunks"] == 2 * 24 and r["image_visits_per_chunk"] > 0          # 2 sweeps x 3000 rows: 24 wave-chunks per frame
    assert r["hull_visits_per_chunk"] <= r["image_visits_per_chunk"]
    assert r["candidate_visits_per_chunk"] <= r["hull_visits_per_chunk"]
    assert 0.0 < r["hull_width_median"] <= 1.0
