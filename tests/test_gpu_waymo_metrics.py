"""GPU: the Waymo detection metrics of cm3d_waymo_metrics (cm3d_amd/waymo_eval.evaluate) against the reference
evaluator's printed output (golden G11) and against the host restatement, its cutoff deduplication, determinism,
capacity errors, the native fusion grid search and the entry point."""
import hashlib
import os
import subprocess
import sys

import numpy as np
import pytest

from cm3d_amd import _lib, fusion, ops, waymo as wm, waymo_eval as we
from tests.waymo_metrics_cases import blob, fixtures, generator

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CASES = sorted(fixtures()["cases"])


def _objs(c):
    return we.decode_objects(blob(c["pred"])), we.decode_objects(blob(c["gt"]))


@pytest.mark.parametrize("name", CASES)
def test_gpu_equals_reference_binary(name):
    c = fixtures()["cases"][name]
    ap, text = we.evaluate(*_objs(c))
    assert text == c["text"]
    assert ap == fusion.parse_waymo_metrics(c["text"])[0]


@pytest.fixture(scope="module")
def random_2000():
    gen = generator()
    P, G = gen.random_set(np.random.default_rng(2000), 2000, gt_rate=6, fp_rate=3)
    return we.decode_objects(wm.encode_objects(P)), we.decode_objects(wm.encode_objects(G))


def test_gpu_equals_host_on_2000_frames(random_2000):
    packed = we.pack(*random_2000)
    counts, hsum = ops.waymo_metrics(packed)
    hc, hh = we.counts_host(packed)
    assert np.array_equal(counts, hc)
    assert np.array_equal(hsum, hh)
    assert counts[:, 0, 0].sum() > 1000                                     # matches at every breakdown of interest
    g = we.metrics_from_counts(counts, hsum)
    h = we.metrics_from_counts(hc, hh)
    for k in g:
        assert abs(g[k][0] - h[k][0]) <= 1e-12 and abs(g[k][1] - h[k][1]) <= 1e-12


def test_cutoff_dedup_equals_every_cutoff(random_2000):
    packed = we.pack(*random_2000)
    a = ops.waymo_metrics(packed)
    b = ops.waymo_metrics(packed, per_cutoff=True)
    assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1])
    c = fixtures()["cases"]["duplicates"]                                  # crowded frames: the 128 / 256 / 1024 column solvers
    packed = we.pack(*_objs(c))
    a = ops.waymo_metrics(packed)
    b = ops.waymo_metrics(packed, per_cutoff=True)
    assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1])


def test_two_runs_bit_identical(random_2000):
    packed = we.pack(*random_2000)
    a, b = ops.waymo_metrics(packed), ops.waymo_metrics(packed)
    assert a[0].tobytes() == b[0].tobytes() and a[1].tobytes() == b[1].tobytes()


def test_large_groups_match_host():
    """One type, 200 and 600 boxes in a frame, then the sizes at which k_wm_match changes instance (64 / 128 / 256 columns).
    The weights are jittered and generic: under exact ties the number of positive pairs of a maximum-weight assignment is
    not unique and scipy's choice need not be the device's (the tie rule is pinned bit for bit against the oracle by the
    `ties` family of tests/assign_cases.py, up to the widest instance, in tests/test_gpu_assign.py)."""
    rng = np.random.default_rng(5)
    boundary = (64, 65, 128, 129, 256, 257)
    frames = []
    for ts, n in enumerate((200, 600) + boundary, start=1):
        c = rng.uniform(-40, 40, (n, 2))
        P, G = [], []
        for i in range(n):
            G.append(we.encode_gt_object([c[i, 0], c[i, 1], 0.0], 4.5, 2.0, 1.6, 0.0, 1, "x", ts, 50))
            P.append(wm.encode_object([c[i, 0] + rng.normal(0, 0.2), c[i, 1] + rng.normal(0, 0.2), 0.0], 4.5, 2.0, 1.6,
                                      rng.normal(0, 0.2), 1, float(rng.uniform()), "x", ts))
        frames.append((n, P, G))
    for n, P, G in frames:                                                   # host only: no boundary group matches emptily
        if n in boundary:
            tp = we.counts_host(we.pack(we.decode_objects(wm.encode_objects(P)), we.decode_objects(wm.encode_objects(G))))[0][0, 0, 0]
            assert 2 * tp >= n, f"group of {n}: {tp} true positives at cutoff 0"
    P, G = sum((f[1] for f in frames), []), sum((f[2] for f in frames), [])
    packed = we.pack(we.decode_objects(wm.encode_objects(P)), we.decode_objects(wm.encode_objects(G)))
    assert set(boundary) <= set(np.diff(packed["gt_off"]).tolist()) and set(boundary) <= set(np.diff(packed["pred_off"]).tolist())
    counts, hsum = ops.waymo_metrics(packed)
    hc, hh = we.counts_host(packed)
    assert np.array_equal(counts, hc) and np.array_equal(hsum, hh)


def test_over_capacity_is_an_error_status():
    n = _lib.MAX_MATCH_BOXES + 1
    P = [wm.encode_object([0.5 * i, 3.0, 0.0], 4.5, 2.0, 1.6, 0.0, 1, 0.5, "x", 1) for i in range(n)]
    G = [we.encode_gt_object([0.5 * i, 3.0, 0.0], 4.5, 2.0, 1.6, 0.0, 1, "x", 1, 50) for i in range(3)]
    packed = we.pack(we.decode_objects(wm.encode_objects(P)), we.decode_objects(wm.encode_objects(G)))
    with pytest.raises(_lib.Cm3dError, match="status 1"):
        ops.waymo_metrics(packed)
    c = fixtures()["cases"]["scores"]
    packed = we.pack(*_objs(c))
    packed["group_bd"] = packed["group_bd"].copy()
    packed["group_bd"][0] = 99
    with pytest.raises(_lib.Cm3dError, match="status 2"):
        ops.waymo_metrics(packed)
    ap, text = we.evaluate(*_objs(c))                                      # the device is fine afterwards
    assert text == c["text"]


def test_native_fusion_grid_search(tmp_path):
    f = fixtures()["fusion"]
    gt_path = tmp_path / "gt.bin"
    gt_path.write_bytes(blob(f["gt"]))
    gt = we.read_objects(str(gt_path))
    scores = []

    def evaluate(path):
        s = we.evaluate(we.read_objects(path), gt)[0]["Overall/L2 mAP"]
        scores.append(s)
        return s
    best = tmp_path / "best.bin"
    alpha, score = fusion.waymo_grid_search(wm.decode_objects(blob(f["pred"])), wm.decode_objects(blob(f["sam3d"])), evaluate,
                                            str(tmp_path / "cur.bin"), str(best), verbose=False)
    assert scores == f["scores"]
    assert alpha == f["best_alpha"] and score == f["best_score"]
    assert hashlib.sha256(best.read_bytes()).hexdigest() == f["best_sha256"]


def test_entry_point_prints_the_binary_lines(tmp_path):
    script = os.path.join(ROOT, "src", "waymo", "compute_detection_metrics.py")
    for name in ("random", "difficulty"):
        c = fixtures()["cases"][name]
        (tmp_path / "p.bin").write_bytes(blob(c["pred"]))
        (tmp_path / "g.bin").write_bytes(blob(c["gt"]))
        r = subprocess.run([sys.executable, script, str(tmp_path / "p.bin"), str(tmp_path / "g.bin")], capture_output=True, text=True,
                           timeout=300)
        assert r.returncode == 0, r.stderr
        assert r.stdout == c["text"]
