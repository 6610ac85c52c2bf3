"""GPU: cm3d_waymo_metrics_sweep (ops.waymo_metrics_sweep, fusion.waymo_grid_search_device) -- every alpha of the SAM3D fusion
grid search scored in one call -- against the reference evaluator's numbers (golden G11), against the per-alpha device path
(fuse, encode, decode, pack, cm3d_waymo_metrics: the same solver on the same rows, so identical even under ties) and against
the host restatement; solver sizes, static groups, determinism, capacity and the entry point."""
import hashlib
import os
import subprocess
import sys

import numpy as np
import pytest

from cm3d_amd import _lib, fusion, ops, waymo as wm, waymo_eval as we
from tests import waymo_sweep_cases as cases
from tests.waymo_metrics_cases import blob, fixtures

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _per_alpha(inp, alphas):
    """The per-alpha device path: one cm3d_waymo_metrics call on each alpha's decoded fused file."""
    out = [ops.waymo_metrics(inp.packed_at(a)) for a in alphas]
    return np.stack([o[0] for o in out]), np.stack([o[1] for o in out])


def _assert_equal(got, want):
    assert got[0].shape == want[0].shape and got[1].shape == want[1].shape
    for a in range(want[0].shape[0]):
        assert np.array_equal(got[0][a], want[0][a]), f"counts differ at alpha index {a}"
        assert np.array_equal(got[1][a], want[1][a]), f"heading sums differ at alpha index {a}"


def test_g11_fixture_equals_the_evaluator_binary(tmp_path):
    f = fixtures()["fusion"]
    best, cur = tmp_path / "best.bin", tmp_path / "out" / "cur.bin"
    alpha, score, scores = fusion.waymo_grid_search_device(wm.decode_objects(blob(f["pred"])), wm.decode_objects(blob(f["sam3d"])),
                                                           we.decode_objects(blob(f["gt"])), str(cur), str(best), verbose=False)
    assert scores == f["scores"]
    assert alpha == f["best_alpha"] and score == f["best_score"]
    assert hashlib.sha256(best.read_bytes()).hexdigest() == f["best_sha256"]
    inp = cases.g11_inputs()
    assert cur.read_bytes() == wm.encode_objects(fusion.fuse_waymo(*inp.sides(), cases.g11_alphas(inp)[-1]))


def test_empty_grid_writes_nothing(tmp_path):
    f = fixtures()["fusion"]
    best, cur = tmp_path / "best.bin", tmp_path / "cur.bin"
    r = fusion.waymo_grid_search_device(wm.decode_objects(blob(f["pred"])), [], we.decode_objects(blob(f["gt"])), str(cur), str(best),
                                        verbose=False)
    assert r == (0, -1, []) and not best.exists() and not cur.exists()


@pytest.fixture(scope="module")
def crafted():
    """The crafted set, 97 alphas, and both references at every one of them."""
    inp = cases.crafted_inputs()
    alphas = cases.long_alphas(97)
    return inp, alphas, _per_alpha(inp, alphas), we.counts_sweep_host(inp.packed_candidates(), alphas)


def test_crafted_set_97_alphas(crafted):
    inp, alphas, device, host = crafted
    _assert_equal(device, host)                                            # the two references agree
    got = ops.waymo_metrics_sweep(inp.packed_candidates(), alphas)
    _assert_equal(got, device)
    _assert_equal(got, host)
    assert got[0][:, :, 0, 0].sum(1).min() > 60 and len({got[0][a].tobytes() for a in range(97)}) > 20


def test_crafted_set_one_alpha(crafted):
    inp, alphas, device, host = crafted
    for a in (0, 3, 5):                                                    # no pair switched; the ties and the clip; every pair switched
        got = ops.waymo_metrics_sweep(inp.packed_candidates(), [alphas[a]])
        assert got[0].shape == (1, 16, 101, 4) and got[1].shape == (1, 16, 101)
        _assert_equal(got, (device[0][a:a + 1], device[1][a:a + 1]))
        _assert_equal(got, (host[0][a:a + 1], host[1][a:a + 1]))


def test_crafted_set_more_alphas_than_one_call_takes(crafted):
    """300 alphas = one full call of ops.SWEEP_ALPHA_CHUNK and a second one: the 97 alphas over and over, shifted so that
    the seam between the calls falls inside the list; every alpha against its references."""
    inp, alphas, device, host = crafted
    n = ops.SWEEP_ALPHA_CHUNK + 44
    pick = [(i + 31) % 97 for i in range(n)]
    got = ops.waymo_metrics_sweep(inp.packed_candidates(), [alphas[i] for i in pick])
    _assert_equal(got, (device[0][pick], device[1][pick]))
    _assert_equal(got, (host[0][pick], host[1][pick]))


def test_two_runs_bit_identical(crafted):
    inp, alphas, _, _ = crafted
    pc = inp.packed_candidates()
    a, b = ops.waymo_metrics_sweep(pc, alphas), ops.waymo_metrics_sweep(pc, alphas)
    assert a[0].tobytes() == b[0].tobytes() and a[1].tobytes() == b[1].tobytes()


def test_solver_sizes_equal_the_per_alpha_path():
    inp, sizes = cases.solver_inputs()
    pc = inp.packed_candidates()
    n_cand = np.diff(pc["cand_off"])
    shard0 = pc["group_bd"] == 0
    assert set(cases.SOLVER_SIZES) <= set(n_cand[shard0].tolist())          # candidate supersets at the instance boundaries
    per_alpha_rows = [np.diff(inp.packed_at(a)["pred_off"]) for a in cases.SOLVER_ALPHAS]
    for rows in per_alpha_rows:                                            # and active rows at them, at every alpha
        assert set(cases.SOLVER_SIZES) <= set(rows.tolist())
    assert any(not np.array_equal(per_alpha_rows[0], r) for r in per_alpha_rows[1:])        # range shards change size
    got = ops.waymo_metrics_sweep(pc, cases.SOLVER_ALPHAS)
    want = _per_alpha(inp, cases.SOLVER_ALPHAS)
    _assert_equal(got, want)
    tp = got[0][:, 0, 0, 0]
    assert tp.min() * 2 > sum(r for r, _ in sizes.values())                 # no group matches emptily
    assert len({got[1][a].tobytes() for a in range(len(cases.SOLVER_ALPHAS))}) == len(cases.SOLVER_ALPHAS)


def test_static_groups_only_and_none():
    f = fixtures()["fusion"]
    only = cases.Inputs(blob(f["pred"]), wm.encode_objects([]), blob(f["gt"]))          # no SAM3D box: nothing depends on alpha
    pc = only.packed_candidates()
    assert pc["group_static"].all() and pc["cand_kind"].size > 100
    alphas = [0.5, 1.0, 2.0]
    got = ops.waymo_metrics_sweep(pc, alphas)
    _assert_equal(got, _per_alpha(only, alphas))
    assert np.array_equal(got[0][0], got[0][2]) and got[0][0, :, 0, 0].sum() > 20
    # none: every prediction is half of a pair, every ground truth within 30 m has one on it (explicit match lists)
    rng = np.random.default_rng(8)
    P, S, G = [], [], []
    k = ("none-static", 1)
    for i in range(40):
        c = [float(rng.uniform(-20, 20)), float(rng.uniform(-20, 20)), 0.0]
        G.append(we.encode_gt_object(c, 4.5, 2.0, 1.6, 0.3, 1, k[0], k[1], 50))
        P.append(wm.encode_object([c[0] + 0.1, c[1], 0.0], 4.5, 2.0, 1.6, 0.35, 1, float(rng.uniform(0.1, 1)), k[0], k[1]))
        S.append(wm.encode_object([c[0], c[1] + 0.1, 0.0], 4.5, 2.0, 1.6, 0.25, 1, float(rng.uniform(0.1, 1)), k[0], k[1]))
    none = cases.Inputs(wm.encode_objects(P), wm.encode_objects(S), wm.encode_objects(G), matches=({k: list(range(40))}, {k: list(range(40))}))
    pc = none.packed_candidates()
    assert not pc["group_static"].any() and pc["group_static"].size == 2
    got = ops.waymo_metrics_sweep(pc, alphas)
    _assert_equal(got, _per_alpha(none, alphas))
    assert not np.array_equal(got[1][0], got[1][2])


def test_over_capacity_raises_and_the_grid_search_falls_back(tmp_path, capsys):
    """600 pairs in one frame: 1200 candidates of which 600 are active at any alpha.  The per-alpha path takes that, the sweep's
    ranking does not."""
    n = 600
    k = ("crowd", 1)
    assert 2 * n > _lib.MAX_MATCH_BOXES >= n
    rng = np.random.default_rng(3)
    P, S, G = [], [], []
    for i in range(n):
        c = [6.0 * (i % 30) - 90.0, 4.0 * (i // 30) - 40.0, 0.0]
        G.append(we.encode_gt_object(c, 4.5, 2.0, 1.6, 0.0, 1, k[0], k[1], 50))
        P.append(wm.encode_object([c[0] + 0.1, c[1], 0.0], 4.5, 2.0, 1.6, 0.05, 1, float(rng.uniform(0.5, 0.625)), k[0], k[1]))
        S.append(wm.encode_object([c[0], c[1] + 0.1, 0.0], 4.5, 2.0, 1.6, -0.05, 1, float(rng.uniform(0.5, 0.625)), k[0], k[1]))
    pred, sam, gt = wm.encode_objects(P), wm.encode_objects(S), wm.encode_objects(G)
    inp = cases.Inputs(pred, sam, gt, match=fusion.match_samples)
    assert len(inp.pm[k]) == n
    alphas = cases.g11_alphas(inp)
    assert 3 <= len(alphas) <= 12
    with pytest.raises(_lib.Cm3dError, match="status 1"):
        ops.waymo_metrics_sweep(inp.packed_candidates(), alphas)
    scores = []

    def evaluate(path):
        scores.append(we.evaluate(we.read_objects(path), inp.gt)[0]["Overall/L2 mAP"])
        return scores[-1]
    loop = fusion.waymo_grid_search(inp.pred_objs, inp.sam_objs, evaluate, str(tmp_path / "loop_cur.bin"), str(tmp_path / "loop_best.bin"),
                                    verbose=False)
    got = fusion.waymo_grid_search_device(inp.pred_objs, inp.sam_objs, inp.gt, str(tmp_path / "cur.bin"), str(tmp_path / "best.bin"),
                                          verbose=False)
    assert "alpha by alpha" in capsys.readouterr().err
    assert got == loop + (scores,) and len(scores) == len(alphas) and max(scores) > 0.1
    assert (tmp_path / "best.bin").read_bytes() == (tmp_path / "loop_best.bin").read_bytes()
    assert (tmp_path / "cur.bin").read_bytes() == (tmp_path / "loop_cur.bin").read_bytes()
    f = fixtures()["fusion"]                                                # the device is fine afterwards
    inp = cases.g11_inputs()
    alphas = cases.g11_alphas(inp)[:4]
    counts, hsum = ops.waymo_metrics_sweep(inp.packed_candidates(), alphas)
    for a in range(4):
        text = we.format_metrics(we.metrics_from_counts(counts[a], hsum[a]))
        assert fusion.parse_waymo_metrics(text)[1] == f["scores"][a]


def test_entry_point_sweep_mode_equals_native(tmp_path):
    f = fixtures()["fusion"]
    for name in ("pred", "sam3d", "gt"):
        (tmp_path / f"{name}.bin").write_bytes(blob(f[name]))
    out = {}
    for mode in ("native", "sweep"):
        (tmp_path / mode).mkdir()
        env = dict(os.environ, CM3D_WAYMO_METRICS=mode, CM3D_PRED_BIN=str(tmp_path / "pred.bin"), CM3D_SAM3D_BIN=str(tmp_path / "sam3d.bin"),
                   CM3D_WAYMO_GT_BIN=str(tmp_path / "gt.bin"), CM3D_OUTPUT_DIR=str(tmp_path / mode))
        r = subprocess.run([sys.executable, "linear_matching.py"], cwd=os.path.join(ROOT, "src", "waymo"), env=env, capture_output=True,
                           text=True, timeout=300)
        assert r.returncode == 0, r.stderr[-2000:]
        out[mode] = r.stdout.strip().splitlines()[-1]
    assert out["sweep"] == out["native"] == f"best alpha {f['best_alpha']}, Overall/L2 mAP {f['best_score']}"
    for name in ("best_matched_pseudolabels_waymo_train_0310.bin", "matched_pseudolabels_waymo_train_0310.bin"):
        assert (tmp_path / "sweep" / name).read_bytes() == (tmp_path / "native" / name).read_bytes()
    assert hashlib.sha256((tmp_path / "sweep" / "best_matched_pseudolabels_waymo_train_0310.bin").read_bytes()).hexdigest() == f["best_sha256"]
