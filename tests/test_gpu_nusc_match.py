"""GPU: cm3d_nusc_match (ops.nusc_match) against its host restatement nusc_eval.match_host, byte for byte, on the case sets of
tests/nusc_match_cases.py, and the paths built on it: nusc_eval.evaluate on golden G10, the grid search, its fallback and the two
entry points.  tests/test_nusc_match_host.py pins match_host to the evaluator's own loop."""
import importlib.util
import json
import os

import numpy as np
import pytest
import torch

from cm3d_amd import _lib, eval_detection as ev, fusion, nusc_eval, ops
from tests import nusc_match_cases as cases
from tests.test_eval_detection import _g10, _g10_dataset

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def sets():
    """Every case set packed, with the host's answer at its 97 alphas (computed once)."""
    out = []
    for case in cases.crafted() + [cases.random_case()]:
        packed = cases.packed_of(case)
        out.append((case, packed, nusc_eval.match_host(packed, case.alphas, want_idx=True)))
    return out


def _assert_equal(got, want, what):
    assert got[0].dtype == np.uint8 and got[1].dtype == np.int32 and got[0].shape == want[0].shape and got[1].shape == want[1].shape
    for a in range(want[0].shape[0]):
        assert got[0][a].tobytes() == want[0][a].tobytes(), f"{what}: tp_bits differ at alpha index {a}"
        assert got[1][a].tobytes() == want[1][a].tobytes(), f"{what}: match_idx differ at alpha index {a}"


def test_97_alphas(sets):
    for case, packed, host in sets:
        _assert_equal(ops.nusc_match(packed, case.alphas, want_idx=True), host, case.name)
        assert (host[0] & 0x0f).any() and len({host[0][a].tobytes() for a in range(97)}) > (1 if "ties" in case.name else 5), case.name


def test_one_alpha(sets):
    for case, packed, host in sets:
        for a in (0, 63, 96):
            got = ops.nusc_match(packed, [case.alphas[a]], want_idx=True)
            _assert_equal(got, (host[0][a:a + 1], host[1][a:a + 1]), f"{case.name} alpha {a}")
        bits, idx = ops.nusc_match(packed, [case.alphas[5]])
        assert idx is None and bits.tobytes() == host[0][5:6].tobytes()


def test_more_alphas_than_one_call_takes(sets):
    """One full call of ops.NUSC_ALPHA_CHUNK alphas and a second one: the 97 alphas over and over, shifted so that the seam
    between the calls falls inside the list."""
    n = ops.NUSC_ALPHA_CHUNK + 44
    pick = [(i + 31) % 97 for i in range(n)]
    for case, packed, host in sets:
        got = ops.nusc_match(packed, [case.alphas[i] for i in pick], want_idx=True)
        _assert_equal(got, (host[0][pick], host[1][pick]), case.name)


def test_two_calls_same_bytes(sets):
    for case, packed, _ in sets[:1] + sets[-1:]:
        a, b = ops.nusc_match(packed, case.alphas, want_idx=True), ops.nusc_match(packed, case.alphas, want_idx=True)
        assert a[0].tobytes() == b[0].tobytes() and a[1].tobytes() == b[1].tobytes()


def test_class_agnostic_and_class_aware_packing(sets):
    case = sets[-1][0]                                                     # the random set, ten classes
    alphas = case.alphas[::12]
    agnostic = nusc_eval.pack(case.cands, case.gt, None, cases.TH)
    aware = sets[-1][1]
    assert agnostic["cand_off"].size * 10 - 9 == aware["cand_off"].size and np.diff(agnostic["gt_off"]).max() > np.diff(aware["gt_off"]).max()
    got = ops.nusc_match(agnostic, alphas, want_idx=True)
    _assert_equal(got, nusc_eval.match_host(agnostic, alphas, want_idx=True), "class-agnostic")
    assert (got[0] & 1).sum() > (ops.nusc_match(aware, alphas)[0] & 1).sum()        # any class may take any box
    one = sets[3][0]                                                       # the steal set: one class, so both packings are one problem
    a = ops.nusc_match(nusc_eval.pack(one.cands, one.gt, None, cases.TH), one.alphas, want_idx=True)
    b = ops.nusc_match(nusc_eval.pack(one.cands, one.gt, ["car"], cases.TH), one.alphas, want_idx=True)
    assert a[0].tobytes() == b[0].tobytes() and a[1].tobytes() == b[1].tobytes()


@pytest.mark.parametrize("n_cand,n_gt", [(_lib.NUSC_MAX_CAND + 1, 3), (40, _lib.NUSC_MAX_GT + 1)])
def test_over_capacity_sets_the_status_and_writes_nothing_outside(n_cand, n_gt):
    case = cases.over_capacity_case(n_cand, n_gt)
    packed = cases.packed_of(case)
    with pytest.raises(_lib.Cm3dError, match="status 1") as e:
        ops.nusc_match(packed, case.alphas, want_idx=True)
    assert e.value.status == 1
    # the raw call on pre-filled outputs with guard bytes on both sides
    L, dev = _lib.lib(), torch.device("cuda")
    t = lambda a, dt: torch.from_numpy(np.ascontiguousarray(a, dt)).to(dev)  # noqa: E731
    co, go = packed["cand_off"], packed["gt_off"]
    C, A, T, GUARD = int(co[-1]), len(case.alphas), 4, 256
    d = [t(packed["cand_xy"], np.float64), t(packed["cand_kind"], np.int32), t(packed["cand_p"], np.float64), t(packed["cand_s"], np.float64),
         t(co, np.int32), t(packed["gt_xy"], np.float64), t(go, np.int32), t(case.alphas, np.float64), t(packed["dist_th"], np.float64)]
    bits = torch.full((GUARD + A * C + GUARD,), 0xAB, dtype=torch.uint8, device=dev)
    idx = torch.full((GUARD + A * C * T + GUARD,), -77, dtype=torch.int32, device=dev)
    status = torch.zeros(1, dtype=torch.int32, device=dev)
    rc = L.cm3d_nusc_match(d[0].data_ptr(), d[1].data_ptr(), d[2].data_ptr(), d[3].data_ptr(), d[4].data_ptr(), d[5].data_ptr(), d[6].data_ptr(),
                           co.size - 1, C, d[7].data_ptr(), A, d[8].data_ptr(), T, bits.data_ptr() + GUARD, idx.data_ptr() + 4 * GUARD,
                           status.data_ptr(), 0, 0, torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    assert rc == 0 and int(status.item()) == 1
    bits, idx = bits.cpu().numpy(), idx.cpu().numpy()
    assert (bits[:GUARD] == 0xAB).all() and (bits[-GUARD:] == 0xAB).all() and (idx[:GUARD] == -77).all() and (idx[-GUARD:] == -77).all()
    bits, idx = bits[GUARD:-GUARD].reshape(A, C), idx[GUARD:-GUARD].reshape(A, C, T)
    host = nusc_eval.match_host(packed, case.alphas, want_idx=True)
    over = slice(int(co[1]), int(co[2]))                                   # the group over capacity is left alone, the others are decided
    assert (bits[:, over] == 0xAB).all() and (idx[:, over] == -77).all()
    for sl in (slice(0, int(co[1])), slice(int(co[2]), C)):
        assert bits[:, sl].tobytes() == host[0][:, sl].tobytes() and idx[:, sl].tobytes() == host[1][:, sl].tobytes()
    ok = cases.packed_of(cases.ties())                                     # the device is fine afterwards
    assert ops.nusc_match(ok, [2.0])[0].tobytes() == nusc_eval.match_host(ok, [2.0])[0].tobytes()


@pytest.mark.parametrize("ci", [0, 1, 2])
def test_g10_evaluate_equals_evaluate_host(tmp_path, ci):
    from cm3d_amd import nusc_io
    g = _g10()
    case = g["cases"][ci]
    res = _g10_dataset(g, case, str(tmp_path))
    tables = nusc_io.NuscTables(g["version"], str(tmp_path))
    cfg = ev.DetectionConfig(case["class_range"], "center_distance", [0.5, 1.0, 2.0, 4.0], 2.0, 0.1, 0.1, 500, 5)
    for object_only in (True, False):
        args = (tables, cfg, res, case["scenes"], None, case["drivable_filtering"], object_only, False)
        dev, host = nusc_eval.NativeEval(*args), nusc_eval.NativeEval(*args, matcher=nusc_eval.match_host)
        md_d, md_h = dev.accumulate(), host.accumulate()
        assert list(md_d) == list(md_h) and dev.recall_actual == host.recall_actual
        for k in md_h:
            for f, v in md_h[k].serialize().items():
                assert np.array_equal(np.asarray(getattr(md_d[k], f)), np.asarray(v), equal_nan=True), (k, f)
        a, b = dev.main(), host.main()
        a.pop("eval_time"); b.pop("eval_time")
        assert json.dumps(a, sort_keys=True) == json.dumps(b, sort_keys=True) and a["mean_ap"] > 0.05


def test_grid_search_device_and_its_fallback_equal_the_loop(tmp_path, capsys):
    """520 more twins in one sample: over a thousand candidates of one class there, of which every alpha takes half.  The sweep
    refuses that group; the grid search then scores alpha by alpha and must leave what the loop leaves.  Without them the sweep
    itself must."""
    cfg = ev.DetectionConfig.deserialize(dict(ev.CVPR_2019, max_boxes_per_sample=2000))
    for extra, tag in ((0, "sweep"), (520, "fallback")):
        tables, pred, sam = cases.fusion_files(tmp_path / tag / "data", n_pairs_extra=extra, narrow=True)
        scores = []

        def evaluate(path):
            scores.append(ev.DetectionEval(tables, cfg, path, None, None, False, False, verbose=False).main()["mean_ap"])
            return scores[-1]
        loop = fusion.grid_search(pred, sam, evaluate, str(tmp_path / tag / "loop" / "cur.json"), str(tmp_path / tag / "loop" / "best.json"),
                                  verbose=False)
        capsys.readouterr()
        scorer = nusc_eval.GridScorer(tables, cfg, None)
        got = fusion.grid_search_device(pred, sam, scorer, str(tmp_path / tag / "dev" / "cur.json"), str(tmp_path / tag / "dev" / "best.json"),
                                        verbose=False)
        assert ("alpha by alpha" in capsys.readouterr().err) == (extra > 0)
        assert got == loop + (scores,) and 5 <= len(scores) <= 16 and max(scores) > 0.05
        for name in ("cur.json", "best.json"):
            assert (tmp_path / tag / "dev" / name).read_bytes() == (tmp_path / tag / "loop" / name).read_bytes()


def _fusion_dataset(tmp_path):
    tables, pred, sam = cases.fusion_files(tmp_path / "data", narrow=True)
    return tables.dataroot, cases.write_json(tmp_path / "pred.json", pred), cases.write_json(tmp_path / "sam.json", sam)


def test_eval_custom_metrics_device_equals_the_default(tmp_path):
    dataroot, pred_path, _ = _fusion_dataset(tmp_path)
    spec = importlib.util.spec_from_file_location("eval_custom_entry", os.path.join(ROOT, "src", "nuscenes", "eval_custom.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    for object_only in ("1", "0"):
        common = [pred_path, "--dataroot", dataroot, "--version", "v1.0-synth", "--verbose", "0", "--object_only", object_only]
        host = mod.main(common + ["--output_dir", str(tmp_path / "host")])
        dev = mod.main(common + ["--output_dir", str(tmp_path / "dev"), "--metrics", "device"])
        host.pop("eval_time"); dev.pop("eval_time")
        assert json.dumps(dev, sort_keys=True) == json.dumps(host, sort_keys=True) and host["mean_ap"] > 0.05
        a, b = json.load(open(tmp_path / "host" / "metrics_details.json")), json.load(open(tmp_path / "dev" / "metrics_details.json"))
        assert json.dumps(a, sort_keys=True) == json.dumps(b, sort_keys=True)


def test_linear_matching_native_and_sweep_modes_equal_the_default(tmp_path, monkeypatch, capsys):
    """The entry point in-process (its paths and mode come from the environment when the module is loaded): unset = the host loop,
    native = the loop with each alpha's matching on the GPU, sweep = every alpha from one call."""
    dataroot, pred_path, sam_path = _fusion_dataset(tmp_path)
    out = {}
    for mode in ("", "native", "sweep"):
        d = tmp_path / (mode or "loop")
        for k, v in dict(CM3D_INPUT_PATH=dataroot, CM3D_VER_NAME="v1.0-synth", CM3D_PRED_JSON=pred_path, CM3D_SAM3D_JSON=sam_path,
                         CM3D_MATCHED_JSON=str(d / "cur.json"), CM3D_BEST_JSON=str(d / "best.json"), CM3D_OUTPUT_DIR=str(d / "metrics")).items():
            monkeypatch.setenv(k, v)
        monkeypatch.delenv("CM3D_EVAL_SCENES", raising=False)
        monkeypatch.setenv("CM3D_NUSC_METRICS", mode) if mode else monkeypatch.delenv("CM3D_NUSC_METRICS", raising=False)
        spec = importlib.util.spec_from_file_location("linear_matching_entry", os.path.join(ROOT, "src", "nuscenes", "linear_matching.py"))
        mod = importlib.util.module_from_spec(spec)
        spec.loader.exec_module(mod)
        assert mod.main() == 0
        out[mode] = [ln for ln in capsys.readouterr().out.splitlines() if ln.startswith(("Curr", "Best", "best alpha"))]
    assert out["sweep"] == out[""] == out["native"] and len(out[""]) >= 11 and out[""][-1].startswith("best alpha")
    for mode in ("native", "sweep"):
        for name in ("cur.json", "best.json"):
            assert (tmp_path / mode / name).read_bytes() == (tmp_path / "loop" / name).read_bytes()
        a, b = json.load(open(tmp_path / mode / "metrics" / "metrics_summary.json")), json.load(open(tmp_path / "loop" / "metrics" / "metrics_summary.json"))
        a.pop("eval_time"); b.pop("eval_time")
        assert json.dumps(a, sort_keys=True) == json.dumps(b, sort_keys=True)
