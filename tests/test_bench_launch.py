"""CPU: `python bench.py --gpus N` brings up its N ranks by itself (no torchrun wrapper), and refuses a rank count that
does not match --gpus.  The rehearsal mode runs the launch, the rendezvous and the single record exchange without kernels."""
import json
import os
import subprocess
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _env(**extra):
    env = {k: v for k, v in os.environ.items() if k not in ("RANK", "WORLD_SIZE", "LOCAL_RANK", "MASTER_ADDR", "MASTER_PORT")}
    env.update(CM3D_DIST_BACKEND="gloo", **extra)
    return env


def test_bench_launches_its_own_ranks():
    r = subprocess.run([sys.executable, "bench.py", "--gpus", "2", "--rehearse-launch"], cwd=ROOT, env=_env(), capture_output=True,
                       text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-2000:]
    lines = [l for l in r.stdout.splitlines() if l.startswith("{")]
    assert len(lines) == 1, r.stdout[-2000:]
    d = json.loads(lines[0])
    assert d["n_gpus"] == 2 and d["ranks_in_group"] == 2 and d["gather_ok"] is True and d["backend"] == "gloo"


def test_bench_launches_eight_ranks_for_the_drivers_scaling_run():
    """The command line the driver uses at N = 8 (`python bench.py --gpus 8 ...`), rehearsed on the CPU: eight ranks come up over
    gloo, rendezvous on 127.0.0.1, exchange their records once, rank 0 prints the line."""
    r = subprocess.run([sys.executable, "bench.py", "--gpus", "8", "--rehearse-launch"], cwd=ROOT, env=_env(OMP_NUM_THREADS="1"),
                       capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-2000:]
    lines = [l for l in r.stdout.splitlines() if l.startswith("{")]
    assert len(lines) == 1, r.stdout[-2000:]
    d = json.loads(lines[0])
    assert d["n_gpus"] == 8 and d["ranks_in_group"] == 8 and d["gather_ok"] is True


def test_bench_refuses_wrong_world_size():
    r = subprocess.run([sys.executable, "bench.py", "--gpus", "8", "--rehearse-launch"], cwd=ROOT,
                       env=_env(RANK="0", WORLD_SIZE="1", LOCAL_RANK="0"), capture_output=True, text=True, timeout=120)
    assert r.returncode == 2 and "WORLD_SIZE" in r.stderr and not r.stdout.strip()


def test_byte_accounting_counts_only_bytes_that_move():
    sys.path.insert(0, ROOT)
    import bench
    # a 1600x900 mask whose eroded rectangle is 100x50 pixels: 5 words x 50 rows exist, not 50 x 900
    bbox = np.array([[64, 10, 163, 59], [0x7FFFFFFF, 0x7FFFFFFF, -1, -1]], np.int32)
    assert bench.packed_rect_bytes(bbox, 50) == 4 * (163 // 32 - 64 // 32 + 1) * 50

    class HB:
        n_frames, n_masks, width, height, raw_stride, n_raw_rows, bytes_per_row = 2, 2, 1600, 900, 5, 70000, 20
        rle_counts = np.zeros(1000, np.uint32)

    class HBQ(HB):              # the quad layout: 12 bytes of a row cross HBM
        raw_stride, bytes_per_row = 3, 12
    assert bench.compulsory_bytes(HBQ, 1, 5000, "rle", True, False, 1000)["k_project_hits"] == 70000 * (12 + 4)
    by = bench.compulsory_bytes(HB, 1, 5000, "rle", True, False, 1000)
    assert by["k_project_hits"] == 70000 * (20 + 4)                       # raw rows in, hit words out, no cloud, no phantom masks
    assert bench.compulsory_bytes(HB, 1, 5000, "rle", True, True, 1000)["k_project_hits"] == 70000 * (20 + 4 + 16)
    assert bench.compulsory_bytes(HB, 1, 5000, "rle", False, True, 1000)["k_project_hits"] == 70000 * (16 + 4)
    assert by["k_rle_erode_pack_wave"] == 4000 + 1000
    full_masks = 2 * 50 * 4 * 900
    assert by["pass_total"] < full_masks + by["k_project_hits"] + 200000     # nothing near a full read of the packed masks
    assert bench.visible_cores() >= 1


def test_dumped_outputs_fit_the_budget_and_batches_do_not_depend_on_the_split(tmp_path):
    sys.path.insert(0, ROOT)
    import bench
    from cm3d_amd import synthetic as syn
    rng = np.random.default_rng(1)
    arrs = {"xyz": rng.normal(size=(50000, 3)).astype(np.float32), "idx": np.arange(60000, dtype=np.int32),
            "flags": np.array([1, 3, 0], np.int32), "none": np.zeros((0, 10))}
    for d in ("a", "b"):
        bench.dump_outputs(arrs, str(tmp_path / d), budget=400_000)
    assert sum(f.stat().st_size for f in (tmp_path / "a").iterdir()) <= 400_000
    for name in arrs:
        a, b = np.load(tmp_path / "a" / f"{name}.npy"), np.load(tmp_path / "b" / f"{name}.npy")
        assert a.dtype == (np.float32 if name == "xyz" else np.float64) and np.array_equal(a, b)
    assert np.array_equal(np.load(tmp_path / "a" / "flags.npy"), [1, 3, 0])
    # NaN / inf: written as 0, with <name>_nonfinite.npy saying which -- finite files, nothing lost, the same rows when sampled
    odd = np.where(np.arange(60000) % 7 == 0, np.inf, np.arange(60000.0))
    odd[3], odd[5] = np.nan, -np.inf
    bench.dump_outputs({"ok": np.zeros(3), "odd": odd}, str(tmp_path / "c"), budget=200_000)
    assert sorted(f.name for f in (tmp_path / "c").iterdir()) == ["odd.npy", "odd_nonfinite.npy", "ok.npy"]
    v, code = np.load(tmp_path / "c" / "odd.npy"), np.load(tmp_path / "c" / "odd_nonfinite.npy")
    assert np.isfinite(v).all() and 0 < v.size < 60000 and v.shape == code.shape and sum(f.stat().st_size for f in (tmp_path / "c").iterdir()) <= 200_000
    fin = v[code == 0]                          # odd[i] == i where finite: a sampled row keeps its value, and the rows stay in order
    assert (code == 2).any() and np.all(np.diff(fin) > 0) and np.all(fin % 7 != 0) and np.all(v[code != 0] == 0)
    bench.dump_outputs({"odd": odd}, str(tmp_path / "d"))
    assert np.array_equal(np.select([np.load(tmp_path / "d" / "odd_nonfinite.npy") == k for k in (1, 2, 3)], [np.nan, np.inf, -np.inf],
                                    np.load(tmp_path / "d" / "odd.npy")), odd, equal_nan=True)
    idx = np.load(tmp_path / "a" / "idx.npy")
    assert 0 < idx.size < 60000 and np.all(np.diff(idx) > 0)          # a sample of the rows, in their order
    cfg = syn.config("tiny")
    split = bench.make_batches_frames(cfg, [0, 20], 20, 3)
    for b, f0 in enumerate((0, 20)):
        one = [syn.make_frame(cfg, f0 + i) for i in range(20)]
        assert [f.token for f in split[b]] == [f.token for f in one]
        assert all(np.array_equal(x.sweeps_raw[0], y.sweeps_raw[0]) and x.rles == y.rles for x, y in zip(split[b], one))


def test_generation_pool_ends_under_a_blocking_sigterm_handler():
    """A profiler can install a SIGTERM handler that blocks in a forked child; the generation pool must still end (its workers take
    the default action and, on success, leave without a signal)."""
    code = ("import signal, sys, time; sys.path.insert(0, '.'); import bench; from cm3d_amd import synthetic as syn; "
            "signal.signal(signal.SIGTERM, lambda *a: time.sleep(1e9)); "
            "print(len(bench.make_batches_frames(syn.config('tiny'), [0, 16], 16, 2)[1]))")
    r = subprocess.run([sys.executable, "-c", code], cwd=ROOT, capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and r.stdout.strip() == "16", r.stderr[-2000:]
