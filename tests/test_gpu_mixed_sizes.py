"""Masks of different image sizes in one batch, on the device.

Kernel level: cm3d_rle_erode_pack_sized on the producer's run lists against cm3d_rle_erode_pack on tests.mixed_size_cases.embed_runs of
them (rule R of include/cm3d_hip.h: the mask pasted top-left into a canvas of zeros) and against plain numpy, bit for bit, including
what must NOT be written -- in the form the product picks and in every forced form.
Engine level: mixed frames against the oracle (which decodes and erodes every mask at its own size, like the reference), the sized
path against the plain one on a single-size batch, slots and captured graphs that change between mixed and single-size batches, and
the Waymo and KITTI entry points on inputs with two image sizes."""
import dataclasses
import json
import os
import pickle
import subprocess
import sys

import numpy as np
import pytest

from cm3d_amd import rle, synthetic as syn
from tests import mask_cases as C
from tests import mixed_size_cases as X
from tests.helpers import oracle_batch

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
_HOOKS = ("CM3D_RLE_FORM", "CM3D_RLE_BANDS", "CM3D_RLEW_LDS_WORDS")


# ----------------------------------------------------------------------------- kernel level
def _wave_form(n_masks, total_runs):
    forced = os.environ.get("CM3D_RLE_FORM")
    return forced[0] == "w" if forced else total_runs <= 1024 * n_masks


def _first_difference(what, name, got, want, n):
    i, q = (int(v[0]) for v in np.nonzero(got != want))
    msg = (f"{what}: {'guard slot' if i >= n else f'mask {i}'}, slot word {q}: expected {int(want[i, q]):#010x}, got {int(got[i, q]):#010x}; "
           f"{int((got != want).sum())} words differ; case {name}")
    print(msg)
    return msg


def run_kernel_case(case):
    """One case through the sized kernel and, embedded, through the plain one: all eight bbox ints and every word of `packed` --
    the stored rectangles, the fill around them, the guard slot -- equal each other and the numpy expectation."""
    from cm3d_amd import ops
    name, W, H, sizes, lists = case
    Wp, n = (W + 31) // 32, len(lists)
    emb = [X.embed_runs(c, w, h, W, H) for c, (w, h) in zip(lists, sizes)]
    wave = _wave_form(n, sum(c.size for c in lists))
    assert wave == _wave_form(n, sum(c.size for c in emb)), f"the two calls would take different forms; case {name}"
    pasted = np.stack([X.paste(rle.counts_to_dense(c, w, h), W, H) for c, (w, h) in zip(lists, sizes)])
    exp = C.erode_ref(pasted)
    exp_words, rects = C.pack_words(exp), C.word_rects(pasted)
    whole = np.tile(np.array([0, 0, Wp, H], np.int32), (n, 1))
    want_bbox = np.concatenate([C.bounds(exp), rects if wave else np.where(rects[:, 2:3] > 0, whole, 0)], axis=1)
    want = np.full((n + 1, H * Wp), C.FILL, np.uint32)
    for i, (xw0, y0, wc, rows) in enumerate(rects.tolist()):
        if wc:
            crop = exp_words[i, y0:y0 + rows, xw0:xw0 + wc]
            if wave:
                want[i, :rows * wc] = crop.reshape(-1)
            else:
                want[i].reshape(H, Wp)[y0:y0 + rows, xw0:xw0 + wc] = crop
    p_s, b_s = ops.erode_rle(lists, W, H, fill=C.FILL, guard_slots=1, sizes=sizes)
    p_p, b_p = ops.erode_rle(emb, W, H, fill=C.FILL, guard_slots=1)
    got_s = p_s.cpu().numpy().view(np.uint32).reshape(n + 1, H * Wp)
    got_p = p_p.cpu().numpy().view(np.uint32).reshape(n + 1, H * Wp)
    b_s, b_p = b_s.cpu().numpy(), b_p.cpu().numpy()
    form = "wave form" if wave else "workgroup form"
    for what, bb in ((f"sized kernel ({form}) against the plain kernel on the embedded lists", b_p), (f"sized kernel ({form}) against numpy", want_bbox)):
        if not np.array_equal(b_s, bb):
            i = int(np.nonzero((b_s != bb).any(axis=1))[0][0])
            msg = f"{what}: mask {i} own size {sizes[i]}: expected bbox {bb[i].tolist()}, got {b_s[i].tolist()}; case {name}"
            print(msg)
            raise AssertionError(msg)
    if not np.array_equal(got_s, got_p):
        raise AssertionError(_first_difference(f"sized kernel ({form}) against the plain kernel on the embedded lists", name, got_s, got_p, n))
    if not np.array_equal(got_s, want):
        raise AssertionError(_first_difference(f"sized kernel ({form}) against numpy", name, got_s, want, n))


def run_kernel_cases():
    for case in X.kernel_cases():
        run_kernel_case(case)


def test_sized_kernels_in_the_form_the_product_picks(monkeypatch):
    for v in _HOOKS:
        monkeypatch.delenv(v, raising=False)
    cases = X.kernel_cases()
    forms = {_wave_form(len(c[4]), sum(l.size for l in c[4])) for c in cases}
    assert forms == {True, False}          # the 3373-run batch takes the workgroup form, the others a wave per mask
    run_kernel_cases()


_CHILD = """
import sys
sys.path.insert(0, {root!r})
from tests import test_gpu_mixed_sizes as T
T.run_kernel_cases()
print("MIXED OK")
"""

_SETTINGS = [
    {"CM3D_RLE_FORM": "wave"},
    {"CM3D_RLE_FORM": "block"},
    {"CM3D_RLE_FORM": "wave", "CM3D_RLE_BANDS": "2"},
    {"CM3D_RLE_FORM": "wave", "CM3D_RLE_BANDS": "4"},
    {"CM3D_RLE_FORM": "wave", "CM3D_RLEW_LDS_WORDS": "512"},
    {"CM3D_RLE_FORM": "wave", "CM3D_RLEW_LDS_WORDS": "390"},
]


@pytest.mark.parametrize("env", _SETTINGS, ids=["wave", "block", "wave-bands2", "wave-bands4", "wave-lds512", "wave-lds390"])
def test_sized_kernels_in_every_forced_form(env):
    """The settings are read once per process, hence a child per setting (as tests/test_gpu_mask_edges.py does it)."""
    base = {k: v for k, v in os.environ.items() if k not in _HOOKS}
    r = subprocess.run([sys.executable, "-c", _CHILD.format(root=ROOT)], env=dict(base, **env), capture_output=True, text=True, timeout=300,
                       cwd=ROOT)
    assert r.returncode == 0 and "MIXED OK" in r.stdout, f"exit status {r.returncode}\n{r.stdout[-3000:]}\n{r.stderr[-3000:]}"


def test_sized_entry_points_check_their_arguments():
    """The canvas checks of the plain pair, and a table is required; a table with values outside [1, W] x [1, H] is clamped on the
    device and writes nothing outside the masks' slots."""
    import torch
    from cm3d_amd import _lib, ops
    L = _lib.lib()
    dev = torch.device("cuda", torch.cuda.current_device())
    st = torch.cuda.current_stream().cuda_stream
    H = 3
    off = torch.tensor([0, 1], dtype=torch.int32, device=dev)
    wh = torch.tensor([[1, 1]], dtype=torch.int32, device=dev)
    packed = torch.full((4200,), 0x5A5A5A5A, dtype=torch.int32, device=dev)
    bbox = torch.full((_lib.BBOX_STRIDE,), 0x5A5A5A5A, dtype=torch.int32, device=dev)
    ws = torch.zeros(max(int(L.cm3d_rle_workspace_bytes(1)), 16), dtype=torch.uint8, device=dev)
    cnts = torch.tensor([1], dtype=torch.int32, device=dev)
    for W, table in ((0, wh.data_ptr()), (4097, wh.data_ptr()), (64, 0)):
        assert L.cm3d_rle_erode_pack_sized(cnts.data_ptr(), off.data_ptr(), 1, 1, W, H, table, packed.data_ptr(), bbox.data_ptr(), ws.data_ptr(),
                                           ws.numel(), st) == -1
        assert L.cm3d_rle_erode_pack_sized_begin(cnts.data_ptr(), off.data_ptr(), 1, 1, W, H, table, packed.data_ptr(), bbox.data_ptr(),
                                                 ws.data_ptr(), ws.numel(), bbox.data_ptr(), bbox.data_ptr(), 1, 0, 0, st) == -1
    torch.cuda.synchronize()
    assert bool((packed == 0x5A5A5A5A).all()) and bool((bbox == 0x5A5A5A5A).all())
    with pytest.raises(ValueError):
        ops.erode_rle([np.array([6], np.uint32)], 3, 2, sizes=[(3, 2), (3, 2)])
    # sizes outside the canvas: clamped to it, so the lists are read as canvas-sized ones
    W, H = 70, 9
    m = (np.random.default_rng(3).random((H, W)) < 0.9).astype(np.uint8)
    lists = [rle.dense_to_counts(m)] * 3
    p_s, b_s = ops.erode_rle(lists, W, H, fill=C.FILL, guard_slots=1, sizes=[(W + 50, H + 7), (1 << 30, 1 << 30), (W, H)])
    p_p, b_p = ops.erode_rle(lists, W, H, fill=C.FILL, guard_slots=1)
    assert torch.equal(p_s, p_p) and torch.equal(b_s, b_p)
    # sizes below 1: clamped to 1 x 1 -- the list overruns that image and is cut off after its first pixel
    p_s, b_s = ops.erode_rle([np.array([0, W * H], np.uint32)] * 2, W, H, fill=C.FILL, guard_slots=1, sizes=[(0, -5), (-(1 << 31), 0)])
    got = p_s.cpu().numpy().view(np.uint32).reshape(3, -1)
    assert (got[:, 1:] == C.FILL).all() and (got[2] == C.FILL).all() and (got[:2, 0] == 0).all()
    assert b_s.cpu().numpy().tolist() == [[C.INT_MAX, C.INT_MAX, -1, -1, 0, 0, 1, 1]] * 2


# ----------------------------------------------------------------------------- engine level
def _lanes(frames, seed=1):
    return [syn.make_lane_table(frames[0].ego_xyz[:2], 2000, seed=seed)]


def _eager(hb, **kw):
    import torch
    from cm3d_amd import lifting
    eng = lifting.LiftEngine(**kw)
    eng.upload(hb)
    eng.run(masks="rle")
    torch.cuda.synchronize()
    return eng.download()


def _rule_r_bbox(oracle, frames, W, H):
    """Bounds of every mask eroded at its own size, its last row cleared where h < H and its last column where w < W."""
    out = []
    for fr in frames:
        for r in fr.rles:
            er = oracle.erode3x3(oracle.rle_decode(r).T)
            h, w = er.shape
            if h < H:
                er[h - 1, :] = 0
            if w < W:
                er[:, w - 1] = 0
            ys, xs = np.nonzero(er)
            out.append([xs.min(), ys.min(), xs.max(), ys.max()] if xs.size else [C.INT_MAX, C.INT_MAX, -1, -1])
    return np.array(out, np.int32)


def test_mixed_frames_against_the_oracle(oracle):
    from cm3d_amd import lifting
    from tests import test_gpu_parity as P
    frames = X.mixed_tiny_frames(4)
    lanes, fl = _lanes(frames), [0] * 4
    hb = lifting.pack_frames(frames, lanes, fl)
    W, H = hb.width, hb.height
    assert (W, H) == (X.TINY_W, X.TINY_H) and hb.mask_wh is not None
    assert {tuple(s) for s in hb.mask_wh.tolist()} == {(W, H), X.SIDE, X.ODD}
    exp = oracle_batch(oracle, frames, lanes, fl, hb)
    # the condition that makes this a test of rule R: points of each cropped camera do project into the rows the crop took away --
    # and into row h-1 itself, which own-size erosion of the all-ones masks keeps and rule R clears
    w, h = X.SIDE
    for cam in (3, 4):
        band = last_row = 0
        for f, fr in enumerate(frames):
            uv = oracle.project_points(exp["points"][exp["pt_off"][f]:exp["pt_off"][f + 1]], fr.cams[cam])
            ok = (uv[:, 2] > lifting.MIN_DIST) & (uv[:, 0] >= 1) & (uv[:, 0] < W - 1) & (uv[:, 1] < H - 1)
            band += int((ok & (np.floor(uv[:, 1]) >= h - 1)).sum())
            last_row += int((ok & (np.floor(uv[:, 1]) == h - 1)).sum())
        assert band > 0 and last_row > 0, (cam, band, last_row)
    got = _eager(hb, keep_colsum=True)
    assert exp["hit_idx"].size > 50
    P._compare(hb, got, dict(exp, bbox=_rule_r_bbox(oracle, frames, W, H)))


@pytest.mark.parametrize("fused_reset", ["1", "0"])
def test_single_size_batch_through_the_sized_path(monkeypatch, fused_reset):
    """An explicit all-canvas table sends a single-size batch through the sized kernels (with the per-pass reset on the launch, and
    without): hit lists, medoids and boxes bit for bit those of the plain path."""
    from cm3d_amd import lifting
    monkeypatch.setenv("CM3D_FUSED_RESET", fused_reset)
    cfg = syn.config("tiny")
    frames = [syn.make_frame(cfg, 20 + i) for i in range(4)]
    lanes = _lanes(frames)
    hb = lifting.pack_frames(frames, lanes, [0] * 4)
    assert hb.mask_wh is None
    plain = _eager(hb)
    table = np.tile(np.array([hb.width, hb.height], np.int32), (hb.n_masks, 1))
    sized = _eager(dataclasses.replace(hb, mask_wh=table))
    assert plain["hit_idx"].size > 50 and set(plain) == set(sized)
    for k in plain:
        assert np.array_equal(plain[k], sized[k], equal_nan=True), k


def _three_batches():
    from cm3d_amd import lifting
    cfg = syn.config("tiny", n_cams=5)
    a = X.mixed_tiny_frames(3, first=0)
    b = [syn.make_frame(cfg, 40 + i) for i in range(2)]
    c = X.mixed_tiny_frames(3, first=60, side=(230, 90))
    out = []
    for k, fs in enumerate((a, b, c)):
        out.append(lifting.pack_frames(fs, _lanes(fs, seed=k), [0] * len(fs)))
    assert out[0].mask_wh is not None and out[1].mask_wh is None and out[2].mask_wh is not None
    assert not np.array_equal(out[0].mask_wh[:4], out[2].mask_wh[:4])
    return out


def _same(a, b, what):
    assert set(a) == set(b)
    for k in a:
        assert np.array_equal(a[k], b[k], equal_nan=True), (what, k)


def test_slots_that_change_between_mixed_and_single_size():
    """LiftPipeline(depth=2): mixed, single-size, mixed with another table, then the first two again -- so that a slot that held a
    mixed batch takes a single-size one and the reverse.  Every batch equals its eager result on an engine of its own."""
    from cm3d_amd import lifting
    hbs = _three_batches()
    eager = [_eager(hb) for hb in hbs]
    assert all(e["hit_idx"].size > 20 for e in eager)
    pipe = lifting.LiftPipeline("cuda:0", depth=2)
    order = [0, 1, 2, 0, 1]                 # slots 0 1 0 1 0: slot 0 mixed -> mixed' -> single, slot 1 single -> mixed
    pending = []
    for k in order:
        if len(pending) == pipe.depth:
            slot, j = pending.pop(0)
            _same(pipe.collect(slot)[1], eager[j], f"batch {j} in slot {slot}")
        pending.append((pipe.submit(hbs[k], masks="rle"), k))
    for slot, j in pending:
        _same(pipe.collect(slot)[1], eager[j], f"batch {j} in slot {slot}")


def test_graphs_of_one_engine_that_changes_between_mixed_and_single_size():
    """One engine takes the three batches one after the other; each pass is captured and replayed: the replay gives the eager result."""
    import torch
    from cm3d_amd import lifting
    hbs = _three_batches()
    eager = [_eager(hb) for hb in hbs]
    eng = lifting.LiftEngine()
    for j in (0, 1, 2, 1):
        eng.upload(hbs[j])
        eng.run(masks="rle")
        torch.cuda.synchronize()
        _same(eng.download(), eager[j], f"batch {j}, eager")
        g = eng.capture_graph(masks="rle")
        eng.b.hit_idx.fill_(-7); eng.b.box.fill_(0); eng.b.packed.fill_(-1); eng.b.bbox.fill_(0)
        g.replay()
        torch.cuda.synchronize()
        _same(eng.download(), eager[j], f"batch {j}, replay")
        del g


def test_dense_route_refuses_a_mixed_batch_on_the_engine():
    from cm3d_amd import lifting
    frames = X.mixed_tiny_frames(1)
    hb = lifting.pack_frames(frames, _lanes(frames), [0])
    eng = lifting.LiftEngine()
    eng.upload(hb)
    with pytest.raises(ValueError, match="dense"):
        eng.decode_masks_dense()
    with pytest.raises(ValueError, match="dense"):
        eng.run(masks="dense")


# ----------------------------------------------------------------------------- entry points
def test_waymo_entry_point_with_two_mask_sizes_in_a_frame(tmp_path, oracle):
    """src/waymo/2d_to_3d.py on a scene whose frames hold masks of 256x144 and 256x100 (and one of 200x144), against the oracle on the
    same files, checked the way tests/test_gpu_entrypoint.py::test_waymo_entry_point checks its single-size scene."""
    from cm3d_amd import lifting, pipeline_waymo as pw, waymo as wm
    scene = "segment-mixed-0"
    written = X.write_waymo_scene(tmp_path, scene, X.mixed_tiny_frames(3, waymo=True))
    assert all(len({tuple(r["size"]) for r in f.rles}) >= 2 for f in written)
    out = tmp_path / "out" / "pred.bin"
    r = subprocess.run([sys.executable, "2d_to_3d.py", "--frames-dir", str(tmp_path / "frames"), "--mask-dir", str(tmp_path / "masks"),
                        "--output", str(out)], cwd=os.path.join(ROOT, "src", "waymo"), capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-2000:]
    blob = open(out, "rb").read()
    frames, lanes = pw.load_scene(str(tmp_path / "frames"), str(tmp_path / "masks"), scene)
    classes = lifting.ClassTable.waymo()
    hb = lifting.pack_frames(frames, [lanes], [0] * len(frames), classes)
    assert hb.mask_wh is not None
    exp = oracle_batch(oracle, frames, [lanes], [0] * len(frames), hb)
    exp_objs = wm.objects_from_results(hb, exp, classes, [(f.context_name, f.timestamp_micros) for f in frames])
    assert f"wrote {len(exp_objs)} objects" in r.stdout
    got, want = wm.decode_objects(blob), wm.decode_objects(wm.encode_objects(exp_objs))
    assert len(got) == len(want) > 0
    for a, b in zip(got, want):
        assert (a["type"], a["id"], a["context_name"], a["timestamp_micros"], a["score"]) == (b["type"], b["id"], b["context_name"], b["timestamp_micros"], b["score"])
        assert (a["width"], a["length"], a["height"]) == (b["width"], b["length"], b["height"])
        assert np.allclose(a["center"] + [a["heading"]], b["center"] + [b["heading"]], rtol=0, atol=1e-4)


def test_kitti_entry_point_with_frames_of_two_sizes(tmp_path, oracle):
    """src/kitti/2d_to_3d.py --batch 64 --obb host on frames of 320x96 and 310x94: one upload, label files string for string the
    oracle's through the same label writer."""
    from cm3d_amd import kitti as kt, lifting
    kdir, mdir = tmp_path / "kitti", tmp_path / "masks"
    for d in (kdir / "training" / "velodyne", kdir / "training" / "calib", mdir):
        os.makedirs(d)
    cfgs = [syn.config("tiny", width=320, height=96, ratio=0.2, n_masks=10), syn.config("tiny", width=310, height=94, ratio=0.2, n_masks=10)]
    n = 4
    for i in range(n):
        cfg = cfgs[i % 2]
        fr, cal = syn.make_kitti_frame(cfg, i)
        fr.sweeps_raw[0].astype(np.float32).tofile(kdir / "training" / "velodyne" / f"{i:06d}.bin")
        with open(kdir / "training" / "calib" / f"{i:06d}.txt", "w") as fh:
            for k, v in cal.items():
                fh.write(f"{k}: " + " ".join(repr(float(x)) for x in np.asarray(v).reshape(-1)) + "\n")
        pickle.dump(fr.rles, open(mdir / f"{i}_masks.pkl", "wb"))
        json.dump({"labels": fr.labels, "detection_scores": fr.scores}, open(mdir / f"{i}_data.json", "w"))
    r = subprocess.run([sys.executable, "2d_to_3d.py", "--kitti-dir", str(kdir), "--mask-dir", str(mdir), "--ratio", "0.2", "--batch", "64",
                        "--obb", "host"], cwd=os.path.join(ROOT, "src", "kitti"), capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-2000:]
    frames = []
    for i in range(n):
        rles = pickle.load(open(mdir / f"{i}_masks.pkl", "rb"))
        data = json.load(open(mdir / f"{i}_data.json"))
        frames.append(kt.frame_from_files(i, str(kdir / "training" / "velodyne" / f"{i:06d}.bin"), str(kdir / "training" / "calib" / f"{i:06d}.txt"),
                                          rles, data["labels"], data["detection_scores"], 0.2))
    assert {(f.width, f.height) for f in frames} == {(320, 96), (310, 94)}
    hb = lifting.pack_frames(frames, [[[0.0, 0.0, 0.0]]], [0] * n)
    assert (hb.width, hb.height) == (320, 96) and hb.mask_wh is not None
    exp = oracle_batch(oracle, frames, [np.zeros((1, 3))], [0] * n, hb)
    per_mask_frame = np.repeat(np.arange(n), np.diff(hb.mask_off))
    exp["hit_xyz"] = exp["points"][np.repeat(exp["pt_off"][per_mask_frame], np.diff(exp["hit_off"])) + exp["hit_idx"]]
    total = 0
    for i in range(n):
        pred = open(kdir / "training" / "pred" / f"{i:06d}.txt").read().splitlines()
        pseudo = open(kdir / "training" / "pseudo" / f"{i:06d}.txt").read().splitlines()
        want_pred, want_pseudo = kt.labels_of_frame(hb, exp, i, lifting.ClassTable.nuscenes(), lifting.SHAPE_PRIORS_CHATGPT)
        assert pred == [l.rstrip("\n") for l in want_pred] and pseudo == [l.rstrip("\n") for l in want_pseudo], i
        total += len(pred)
    assert total > 3 and f"wrote {total} labels" in r.stdout
