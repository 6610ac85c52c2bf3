"""Masks of different image sizes in one batch, host side: lifting.pack_frames' canvas and size table, what it refuses, the
Waymo loader on a frame with two mask sizes, and -- with the CPU oracle -- rule R itself: the in-mask lists of a mask eroded at its
own size equal those of the mask pasted into a canvas of zeros and eroded there."""
import dataclasses

import numpy as np
import pytest

from cm3d_amd import lifting, rle, synthetic as syn
from tests import mask_cases as C
from tests import mixed_size_cases as X


def _lanes(frames):
    return [syn.make_lane_table(frames[0].ego_xyz[:2], 500, seed=3)]


# ----------------------------------------------------------------------------- embed_runs
@pytest.mark.parametrize("case", X.kernel_cases(), ids=lambda c: c[0].split(":")[0])
def test_embed_runs_is_pasting_into_a_canvas_of_zeros(case):
    _, W, H, sizes, lists = case
    for (w, h), c in zip(sizes, lists):
        e = X.embed_runs(c, w, h, W, H)
        assert int(e.astype(np.int64).sum()) == W * H
        assert np.array_equal(rle.counts_to_dense(e, W, H), X.paste(rle.counts_to_dense(c, w, h), W, H))
        ones = e[1::2]
        assert (ones[:-1] > 0).all() and (e[2::2][:ones.size - 1] > 0).all() if ones.size > 1 else True      # no zero-length runs inside
    with pytest.raises(ValueError):
        X.embed_runs([10], 5, 2, 4, 4)
    with pytest.raises(ValueError):
        X.embed_runs([9], 5, 2, 8, 4)


def test_case_table_reaches_what_it_is_built_for():
    cases = X.kernel_cases()
    W, H = X.SMALL_CANVAS
    assert {s for c in cases[:len(X.SMALL_SIZES)] for s in c[3]} == set(X.SMALL_SIZES)
    # own-size erosion keeps the last own row and column of an all-ones mask, rule R does not
    for w, h in [(95, 40), (96, 39), (65, 33)]:
        own = C.erode_ref(np.ones((h, w), np.uint8))
        r = C.erode_ref(X.paste(np.ones((h, w), np.uint8), W, H))
        assert own.all()
        assert r[:h, :w].sum() == (w - (w < W)) * (h - (h < H)) and r.sum() == r[:h, :w].sum()
    # a kernel that decoded the wrapping run with the canvas width would shear it
    wrap = dict(X.family(65, 33))["run that wraps across an own row end"]
    c = rle.dense_to_counts(wrap)
    assert c.size == 3 and not np.array_equal(rle.counts_to_dense(np.concatenate([c, [W * H - 65 * 33]]), W, H), X.paste(wrap, W, H))
    # the sized call and the plain call on the embedded lists take the same form (a wave per mask up to 1024 runs per mask on average)
    for _, cw, ch, sizes, lists in cases:
        emb = [X.embed_runs(c, w, h, cw, ch) for c, (w, h) in zip(lists, sizes)]
        assert (sum(c.size for c in lists) <= 1024 * len(lists)) == (sum(c.size for c in emb) <= 1024 * len(lists))
    big = [c for c in cases if "3373" in c[0]][0]
    assert sum(c.size for c in big[4]) > 1024 * len(big[4])
    assert big[4][0].size == 3373 > 2048
    assert any(c[1] == 4096 for c in cases)


# ----------------------------------------------------------------------------- pack_frames
def test_pack_frames_takes_masks_of_three_sizes():
    fr, = X.mixed_tiny_frames(1, all_ones=False)
    assert fr.cams.shape[0] == 5 and (fr.width, fr.height) == (X.TINY_W, X.TINY_H)
    hb = lifting.pack_frames([fr], _lanes([fr]), [0])
    assert (hb.width, hb.height) == (256, 144)
    want = np.array([r["size"] for r in fr.rles], np.int32)
    assert hb.mask_wh.dtype == np.int32 and np.array_equal(hb.mask_wh, want)
    cams = np.asarray(fr.cam_nums)
    assert (want[(cams == 3) | (cams == 4)] == X.SIDE).all() and ((cams == 3) | (cams == 4)).any()
    assert (want == X.ODD).all(axis=1).sum() == 1 and (want == (256, 144)).all(axis=1).any()
    # the run lists are the producer's, untouched
    assert np.array_equal(hb.rle_counts, np.concatenate([rle.string_to_counts(r["counts"]) for r in fr.rles]))
    assert np.array_equal(np.diff(hb.rle_off), [rle.string_to_counts(r["counts"]).size for r in fr.rles])


def test_canvas_is_the_maximum_over_frames_and_masks():
    a, = X.mixed_tiny_frames(1, all_ones=False)
    b = X.crop_frame(syn.make_frame(syn.config("tiny", n_cams=5), 1), {c: (180, 144) for c in range(5)})
    b.width, b.height = 180, 144
    hb = lifting.pack_frames([a, b], _lanes([a]), [0, 0])
    assert (hb.width, hb.height) == (256, 144) and hb.mask_wh.shape == (hb.n_masks, 2)
    assert (hb.mask_wh[hb.mask_off[1]:] == (180, 144)).all()
    # a frame object may understate its images: the masks count too
    b.width, b.height = 100, 50
    assert (lifting.pack_frames([b], _lanes([a]), [0]).width, lifting.pack_frames([b], _lanes([a]), [0]).height) == (180, 144)


def test_single_size_batch_is_packed_as_before():
    cfg = syn.config("tiny")
    frames = [syn.make_frame(cfg, i) for i in range(3)]
    for layout in ("rows", "quads"):
        hb = lifting.pack_frames(frames, _lanes(frames), [0, 0, 0], layout=layout)
        assert hb.mask_wh is None and (hb.width, hb.height) == (cfg.width, cfg.height)
        # field for field what the frames hold (the arrays the parent commit packed; tests/golden pins them through the GPU tests)
        assert np.array_equal(hb.rle_counts, np.concatenate([rle.string_to_counts(r["counts"]) for f in frames for r in f.rles]))
        assert np.array_equal(hb.mask_off, np.concatenate([[0], np.cumsum([len(f.rles) for f in frames])]))
        assert np.array_equal(hb.mask_cam, np.concatenate([f.cam_nums for f in frames]))
        assert np.array_equal(hb.cams, np.stack([f.cams for f in frames]))
        # ... and the same HostBatch, array for array, as a batch whose table says "canvas size" for every mask
        same = lifting.pack_frames([X.crop_frame(f, {c: (cfg.width, cfg.height) for c in range(6)}) for f in frames], _lanes(frames), [0, 0, 0],
                                   layout=layout)
        for fld in dataclasses.fields(hb):
            u, v = getattr(hb, fld.name), getattr(same, fld.name)
            assert (np.array_equal(u, v, equal_nan=True) if isinstance(u, np.ndarray) else u == v), fld.name


def test_what_pack_frames_refuses():
    fr, = X.mixed_tiny_frames(1, all_ones=False)
    lanes = _lanes([fr])
    k = [int(c) for c in fr.cam_nums].index(3) if 3 in fr.cam_nums else [int(c) for c in fr.cam_nums].index(4)
    # a run list that covers the canvas, not the mask's own size
    bad = X.crop_frame(fr, {})
    bad.rles[k] = {"size": list(X.SIDE), "counts": rle.counts_to_string(np.array([256 * 144], np.uint32))}
    with pytest.raises(ValueError, match="do not cover"):
        lifting.pack_frames([bad], lanes, [0])
    wide = X.crop_frame(fr, {})
    wide.rles[k] = {"size": [4097, 2], "counts": rle.counts_to_string(np.array([4097 * 2], np.uint32))}
    with pytest.raises(ValueError, match="4096"):
        lifting.pack_frames([wide], lanes, [0])
    ok = X.crop_frame(fr, {})
    ok.rles[k] = {"size": [4096, 2], "counts": rle.counts_to_string(np.array([4096 * 2], np.uint32))}
    assert lifting.pack_frames([ok], lanes, [0]).width == 4096


def test_dense_route_refuses_a_mixed_batch():
    from cm3d_amd import pipeline_waymo as pw
    frames = X.mixed_tiny_frames(2, waymo=True)
    classes = lifting.ClassTable.waymo()
    lanes = _lanes(frames)[0]
    hb = lifting.pack_frames(frames, [lanes], [0, 0], classes)
    with pytest.raises(ValueError, match="dense"):
        lifting.require_one_mask_size(hb)
    with pytest.raises(ValueError, match="dense"):      # the entry point's --masks dense: refused before anything reaches the device
        pw.lift_scene(None, frames, lanes, classes, masks="dense")
    single = [syn.make_waymo_frame(syn.config("tiny", n_cams=5), 0)]
    lifting.require_one_mask_size(lifting.pack_frames(single, [lanes], [0], classes))


# ----------------------------------------------------------------------------- rule R, with the oracle
def test_rule_r_own_size_lists_equal_zero_canvas_lists(oracle):
    """oracle.points_in_mask on erode3x3(own-size mask) == on erode3x3(mask pasted into a zero canvas): the argument of
    include/cm3d_hip.h on six frames, every mask cropped to five sizes, pixels set on purpose in the last three own rows and columns."""
    cfg = syn.config("tiny")
    W, H = cfg.width, cfg.height
    sizes = [(W, H), (W, 100), (200, H), (255, 143), (97, 65)]
    rng = np.random.default_rng(5)
    n_cases = n_hits = n_band = 0
    for i in range(6):
        fr = syn.make_frame(cfg, i)
        pts = np.concatenate([oracle.sweep_prep(r, x[0:9], x[9:12], x[12:21], x[21:24], oracle.EGO_HALFW_F32)
                              for r, x in zip(fr.sweeps_raw, fr.sweep_xf)], 0)
        for rl, cam in zip(fr.rles, fr.cam_nums):
            full = rle.counts_to_dense(rle.string_to_counts(rl["counts"]), W, H)
            uv = oracle.project_points(pts, fr.cams[cam])
            for w, h in sizes:
                own = full[:h, :w].copy()
                own[h - 3:, :] |= rng.random((3, w)) < 0.5
                own[:, w - 3:] |= rng.random((h, 3)) < 0.5
                a = oracle.points_in_mask(pts, fr.cams[cam], oracle.erode3x3(own))
                b = oracle.points_in_mask(pts, fr.cams[cam], oracle.erode3x3(X.paste(own, W, H)))
                assert np.array_equal(a, b), (i, cam, w, h)
                n_cases += 1
                n_hits += a.size
                n_band += int(((uv[:, 2] > 0) & (np.floor(uv[:, 1]) >= h - 1) & (uv[:, 1] < H - 1) & (uv[:, 0] >= 1) & (uv[:, 0] < w - 1)).sum()) if h < H else 0
    assert n_cases == 240 and n_hits > 1000 and n_band > 0      # points do fall where the two erosions differ


# ----------------------------------------------------------------------------- the Waymo loader
def test_waymo_load_scene_with_two_mask_sizes_in_a_frame(tmp_path):
    from cm3d_amd import pipeline_waymo as pw
    scene = "segment-mixed-0"
    frames = X.write_waymo_scene(tmp_path, scene, X.mixed_tiny_frames(2, waymo=True))
    assert all(len({tuple(r["size"]) for r in f.rles}) >= 2 for f in frames)
    loaded, lanes = pw.load_scene(str(tmp_path / "frames"), str(tmp_path / "masks"), scene)
    assert len(loaded) == 2 and all((f.width, f.height) == (X.TINY_W, X.TINY_H) for f in loaded)
    hb = lifting.pack_frames(loaded, [lanes], [0, 0], lifting.ClassTable.waymo())
    assert (hb.width, hb.height) == (X.TINY_W, X.TINY_H)
    assert np.array_equal(hb.mask_wh, np.array([r["size"] for f in frames for r in f.rles], np.int32))
