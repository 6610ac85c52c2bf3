"""Masks of different image sizes in one batch (cm3d_rle_erode_pack_sized, lifting.pack_frames): the expected-value generator and
the case tables of tests/test_mixed_sizes_host.py and tests/test_gpu_mixed_sizes.py.  numpy only, no GPU, no torch.

RULE R (include/cm3d_hip.h): a mask of its own size (w, h) <= the batch's canvas (W, H) is stored as if it had been pasted top-left
into a W x H canvas of zeros and eroded there.  `embed_runs` does the pasting on run lists -- the host re-encode the product
avoids --, so the plain kernel on embed_runs(list) is what the sized kernel must give on the list itself."""
import copy
import functools

import numpy as np

from cm3d_amd import rle
from tests import mask_cases as C


# ----------------------------------------------------------------------------- helpers
def embed_runs(counts, w, h, W, H):
    """Run list over the row-major w x h image -> run list over the W x H canvas that holds the image top-left and zeros elsewhere.
    Every 1-run is cut at its own row ends, its pieces move to the canvas's row stride, pieces that touch again (w == W) are joined."""
    c = np.asarray(counts, np.int64)
    if not (1 <= w <= W and 1 <= h <= H) or int(c.sum()) != w * h:
        raise ValueError("embed_runs: the list does not cover w x h, or w x h does not fit the canvas")
    ends = np.cumsum(c)
    s1, e1 = (ends - c)[1::2], ends[1::2]               # the 1-runs [s1, e1)
    s1, e1 = s1[e1 > s1], e1[e1 > s1]
    if s1.size == 0:
        return np.array([W * H], np.uint32)
    ys, ye = s1 // w, (e1 - 1) // w
    nrows = ye - ys + 1
    k = np.repeat(np.arange(s1.size), nrows)
    row = np.repeat(ys, nrows) + np.arange(int(nrows.sum())) - np.repeat(np.cumsum(nrows) - nrows, nrows)
    p0 = np.maximum(s1[k], row * w) - row * w + row * W
    p1 = np.minimum(e1[k], (row + 1) * w) - row * w + row * W
    join = p0[1:] == p1[:-1]
    p0, p1 = p0[np.concatenate([[True], ~join])], p1[np.concatenate([~join, [True]])]
    return C.spans_to_runs(p0, p1, W * H)


def paste(mask_hw, W, H):
    """(h, w) mask -> (H, W) canvas of zeros with the mask top-left."""
    m = np.asarray(mask_hw)
    out = np.zeros((H, W), np.uint8)
    out[:m.shape[0], :m.shape[1]] = m != 0
    return out


def crop_rle(rl, w, h):
    """COCO RLE dict -> the dict of its top-left w x h crop, as a producer that thumbnails the smaller image would write it."""
    W, H = rl["size"]
    cnts = rle.string_to_counts(rl["counts"]) if isinstance(rl["counts"], (bytes, bytearray)) else np.asarray(rl["counts"], np.uint32)
    return rle.encode_mask(rle.counts_to_dense(cnts, W, H)[:h, :w])


def crop_frame(frame, cam_sizes, mask_sizes=None, ones=()):
    """A copy of `frame` whose masks of the cameras in cam_sizes ({cam: (w, h)}) are cropped to that camera's size and re-encoded;
    mask_sizes ({mask index: (w, h)}) crops single masks; every camera listed in `ones` gets one more mask, all ones, of that
    camera's size (label of mask 0, score 0.5).  width / height keep their meaning of "this frame's largest image"."""
    fr = copy.copy(frame)
    fr.rles, fr.labels, fr.scores, fr.cam_nums = list(frame.rles), list(frame.labels), list(frame.scores), list(frame.cam_nums)
    for i, (rl, cam) in enumerate(zip(frame.rles, frame.cam_nums)):
        size = (mask_sizes or {}).get(i, cam_sizes.get(int(cam)))
        if size is not None:
            fr.rles[i] = crop_rle(rl, *size)
    for cam in ones:
        w, h = cam_sizes.get(int(cam), (frame.width, frame.height))
        fr.rles.append(rle.encode_mask(np.ones((h, w), np.uint8)))
        fr.labels.append(frame.labels[0]); fr.scores.append(0.5); fr.cam_nums.append(int(cam))
    return fr


# ----------------------------------------------------------------------------- kernel-level cases
SMALL_CANVAS = (96, 40)
SMALL_SIZES = [(96, 40), (95, 40), (96, 39), (65, 33), (64, 32), (63, 31), (33, 7), (32, 3), (31, 3), (3, 3), (2, 2), (1, 1)]


def family(w, h):
    """[(label, (h, w) mask)] of one own size: what own-size erosion and rule R treat differently, and what a kernel that decodes
    with the canvas width gets wrong."""
    rng = np.random.default_rng([7, w, h])
    Z = lambda: np.zeros((h, w), np.uint8)
    out = [("all ones", np.ones((h, w), np.uint8)), ("empty", Z())]
    m = Z()
    m[max(h - 3, 0):h, max(w - 3, 0):w] = 1                     # 3x3 block (clipped) whose centre is the pixel (w-2, h-2)
    out.append(("3x3 block around (w-2, h-2)", m))
    if h >= 2:                                                  # one 1-run from (w-2, y) into (1, y+1) of the OWN image
        y = (h - 2) // 2
        m = Z()
        m.reshape(-1)[max(y * w + w - 2, 0):min((y + 1) * w + 1, w * h - 1) + 1] = 1
        out.append(("run that wraps across an own row end", m))
    m = (rng.random((h, w)) < 0.93).astype(np.uint8)            # blobs: mostly set, so that the erosion leaves pixels
    m[h - 1, w - 1] = 1
    out.append(("blobs", m))
    m = Z()
    m[h // 4:h, w // 3:w] = rng.random((h - h // 4, w - w // 3)) < 0.97
    out.append(("blob into the last own row and column", m))
    return out


@functools.lru_cache(None)
def kernel_cases():
    """[(name, W, H, [(w, h)], [run list])]: every list covers its own w x h."""
    out = []
    W, H = SMALL_CANVAS
    every_size, every_list = [], []
    for w, h in SMALL_SIZES:
        lm = family(w, h)
        lists = [rle.dense_to_counts(m) for _, m in lm]
        out.append((f"canvas {W}x{H}, own {w}x{h}: " + " | ".join(l for l, _ in lm), W, H, [(w, h)] * len(lists), lists))
        every_size += [(w, h)] * len(lists)
        every_list += lists
    # all of them in one batch, canvas-sized masks between them: neighbouring slots
    mixed_s, mixed_l = [], []
    full = [rle.dense_to_counts(m) for _, m in family(W, H)]
    for k, (s, c) in enumerate(zip(every_size, every_list)):
        mixed_s.append(s); mixed_l.append(c)
        if k % 5 == 4:
            mixed_s.append((W, H)); mixed_l.append(full[(k // 5) % len(full)])
    out.append((f"canvas {W}x{H}: every size and family in one batch, canvas-sized masks between them", W, H, mixed_s, mixed_l))
    # 3373 runs: past the 2048 the workgroup form keeps in registers, past one 512-run wave chunk, many 128-run bands
    w, h = 95, 71
    alt = (((np.arange(h)[:, None] * w + np.arange(w)[None, :]) >> 1) & 1).astype(np.uint8)     # pixel pairs, alternating along the run order
    c = rle.dense_to_counts(alt)
    assert c.size == 3373, c.size
    out.append(("canvas 96x72, own 95x71 alternating pixel pairs (3373 runs) next to a solid block", 96, 72, [(95, 71), (95, 71), (96, 72)],
                [c, rle.dense_to_counts(np.pad(np.ones((60, 80), np.uint8), ((5, 6), (7, 8)))), rle.dense_to_counts(np.ones((72, 96), np.uint8))]))
    # the widest supported row (tile floor included)
    rng = np.random.default_rng(11)
    a = (rng.random((3, 4095)) < 0.98).astype(np.uint8); a[:, -40:] = 1
    b = (rng.random((2, 4065)) < 0.98).astype(np.uint8); b[:, -40:] = 1
    out.append(("canvas 4096x3, own 4095x3 and 4065x2", 4096, 3, [(4095, 3), (4065, 2), (4095, 3), (4096, 3)],
                [rle.dense_to_counts(a), rle.dense_to_counts(b), rle.dense_to_counts(np.ones((3, 4095), np.uint8)),
                 rle.dense_to_counts(np.ones((3, 4096), np.uint8))]))
    return out


# ----------------------------------------------------------------------------- engine-level frames
TINY_W, TINY_H = 256, 144
SIDE = (256, 100)            # cameras 3 and 4 ("SIDE_LEFT", "SIDE_RIGHT"): full width, fewer rows, like Waymo's 1920x886 beside 1920x1280
ODD = (200, 144)             # one further mask, narrower than the canvas


def mixed_tiny_frames(n_frames=4, first=0, waymo=False, all_ones=True, side=SIDE):
    """Five-camera `tiny` frames with the masks of cameras 3 and 4 cropped to `side`, the first mask of another camera cropped to
    ODD, and (all_ones) one all-ones mask more on each cropped camera -- own-size erosion keeps their last row, rule R must not, and
    points do project there (the tests assert it)."""
    from cm3d_amd import synthetic as syn
    cfg = syn.config("tiny", n_cams=5)
    out = []
    for i in range(first, first + n_frames):
        fr = syn.make_waymo_frame(cfg, i) if waymo else syn.make_frame(cfg, i)
        other = [k for k, c in enumerate(fr.cam_nums) if int(c) not in (3, 4)]
        out.append(crop_frame(fr, {3: side, 4: side}, {other[0]: ODD} if other else None, (3, 4) if all_ones else ()))
    return out


def write_waymo_scene(tmp_path, scene, frames):
    """Extracted-frame files and mask files of a scene, from Waymo-shaped frame objects (cams: the frames' own records are rebuilt
    from raw calibrations by the loader, so the raw ones are written: synthetic.make_waymo_frame's, recovered as
    tests/test_gpu_entrypoint.py does)."""
    import json
    import os
    import pickle
    from cm3d_amd import geometry as geo, synthetic as syn
    cfg = syn.config("tiny", n_cams=5)
    fdir, mdir = tmp_path / "frames" / scene, tmp_path / "masks" / scene
    os.makedirs(fdir); os.makedirs(mdir)
    S = np.array([[0, -1, 0, 0], [0, 0, -1, 0], [1, 0, 0, 0], [0, 0, 0, 1]], np.float64)
    centre = None
    for i, fr in enumerate(frames):
        P = np.asarray(fr.pose).reshape(4, 4)
        centre = P[:2, 3] if centre is None else centre
        base = syn.make_frame(cfg, int(fr.token.rsplit("-", 1)[1]))
        ext, intr = [], []
        for c in range(base.cams.shape[0]):
            t_cs_neg, R_csT, _ = geo.cam_stage(base.cams[c], 1)
            T = np.eye(4); T[:3, :3] = R_csT.T; T[:3, 3] = -t_cs_neg
            K = geo.cam_K(base.cams[c]) / cfg.ratio
            ext.append((T @ S).reshape(16)); intr.append([K[0, 0], K[1, 1], K[0, 2], K[1, 2], 0, 0, 0, 0, 0])
        rec = dict(points=fr.sweeps_raw[0][:, :3], extrinsics=np.array(ext), intrinsics=np.array(intr), pose=P.reshape(16),
                   timestamp_micros=np.int64(fr.timestamp_micros), context_name=np.str_(fr.context_name))
        if i == 0:
            polys = [np.cumsum(np.concatenate([[[centre[0] - 200 + 40 * k, centre[1] - 200, 0.0]], np.tile([[0.0, 0.5, 0.0]], (800, 1))]), 0) for k in range(10)]
            rec["lanes"] = np.vstack(polys); rec["lane_off"] = np.concatenate([[0], np.cumsum([len(p) for p in polys])])
        np.savez_compressed(fdir / f"{i}_frame.npz", **rec)
        pickle.dump(fr.rles, open(mdir / f"{i}_masks.pkl", "wb"))
        json.dump({"labels": fr.labels, "detection_scores": fr.scores, "cam_nums": fr.cam_nums}, open(mdir / f"{i}_data.json", "w"))
    return frames
