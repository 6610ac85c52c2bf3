"""The mask kernels (csrc/masks.hip) at image edges, word seams, run-count boundaries, zero-length runs and pixel indices above
2^24, bit for bit against the plain reference of tests/mask_cases.py -- including what they must NOT write: `packed` is
pre-filled, and every word outside a mask's stored rectangle (and one guard slot behind the last mask) has to keep the fill."""
import os
import subprocess
import sys

import numpy as np
import pytest

from cm3d_amd import rle
from tests import mask_cases as C

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FAMILIES = {"F1": C.f1_cases, "F2": C.f2_cases, "F3": C.f3_cases, "F4": C.f4_cases, "F5": C.f5_cases}


def _wave_form(n_masks, total_runs):
    """The form cm3d_rle_erode_pack takes: the forced one, or a wave per mask up to an average of 1024 runs per mask."""
    forced = os.environ.get("CM3D_RLE_FORM")
    return forced[0] == "w" if forced else total_runs <= 1024 * n_masks


def _fail(what, W, H, name, got, exp, stride):
    """First differing word of two (n, words) arrays -> an assertion message that names the mask, (y, word) and both words."""
    got, exp = got.reshape(got.shape[0], -1), exp.reshape(exp.shape[0], -1)
    i, q = (int(v[0]) for v in np.nonzero(got != exp))
    msg = (f"{what}: W={W} H={H} mask {i}, first difference at (y, word) = ({q // stride}, {q % stride}) [slot word {q}]: "
           f"expected {int(exp[i, q]):#010x}, got {int(got[i, q]):#010x}; {int((got != exp).sum())} words differ; case {name}")
    print(msg)
    return msg


def _check_words(what, W, H, name, got, exp, stride):
    if not np.array_equal(got, exp):
        raise AssertionError(_fail(what, W, H, name, got, exp, stride))


def _check_bbox(what, W, H, name, got, exp):
    if not np.array_equal(got, exp):
        i = int(np.nonzero((got != exp).any(axis=1))[0][0])
        msg = f"{what}: W={W} H={H} mask {i}: expected bbox {exp[i].tolist()}, got {got[i].tolist()}; case {name}"
        print(msg)
        raise AssertionError(msg)


def _reference(W, H, items, cache):
    """Per item: (mask, run list, eroded mask).  Items are keyed on their identity: a list that several cases share is expanded
    and eroded once."""
    items = list(items)
    new = [it for it in {id(it): it for it in items}.values() if id(it) not in cache]
    if new:
        masks, counts = [], []
        for it in new:
            a = np.asarray(it)
            masks.append(a.astype(np.uint8) if a.ndim == 2 else rle.counts_to_dense(a, W, H))
            counts.append(rle.dense_to_counts(a) if a.ndim == 2 else a.astype(np.uint32))
        masks = np.stack(masks)
        exp = C.erode_ref(masks)
        for k, it in enumerate(new):
            cache[id(it)] = (it, masks[k], counts[k], exp[k])
    ref = [cache[id(it)] for it in items]
    return np.stack([r[1] for r in ref]), [r[2] for r in ref], np.stack([r[3] for r in ref])


def run_case(case, cache):
    """decode, erode and erode_rle of one case against the reference, per mask and bit for bit."""
    from cm3d_amd import ops
    W, H, items, name = case
    Wp = (W + 31) // 32
    masks, counts, exp = _reference(W, H, items, cache)
    n = len(counts)
    exp_words, exp_bounds = C.pack_words(exp), C.bounds(exp)
    whole = np.tile(np.array([0, 0, Wp, H], np.int32), (n, 1))

    dense = ops.decode([{"size": [W, H], "counts": c} for c in counts], as_counts=True).cpu().numpy()
    if not np.array_equal(dense, masks):
        i, y, x = (int(v[0]) for v in np.nonzero(dense != masks))
        raise AssertionError(f"decode: W={W} H={H} mask {i} pixel (x, y) = ({x}, {y}): expected {masks[i, y, x]}, got {dense[i, y, x]}; case {name}")

    packed, bbox = ops.erode(masks * np.uint8(153))
    _check_words("erode", W, H, name, packed.cpu().numpy().view(np.uint32), exp_words, Wp)
    _check_bbox("erode", W, H, name, bbox.cpu().numpy(), np.concatenate([exp_bounds, whole], axis=1))

    wave = _wave_form(n, sum(c.size for c in counts))
    rects = C.word_rects(masks)
    packed, bbox = ops.erode_rle(counts, W, H, fill=C.FILL, guard_slots=1)
    got = packed.cpu().numpy().view(np.uint32).reshape(n + 1, H * Wp)
    want = np.full((n + 1, H * Wp), C.FILL, np.uint32)          # an empty mask's slot and the guard slot stay as they were
    for i, (xw0, y0, wc, rows) in enumerate(rects.tolist()):
        if wc:
            crop = exp_words[i, y0:y0 + rows, xw0:xw0 + wc]
            if wave:        # the rectangle's rows one behind the other from the start of the slot
                want[i, :rows * wc] = crop.reshape(-1)
            else:           # the rectangle where it lies in the image
                want[i].reshape(H, Wp)[y0:y0 + rows, xw0:xw0 + wc] = crop
    form = "erode_rle (wave form)" if wave else "erode_rle (workgroup form)"
    _check_bbox(form, W, H, name, bbox.cpu().numpy(),
                np.concatenate([exp_bounds, rects if wave else np.where(rects[:, 2:3] > 0, whole, 0)], axis=1))
    if not np.array_equal(got, want):
        i = int(np.nonzero((got != want).any(axis=1))[0][0])
        stride = int(rects[i, 2]) if wave and i < n and rects[i, 2] else Wp
        raise AssertionError(_fail(form, W, H, name, got, want, stride))


def run_f5(case):
    """erode_rle alone, on an image whose dense form is never built: the stored rectangles against the erosion of their crops."""
    from cm3d_amd import ops
    W, H, items, name = case
    Wp = (W + 31) // 32
    counts = [c for c, _ in items]
    n = len(counts)
    wave = _wave_form(n, sum(c.size for c in counts))
    packed, bbox = ops.erode_rle(counts, W, H, fill=C.FILL, guard_slots=1)
    got = packed.cpu().numpy().view(np.uint32).reshape(n + 1, H * Wp)
    bbox = bbox.cpu().numpy()
    for i, (_, blocks) in enumerate(items):
        rect, e = C.f5_expected(blocks, W, H)
        xw0, y0, wc, rows = rect
        ys, xs = np.nonzero(e)
        want_bbox = [xw0 * 32 + xs.min(), y0 + ys.min(), xw0 * 32 + xs.max(), y0 + ys.max()] + (list(rect) if wave else [0, 0, Wp, H])
        assert bbox[i].tolist() == want_bbox, f"F5 mask {i}: expected bbox {want_bbox}, got {bbox[i].tolist()}; case {name}"
        slot = got[i].copy()
        if wave:
            words = slot[:rows * wc].copy()
            slot[:rows * wc] = C.FILL
        else:
            region = slot.reshape(H, Wp)[y0:y0 + rows, xw0:xw0 + wc]
            words = region.reshape(-1).copy()
            region[...] = C.FILL
        px = C.unpack_rect(words, rect, W)
        if not np.array_equal(px, e) or not np.array_equal(words.reshape(rows, wc), C.pack_words(e)):
            raise AssertionError(_fail(f"erode_rle F5 mask {i} rect {rect}", W, H, name, words[None], C.pack_words(e).reshape(1, -1), wc))
        stray = np.flatnonzero(slot != C.FILL)
        assert stray.size == 0, (f"F5 mask {i}: {stray.size} words written outside the stored rectangle {rect}, first at slot word "
                                 f"{int(stray[0])}: {int(slot[stray[0]]):#010x}; case {name}")
    assert (got[n] == C.FILL).all(), f"F5: the guard slot behind the last mask was written; case {name}"


def run_families(names):
    cache = {}
    for f in names:
        for case in FAMILIES[f]():
            if f == "F5":
                run_f5(case)
            else:
                run_case(case, cache)
        cache.clear()


def test_mask_kernels_in_the_form_the_product_picks(monkeypatch):
    """F1..F5 with nothing forced: a wave per mask for every batch but the one whose lists average one run more than 1024."""
    for v in ("CM3D_RLE_FORM", "CM3D_RLE_BANDS", "CM3D_RLEW_LDS_WORDS"):
        monkeypatch.delenv(v, raising=False)
    cases = C.f3_cases()
    assert _wave_form(len(cases[4][2]), sum(c.size for c in cases[4][2])) and not _wave_form(len(cases[5][2]), sum(c.size for c in cases[5][2]))
    run_families(["F1", "F2", "F3", "F4", "F5"])


_CHILD = """
import sys
sys.path.insert(0, {root!r})
from tests import test_gpu_mask_edges as T
T.run_families({families!r})
print("EDGES OK")
"""

_SETTINGS = [
    ({"CM3D_RLE_FORM": "wave"}, True),
    ({"CM3D_RLE_FORM": "block"}, True),
    ({"CM3D_RLE_FORM": "wave", "CM3D_RLE_BANDS": "2"}, False),
    ({"CM3D_RLE_FORM": "wave", "CM3D_RLE_BANDS": "4"}, False),
    ({"CM3D_RLE_FORM": "wave", "CM3D_RLEW_LDS_WORDS": "512"}, False),
    ({"CM3D_RLE_FORM": "wave", "CM3D_RLEW_LDS_WORDS": "390"}, False),      # the floor: one output row per tile at W = 4096
]


@pytest.mark.parametrize("env,with_f5", _SETTINGS, ids=["wave", "block", "wave-bands2", "wave-bands4", "wave-lds512", "wave-lds390"])
def test_mask_kernels_in_every_forced_form(env, with_f5):
    """The same runner with each form of cm3d_rle_erode_pack forced (the settings are read once per process, hence the child):
    a wave per mask, a workgroup per mask, rows in 2 and 4 bands, and LDS slices that cut a mask into many tiles."""
    families = ["F1", "F2", "F3", "F4"] + (["F5"] if with_f5 else [])
    base = {k: v for k, v in os.environ.items() if k not in ("CM3D_RLE_FORM", "CM3D_RLE_BANDS", "CM3D_RLEW_LDS_WORDS")}
    r = subprocess.run([sys.executable, "-c", _CHILD.format(root=ROOT, families=families)], env=dict(base, **env), capture_output=True,
                       text=True, timeout=300, cwd=ROOT)
    # (a child that a signal or a HIP fault ended fails here like any other; nothing is started after it)
    assert r.returncode == 0 and "EDGES OK" in r.stdout, f"exit status {r.returncode}\n{r.stdout[-3000:]}\n{r.stderr[-3000:]}"


@pytest.mark.parametrize("W", [0, 4097])
def test_unsupported_widths_are_refused_before_any_launch(W):
    """W = 0 and W = 4097 (one past the widest row the kernels hold): CM3D_ERR_ARG from all three entry points, the outputs
    untouched, and Cm3dError from ops."""
    import torch
    from cm3d_amd import _lib, ops
    L = _lib.lib()
    H, ERR_ARG = 3, -1
    dev = torch.device("cuda", torch.cuda.current_device())
    st = torch.cuda.current_stream().cuda_stream
    cnts = torch.tensor([max(W * H, 1)], dtype=torch.int32, device=dev)
    off = torch.tensor([0, 1], dtype=torch.int32, device=dev)
    words = 4200
    dense = torch.full((words * 4,), 0x5A, dtype=torch.uint8, device=dev)
    packed = torch.full((words,), 0x5A5A5A5A, dtype=torch.int32, device=dev)
    bbox = torch.full((_lib.BBOX_STRIDE,), 0x5A5A5A5A, dtype=torch.int32, device=dev)
    ws = torch.zeros(max(int(L.cm3d_rle_workspace_bytes(1)), 16), dtype=torch.uint8, device=dev)
    assert L.cm3d_rle_to_dense(cnts.data_ptr(), off.data_ptr(), 1, 1, W, H, dense.data_ptr(), ws.data_ptr(), ws.numel(), st) == ERR_ARG
    assert L.cm3d_erode_pack(dense.data_ptr(), 1, W, H, packed.data_ptr(), bbox.data_ptr(), st) == ERR_ARG
    assert L.cm3d_rle_erode_pack(cnts.data_ptr(), off.data_ptr(), 1, 1, W, H, packed.data_ptr(), bbox.data_ptr(), ws.data_ptr(),
                                 ws.numel(), st) == ERR_ARG
    torch.cuda.synchronize()
    assert bool((dense == 0x5A).all()) and bool((packed == 0x5A5A5A5A).all()) and bool((bbox == 0x5A5A5A5A).all())
    # the supported widths next to them pass the same calls
    for Wok in (1, 4096):
        c = torch.tensor([Wok * H], dtype=torch.int32, device=dev)
        assert L.cm3d_rle_to_dense(c.data_ptr(), off.data_ptr(), 1, 1, Wok, H, dense.data_ptr(), ws.data_ptr(), ws.numel(), st) == 0
        assert L.cm3d_erode_pack(dense.data_ptr(), 1, Wok, H, packed.data_ptr(), bbox.data_ptr(), st) == 0
        assert L.cm3d_rle_erode_pack(c.data_ptr(), off.data_ptr(), 1, 1, Wok, H, packed.data_ptr(), bbox.data_ptr(), ws.data_ptr(),
                                     ws.numel(), st) == 0
    torch.cuda.synchronize()
    counts = [np.array([max(W * H, 1)], np.uint32)]
    with pytest.raises(_lib.Cm3dError):
        ops.decode([{"size": [W, H], "counts": counts[0]}], as_counts=True)
    with pytest.raises(_lib.Cm3dError):
        ops.erode(np.zeros((1, H, W), np.uint8))
    with pytest.raises(_lib.Cm3dError):
        ops.erode_rle(counts, W, H)
