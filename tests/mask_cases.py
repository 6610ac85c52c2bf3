"""Case table of the mask kernels (csrc/masks.hip) and a plain reference of what they compute: numpy only, no GPU, no torch.

The families aim at the places where the kernels change path -- image edges, the seams between 32-bit words, the run counts
at which a list is cut into chunks or bands, pixel indices a float32 no longer holds exactly, zero-length runs -- and every
expected value is exact.  tests/test_mask_cases_host.py keeps the table honest on the CPU (each family reaches the branch it
is built for); tests/test_gpu_mask_edges.py runs it on the device.

A case is (W, H, items, name); an item is a mask ((H, W) array, non-zero = set) or a COCO run list (1-D uint32, alternating
0-run, 1-run, ... over the row-major image).  The same array OBJECT may appear in several cases (F3 lays one batch out four
times): a runner can key what it derives from an item on id(item)."""
import functools

import numpy as np

from cm3d_amd import rle

INT_MAX = 0x7FFFFFFF
FILL = 0xA5A5A5A5              # what the GPU tests put into `packed` before a call


# ----------------------------------------------------------------------------- the reference
def erode_ref(mask_hw):
    """3x3 erosion of a mask (or a stack (..., H, W) of masks); neighbours outside the image count as set: the AND of the nine
    shifted views of the mask padded with ones."""
    m = np.asarray(mask_hw) != 0
    H, W = m.shape[-2:]
    p = np.pad(m, [(0, 0)] * (m.ndim - 2) + [(1, 1), (1, 1)], constant_values=True)
    out = np.ones_like(m)
    for dy in range(3):
        for dx in range(3):
            out &= p[..., dy:dy + H, dx:dx + W]
    return out.astype(np.uint8)


def bounds(stack):
    """(n, H, W) -> (n, 4) int32 x0, y0, x1, y1 (inclusive) of the set pixels; INT_MAX, INT_MAX, -1, -1 for an empty mask."""
    s = np.asarray(stack) != 0
    n, H, W = s.shape
    cols, rows = s.any(axis=1), s.any(axis=2)
    some = cols.any(axis=1)
    b = np.empty((n, 4), np.int32)
    b[:, 0] = np.argmax(cols, axis=1)
    b[:, 1] = np.argmax(rows, axis=1)
    b[:, 2] = W - 1 - np.argmax(cols[:, ::-1], axis=1)
    b[:, 3] = H - 1 - np.argmax(rows[:, ::-1], axis=1)
    b[~some] = [INT_MAX, INT_MAX, -1, -1]
    return b


def word_rects(stack):
    """(n, H, W) -> (n, 4) int32 xw0, y0, wc, rows: the rectangle of whole 32-bit words that holds each mask's set pixels
    (include/cm3d_hip.h, `packed`); zeros for an empty mask."""
    b = bounds(stack).astype(np.int64)
    r = np.stack([b[:, 0] >> 5, b[:, 1], (b[:, 2] >> 5) - (b[:, 0] >> 5) + 1, b[:, 3] - b[:, 1] + 1], axis=1)
    r[b[:, 2] < 0] = 0
    return r.astype(np.int32)


def word_rect(mask_hw):
    """(xw0, y0, wc, rows) of one mask's set pixels; all zeros for an empty mask."""
    return tuple(int(v) for v in word_rects(np.asarray(mask_hw)[None])[0])


def pack_words(stack):
    """(..., H, W) pixels -> (..., H, Wp) uint32, bit x & 31 of word x >> 5 = pixel x; the pad bits of a row's last word are 0."""
    s = np.asarray(stack) != 0
    W = s.shape[-1]
    Wp = (W + 31) // 32
    if Wp * 32 != W:
        s = np.pad(s, [(0, 0)] * (s.ndim - 1) + [(0, Wp * 32 - W)])
    return np.ascontiguousarray(np.packbits(s, axis=-1, bitorder="little")).view("<u4").astype(np.uint32, copy=False)


def unpack_rect(slot_words, rect, W):
    """The pixels ((rows, columns) uint8) of one mask's stored rectangle: slot_words are the mask's slot of `packed` (rows * wc
    words from its start are read), rect = (xw0, y0, wc, rows).  Columns run from x = 32 * xw0 to the rectangle's last word or
    the image's right edge, whichever comes first."""
    xw0, _, wc, rows = (int(v) for v in rect)
    w = np.ascontiguousarray(np.asarray(slot_words).reshape(-1)[:rows * wc].astype("<u4"))
    bits = np.unpackbits(w.view(np.uint8).reshape(rows, wc * 4), axis=1, bitorder="little")
    return bits[:, :min(wc * 32, W - xw0 * 32)]


def rw_row_of_emulated(s, W):
    """masks.hip's rw_row_of in numpy: pixel index -> row through a float32 reciprocal and one correction each way."""
    s = np.asarray(s, np.uint32)
    rcp = np.float32(1.0) / np.float32(W)
    y = (s.astype(np.float32) * rcp).astype(np.int32)
    y = y - (y.astype(np.uint32) * np.uint32(W) > s)
    y = y + ((y + 1).astype(np.uint32) * np.uint32(W) <= s)
    return y


# ----------------------------------------------------------------------------- run lists
def split_runs(counts, positions, rng):
    """Insert zero-length runs: every entry of `positions` cuts one run a into a1, 0, a2 (a1 + a2 = a).  An entry is a run index
    i (a1 drawn from 0..a, both ends included) or (i, a1); an index named k times is cut k times, a1, 0, a2, 0, a3, ...  Indices
    refer to `counts` as given.  The result describes the same mask and has the same sum."""
    counts = np.asarray(counts, np.uint32)
    cuts = {}
    for p in positions:
        i, a1 = (p if isinstance(p, tuple) else (p, None))
        cuts.setdefault(int(i) % counts.size, []).append(a1)
    out = []
    for i, a in enumerate(counts.tolist()):
        for a1 in cuts.get(i, ()):
            a1 = int(rng.integers(0, a + 1)) if a1 is None else min(int(a1), a)
            out += [a1, 0]
            a -= a1
        out.append(a)
    out = np.array(out, np.uint32)
    assert int(out.astype(np.int64).sum()) == int(counts.astype(np.int64).sum()) and out.size == counts.size + 2 * len(positions)
    return out


def spans_to_runs(p0, p1, total):
    """Sorted, non-touching pixel intervals [p0, p1) -> run lengths over `total` pixels."""
    p0, p1 = np.asarray(p0, np.int64), np.asarray(p1, np.int64)
    assert (p0 < p1).all() and (p0[1:] > p1[:-1]).all() and (p0.size == 0 or (p0[0] >= 0 and p1[-1] <= total))
    edges = np.empty(2 * p0.size + 1, np.int64)
    edges[0], edges[1::2], edges[2::2] = 0, p0, p1
    c = np.diff(edges)
    if p0.size == 0 or p1[-1] < total:
        c = np.concatenate([c, [total - edges[-1]]])
    return c.astype(np.uint32)


# ----------------------------------------------------------------------------- F1
F1_SIZES = [(3, 3), (4, 3), (3, 4), (5, 2), (2, 5), (6, 2), (1, 8), (8, 1)]


@functools.lru_cache(None)
def f1_cases():
    """Every mask of the tiny sizes but the last (the full one, which F2 has at every size): the mask count of a call is then
    no multiple of 4, and the wave form's last workgroup is only partly used."""
    out = []
    for W, H in F1_SIZES:
        n = (1 << (W * H)) - 1
        bits = (np.arange(n, dtype=np.uint32)[:, None] >> np.arange(W * H, dtype=np.uint32)) & 1
        out.append((W, H, bits.astype(np.uint8).reshape(n, H, W), f"F1 all masks {W}x{H}"))
    return out


# ----------------------------------------------------------------------------- F2
F2_WIDTHS = [1, 2, 31, 32, 33, 63, 64, 65, 95, 96, 97, 2016, 2047, 2048, 2049, 2080, 4064, 4095, 4096]
F2_HEIGHTS = [1, 2, 3, 5, 67]
F2_BAR_X = list(range(29, 35)) + list(range(61, 67))


def f2_masks(W, H):
    """[(label, mask)] of one size."""
    rng = np.random.default_rng([2, W, H])
    Z = lambda: np.zeros((H, W), np.uint8)
    out = [("full", np.ones((H, W), np.uint8)), ("empty", Z())]
    for cy in (0, H - 1):
        for cx in (0, W - 1):
            m = Z(); m[cy, cx] = 1
            out.append((f"pixel at ({cx},{cy})", m))
    for cy in (0, H // 2, H - 1):           # 3x3 blocks (clipped to the image) at the corners and the edges' middles
        for cx in (0, W // 2, W - 1):
            if (cx, cy) == (W // 2, H // 2):
                continue
            x0 = min(max(cx - 1, 0), max(W - 3, 0)); y0 = min(max(cy - 1, 0), max(H - 3, 0))
            m = Z(); m[y0:y0 + 3, x0:x0 + 3] = 1
            out.append((f"3x3 block at ({x0},{y0})", m))
    m = np.ones((H, W), np.uint8); m[H // 2, W // 2] = 0
    out.append(("hole", m))
    out.append(("checkerboard", ((np.arange(H)[:, None] + np.arange(W)[None, :]) & 1).astype(np.uint8)))
    for bw in (1, 2, 3, 4):
        for x in F2_BAR_X:
            if x + bw <= W:
                m = Z(); m[:, x:x + bw] = 1
                out.append((f"vertical bar x={x} width {bw}", m))
    y0 = min(max(H // 2 - 1, 0), max(H - 3, 0))
    m = Z(); m[y0:y0 + 3, :] = 1
    out.append(("horizontal bar", m))
    if H >= 2:                              # one 1-run from (W-2, y) into (1, y+1)
        y = (H - 2) // 2
        m = Z()
        m.reshape(-1)[max(y * W + W - 2, 0):min((y + 1) * W + 1, W * H - 1) + 1] = 1
        out.append(("run that wraps into the next row", m))
    for d in (0.5, 0.9, 0.99):
        out.append((f"noise {d}", (rng.random((H, W)) < d).astype(np.uint8)))
    Wp = (W + 31) // 32
    if Wp > 64:                             # 64 or more word columns, not the whole width: from word 0, and ending in the last word
        for label, xa, xb in (("from word 0", 3, 63 * 32 + 5), ("to the last word", (Wp - min(Wp - 1, 67)) * 32 + 7, W)):
            m = Z()
            m[:, xa:xb] = rng.random((H, xb - xa)) < 0.97
            m[0, xa] = 1; m[H - 1, xb - 1] = 1
            out.append((f"wide blob {label}", m))
    return out


@functools.lru_cache(None)
def f2_cases():
    out = []
    for W in F2_WIDTHS:
        for H in F2_HEIGHTS:
            lm = f2_masks(W, H)
            out.append((W, H, [m for _, m in lm], f"F2 {W}x{H}: " + " | ".join(f"{i} {l}" for i, (l, _) in enumerate(lm))))
    return out


# ----------------------------------------------------------------------------- F3
F3_W, F3_H = 1600, 900
F3_RUNS = [1, 2, 3, 127, 128, 129, 511, 512, 513, 1023, 1024, 1025, 2047, 2048, 2049, 4097]


def f3_list(n, seed=0):
    """A run list of exactly n runs on the F3 image, made of dashes one pixel high (a dash is one 1-run): dash j lies in row
    r0 + j % rows of column block j // rows (blocks are 100 px apart, a dash starts in the first 20 px of its block and is
    3..60 px long), so dashes of consecutive rows overlap and the erosion leaves pixels.  An even n needs the last pixel of the
    image set: the dashes then end in the last row and the last of them runs to the last column."""
    W, H = F3_W, F3_H
    rng = np.random.default_rng([3, n, seed])
    k = n // 2
    if k == 0:
        return np.array([W * H], np.uint32)
    rows = min(k, H)
    assert (k + rows - 1) // rows * 100 <= W
    r0 = H - rows if n % 2 == 0 else int(rng.integers(0, H - rows + 1))
    j = np.arange(k)
    y, x0 = r0 + j % rows, (j // rows) * 100 + rng.integers(0, 20, k)
    x1 = x0 + rng.integers(3, 61, k)                    # exclusive
    order = np.lexsort((x0, y))
    p0, p1 = (y * W + x0)[order], (y * W + x1)[order]
    if n % 2 == 0:
        p1[-1] = W * H
    c = spans_to_runs(p0, p1, W * H)
    assert c.size == n, (n, c.size)
    return c


@functools.lru_cache(None)
def f3_cases():
    """The 16 lists in one batch, laid out four times behind 0..3 one-run empty masks (each list then starts at each of the four
    word alignments), and two batches at an average of exactly 1024 runs per mask and one run more."""
    W, H = F3_W, F3_H
    lists = {n: f3_list(n) for n in F3_RUNS}
    empty = np.array([W * H], np.uint32)
    out = [(W, H, [empty] * k + [lists[n] for n in F3_RUNS], f"F3 runs {F3_RUNS} behind {k} one-run masks") for k in range(4)]
    out.append((W, H, [lists[1023], lists[1024], lists[1025], lists[1024]], "F3 total_runs == 1024 * n_masks"))
    out.append((W, H, [lists[1023], lists[1024], lists[1025], f3_list(1025, seed=1)], "F3 total_runs == 1024 * n_masks + 1"))
    return out


def f3_alignments(case):
    """Start offset modulo 4 of every list of an F3 case within its batch."""
    sizes = [np.asarray(c).size for c in case[2]]
    return [int(o) % 4 for o in np.concatenate([[0], np.cumsum(sizes)[:-1]])]


# ----------------------------------------------------------------------------- F4
F4_F2_SIZES = [(1, 5), (33, 5), (65, 3), (97, 67), (2049, 3)]
F4_F2_LABELS = ["hole", "checkerboard", "noise 0.9", "run that wraps into the next row", "pixel at (0,0)", "3x3 block at (0,0)"]
F4_F3_RUNS = [3, 127, 511, 1023, 2047]


F4_INSERTIONS = 9


def f4_positions(counts, rng):
    """Run 0 with nothing in front (a leading 0, 0) and once more anywhere, the last run, one run cut twice in a row, two random
    runs, and two 1-runs cut one pixel from their start and from their end (a one-pixel 1-run that abuts the rest of its
    stretch: leaving it out changes the erosion, which a one-pixel run between clear pixels never does)."""
    counts = np.asarray(counts)
    n = counts.size
    mid = int(rng.integers(0, n))
    ones = np.arange(1, n, 2)
    ones = ones[counts[ones] >= 3] if (counts[ones] >= 3).any() else ones
    j1, j2 = (int(v) for v in rng.choice(ones, 2))
    return [(0, 0), 0, n - 1, mid, mid, int(rng.integers(0, n)), int(rng.integers(0, n)), (j1, 1), (j2, int(counts[j2]) - 1)]


@functools.lru_cache(None)
def f4_cases():
    """Zero-length runs inserted into lists of F2 and F3 (9 insertions = 18 more runs each, so the 511-run list crosses 512 and
    the 2047-run list 2048).  An item still describes its source's mask, which is checked here against the source itself."""
    rng = np.random.default_rng(4)
    out = []
    for W, H in F4_F2_SIZES:
        src = [m for l, m in f2_masks(W, H) if l in F4_F2_LABELS]
        items = []
        for m in src:
            c = rle.dense_to_counts(m)
            s = split_runs(c, f4_positions(c, rng), rng)
            assert np.array_equal(rle.counts_to_dense(s, W, H), m)
            items.append(s)
        out.append((W, H, items, f"F4 zero-length runs in F2 lists {W}x{H}: {F4_F2_LABELS}"))
    W, H = F3_W, F3_H
    items = []
    for n in F4_F3_RUNS:
        c = f3_list(n)
        s = split_runs(c, f4_positions(c, rng), rng)
        assert np.array_equal(rle.counts_to_dense(s, W, H), rle.counts_to_dense(c, W, H))
        items.append(s)
    out.append((W, H, items, f"F4 zero-length runs in F3 lists of {F4_F3_RUNS} runs"))
    return out


# ----------------------------------------------------------------------------- F5
F5_W, F5_H = 4095, 32767
# per mask: blocks (x0, y0, x1, y1), inclusive, sorted by row, no two in one row
F5_MASKS = [
    ("40x9 block ending in the last row and column", [(4055, 32758, 4094, 32766)]),
    ("40x9 block in the first rows", [(100, 0, 139, 8)]),
    ("block in the middle, left edge at x = 4064", [(4064, 16380, 4094, 16388)]),
    ("two 5x5 blocks at rows 3 and 32760 in the same two word columns", [(62, 3, 66, 7), (60, 32760, 64, 32764)]),
    ("full-width bar of 3 rows at row 20000", [(0, 20000, 4094, 20002)]),
]


@functools.lru_cache(None)
def f5_cases():
    """Masks whose pixel indices pass 2^24 (float32 stops holding integers exactly) on an image near the C ABI's size limit.
    Items are (run list, blocks): the image itself (134 M pixels) is never built."""
    W, H = F5_W, F5_H
    items = []
    for _, blocks in F5_MASKS:
        rows = np.concatenate([np.arange(y0, y1 + 1) for _, y0, _, y1 in blocks])
        x0 = np.concatenate([np.full(y1 - y0 + 1, xa) for xa, y0, _, y1 in blocks])
        x1 = np.concatenate([np.full(y1 - y0 + 1, xb) for _, y0, xb, y1 in blocks])
        items.append((rle.spans_to_counts(rows, x0, x1, W, H), blocks))
    return [(W, H, items, "F5 4095x32767: " + " | ".join(f"{i} {l}" for i, (l, _) in enumerate(F5_MASKS)))]


def f5_rect(blocks):
    xa, ya = min(b[0] for b in blocks), min(b[1] for b in blocks)
    xb, yb = max(b[2] for b in blocks), max(b[3] for b in blocks)
    return (xa >> 5, ya, (xb >> 5) - (xa >> 5) + 1, yb - ya + 1)


def f5_expected(blocks, W, H):
    """(rect, eroded pixels of the rect as unpack_rect returns them): the erosion of the rectangle's crop with a one-pixel margin;
    margin pixels outside the image are ones (the border rule), those inside are what the image holds there."""
    rect = f5_rect(blocks)
    xw0, y0, wc, rows = rect
    cx0, cx1 = xw0 * 32 - 1, min((xw0 + wc) * 32, W)            # columns cx0 .. cx1, rows y0 - 1 .. y0 + rows
    ys, xs = np.arange(y0 - 1, y0 + rows + 1), np.arange(cx0, cx1 + 1)
    crop = ((ys < 0) | (ys >= H))[:, None] | ((xs < 0) | (xs >= W))[None, :]
    crop = crop.astype(np.uint8)
    for xa, ya, xb, yb in blocks:
        crop[ya - (y0 - 1):yb - (y0 - 1) + 1, xa - cx0:xb - cx0 + 1] = 1
    return rect, erode_ref(crop)[1:-1, 1:-1]
