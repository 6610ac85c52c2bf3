"""Cases of the virtual-point stage (include/cm3d_hip.h: cm3d_hit_project, cm3d_virtual_points), shared by
tests/test_virtual_points_host.py and tests/test_gpu_virtual_points.py.  Host only: nothing here touches the device.

A case is one call: masks already eroded and bit-packed on the host in one of the three stored forms (the whole image, the rectangle
of the set pixels' words, the rectangle written at the image's row stride with the words around it left as they were), cameras of one
to three stages, and lists whose (u, v, depth) rows are given directly -- the rule's steps 2 to 5 take them as an input."""
import numpy as np

from cm3d_amd._lib import BBOX_STRIDE, CAM_STRIDE

GARBAGE = np.uint32(0xDEADBEEF)       # what the words a mask kernel never wrote hold


def rot(axis, deg):
    a = np.deg2rad(deg)
    c, s = np.cos(a), np.sin(a)
    R = {"x": [[1, 0, 0], [0, c, -s], [0, s, c]], "y": [[c, 0, s], [0, 1, 0], [-s, 0, c]], "z": [[c, -s, 0], [s, c, 0], [0, 0, 1]]}[axis]
    R = np.array(R, np.float64)
    return np.round(R) if deg % 90 == 0 else R                   # a quarter turn is a signed permutation: exactly orthonormal in float32


def camera(stages=2, offset=0.0, skew=0.0, fx=620.0, fy=610.0, cx=101.5, cy=58.25, exact=False):
    """A float32 camera record of `stages` rigid stages whose first stage carries the world offset (metres along x and y): t_pre on the
    first stage, t_post on every stage but the first of three (so that both flags occur with and without).  exact: every stage is a
    quarter turn, so that the float32 record's R^T is R's inverse exactly (the cosines of any other angle are rounded)."""
    r = np.zeros(CAM_STRIDE, np.float32)
    spec = {1: [("z", 12.0, (-offset, -offset * 0.5, 1.0), (0.2, -0.1, 0.3))],
            2: [("z", -33.0, (-offset, -offset * 0.5, -0.7), None), ("x", -88.0, (0.4, 0.1, -0.2), (0.05, 0.02, -0.03))],
            3: [("z", 20.0, (-offset, -offset * 0.5, 0.3), None), ("y", 7.0, None, (0.3, -0.2, 0.1)), ("x", -91.0, (0.1, 0.2, 0.3), (0.01, -0.02, 0.03))]}[stages]
    flags = 0
    for s, (axis, deg, t_pre, t_post) in enumerate(spec):
        deg = (90.0, -90.0, 90.0)[s] if exact else deg
        if t_pre is not None:
            r[15 * s:15 * s + 3] = t_pre
            flags |= 1 << (2 * s)
        r[15 * s + 3:15 * s + 12] = rot(axis, deg).reshape(9)
        if t_post is not None:
            r[15 * s + 12:15 * s + 15] = t_post
            flags |= 2 << (2 * s)
    r[45:54] = [fx, skew, cx, 0, fy, cy, 0, 0, 1]
    r[54], r[55] = stages, flags
    return r


def forward64(cam, p):
    """The camera's chain in float64 for one point: (u, v, depth)."""
    cam = np.asarray(cam, np.float32).astype(np.float64)
    p = np.asarray(p, np.float64).copy()
    ns, fl = int(cam[54]), int(cam[55])
    for s in range(ns):
        st = cam[15 * s:15 * s + 15]
        if fl & (1 << (2 * s)):
            p = p + st[0:3]
        p = st[3:12].reshape(3, 3) @ p
        if fl & (2 << (2 * s)):
            p = p + st[12:15]
    h = cam[45:54].reshape(3, 3) @ p
    return h[0] / h[2], h[1] / h[2], p[2]


def world_points(cam, uvd):
    """float32 world rows (n, 4) that the camera sees at about the given (u, v, depth) rows: the chain inverted in float64."""
    cam64 = np.asarray(cam, np.float32).astype(np.float64)
    K = cam64[45:54].reshape(3, 3)
    ns, fl = int(cam64[54]), int(cam64[55])
    out = np.zeros((len(uvd), 4), np.float32)
    for i, (u, v, d) in enumerate(np.asarray(uvd, np.float64)):
        p = np.linalg.solve(K, np.array([u * d, v * d, d]))
        for s in range(ns - 1, -1, -1):
            st = cam64[15 * s:15 * s + 15]
            if fl & (2 << (2 * s)):
                p = p - st[12:15]
            p = np.linalg.solve(st[3:12].reshape(3, 3), p)
            if fl & (1 << (2 * s)):
                p = p - st[0:3]
        out[i, :3] = p
    return out


def pack_mask(eroded, form="rect", fill=GARBAGE):
    """(slot of H * Wp uint32 words, bbox row) of one eroded mask (H, W) bool in a stored form: "image" -- cm3d_erode_pack's, the whole
    image with wc = Wp; "rect" -- cm3d_rle_erode_pack's, the rectangle of the set pixels' words, row after row from the start of the
    slot; "stride" -- its workgroup-per-mask form: the whole image reported, only the words of the set pixels' rectangle written, at the
    image's row stride.  Words that are not written hold `fill`."""
    eroded = np.asarray(eroded, bool)
    H, W = eroded.shape
    Wp = (W + 31) // 32
    bits = np.zeros((H, Wp * 32), np.uint8)
    bits[:, :W] = eroded
    words = np.packbits(bits, axis=1, bitorder="little").view(np.uint32).reshape(H, Wp)
    slot = np.full(H * Wp, fill, np.uint32)
    bb = np.zeros(BBOX_STRIDE, np.int32)
    ys, xs = np.nonzero(eroded)
    if ys.size == 0:
        bb[:4] = W, H, -1, -1
        return slot, bb
    x0, y0, x1, y1 = int(xs.min()), int(ys.min()), int(xs.max()), int(ys.max())
    bb[:4] = x0, y0, x1, y1
    xw0, wc, rows = x0 >> 5, (x1 >> 5) - (x0 >> 5) + 1, y1 - y0 + 1
    if form == "image":
        slot[:] = words.reshape(-1)
        bb[4:] = 0, 0, Wp, H
    elif form == "rect":
        slot[:rows * wc] = words[y0:y1 + 1, xw0:xw0 + wc].reshape(-1)
        bb[4:] = xw0, y0, wc, rows
    elif form == "stride":
        img = slot.reshape(H, Wp)
        img[y0:y1 + 1, xw0:xw0 + wc] = words[y0:y1 + 1, xw0:xw0 + wc]
        bb[4:] = 0, 0, Wp, H
    else:
        raise ValueError(form)
    return slot, bb


def blob(W, H, x0, y0, w, h, seed, density=0.6):
    """An eroded mask: random pixels of the given density inside a rectangle, its four corners always set."""
    m = np.zeros((H, W), bool)
    m[y0:y0 + h, x0:x0 + w] = np.random.default_rng(seed).random((h, w)) < density
    m[y0, x0] = m[y0, x0 + w - 1] = m[y0 + h - 1, x0] = m[y0 + h - 1, x0 + w - 1] = True
    return m


def uvd_list(mask, n, seed, depth=(4.0, 60.0)):
    """n (u, v, depth, 0) rows scattered over the mask's bounds."""
    rng = np.random.default_rng(seed)
    ys, xs = np.nonzero(mask)
    out = np.zeros((n, 4), np.float32)
    if n and ys.size:
        out[:, 0] = rng.uniform(xs.min(), xs.max() + 1, n)
        out[:, 1] = rng.uniform(ys.min(), ys.max() + 1, n)
        out[:, 2] = rng.uniform(*depth, n)
    return out


class Case:
    """One call's inputs.  masks: list of (eroded (H, W) bool, form, frame, camera, list rows (n, 4), flags word)."""

    def __init__(self, name, W, H, cams, masks, per_mask=50, seed=0, max_px=0.0, kept_only=True, frame_seed=None, slack=3):
        self.name, self.W, self.H, self.per_mask, self.seed, self.max_px, self.kept_only = name, W, H, per_mask, seed, max_px, kept_only
        self.cams = np.ascontiguousarray(cams, np.float32)                  # (F, n_cams, CAM_STRIDE)
        F = self.cams.shape[0]
        self.frame_seed = np.arange(F, dtype=np.uint32) if frame_seed is None else np.asarray(frame_seed, np.uint32)
        masks = sorted(masks, key=lambda m: m[2])                           # a frame's masks lie together
        self.eroded = [m[0] for m in masks]
        packed = [pack_mask(m[0], m[1]) for m in masks]
        Wp = (W + 31) // 32
        self.packed = np.stack([p[0] for p in packed]) if masks else np.zeros((0, H * Wp), np.uint32)
        self.bbox = np.stack([p[1] for p in packed]) if masks else np.zeros((0, BBOX_STRIDE), np.int32)
        self.mask_frame = np.array([m[2] for m in masks], np.int32)
        self.mask_cam = np.array([m[3] for m in masks], np.int32)
        self.mask_off = np.searchsorted(self.mask_frame, np.arange(F + 1)).astype(np.int32)
        self.flags = np.array([m[5] for m in masks], np.int32)
        lists = [np.asarray(m[4], np.float32).reshape(-1, 4) for m in masks]
        self.off = np.concatenate([[0], np.cumsum([len(x) for x in lists])]).astype(np.int32)
        self.idx_cap = int(self.off[-1])
        # rows behind idx_cap exist and hold what must never be read: a return right on every pixel
        tail = np.zeros((slack, 4), np.float32)
        self.hit_uvd = np.concatenate(lists + [tail]) if lists else tail

    @property
    def M(self):
        return len(self.eroded)

    def host_args(self):
        return dict(packed=self.packed, bbox=self.bbox, W=self.W, H=self.H, cams=self.cams, mask_off=self.mask_off, mask_frame=self.mask_frame,
                    mask_cam=self.mask_cam, flags=self.flags, hit_uvd=self.hit_uvd, off=self.off, idx_cap=self.idx_cap, per_mask=self.per_mask,
                    seed=self.seed, max_px=self.max_px, kept_only=self.kept_only, frame_seed=self.frame_seed)


W0, H0 = 200, 120
CAMS2 = np.stack([np.stack([camera(2, 0.0), camera(1, 1700.0)]), np.stack([camera(3, 1700.0), camera(2, 0.0, skew=3.5)])])   # (2 frames, 2 cameras)


CAMS_EXACT = np.stack([np.stack([camera(1, 2000.0, exact=True), camera(2, 0.0, exact=True), camera(3, 2000.0, exact=True),
                                 camera(2, 2000.0, skew=3.5, exact=True)])])


def _m(mask, form="rect", f=0, c=0, n=40, seed=1, flags=3, lst=None):
    return (mask, form, f, c, uvd_list(mask, n, seed) if lst is None else lst, flags)


def _single(W, H, x, y):
    m = np.zeros((H, W), bool)
    m[y, x] = True
    return m


def case_shapes():
    """A = 1, A < K, A = K, A >> K; rectangles of 1, 2 and 3 words per row; pixels at bits 0 and 31; empty rows; all three stored forms;
    an empty mask; every list length next to a wave and next to the LDS stage."""
    a_eq_k = np.zeros((H0, W0), bool)
    a_eq_k[10:15, 40:50] = True                                             # 50 pixels = K
    seams = np.zeros((H0, W0), bool)
    seams[20, [32, 63, 64, 95, 96]] = True                                  # bits 0 and 31 of words 1 and 2, bit 0 of word 3
    seams[27, [31, 32, 127]] = True                                         # empty rows between; bit 31 of words 0 and 3
    gaps = blob(W0, H0, 5, 30, 90, 40, 7)
    gaps[35:50] = False                                                     # empty rows between set rows
    masks = [_m(_single(W0, H0, 77, 5), "rect", n=1), _m(blob(W0, H0, 100, 3, 6, 4, 2, 0.3), "image", n=63),
             _m(a_eq_k, "stride", n=64), _m(blob(W0, H0, 33, 60, 30, 50, 3), "rect", n=65),          # one word per row
             _m(blob(W0, H0, 20, 50, 40, 30, 4), "image", n=257), _m(blob(W0, H0, 30, 10, 70, 60, 5), "stride", n=257),   # two, three words
             _m(seams, "rect", n=7), _m(seams, "stride", n=7, seed=9), _m(gaps, "rect", n=30), _m(np.zeros((H0, W0), bool), "rect", n=5),
             _m(blob(W0, H0, 150, 80, 49, 39, 6), "rect", n=0), _m(blob(W0, H0, 0, 0, 200, 120, 8), "image", n=300)]
    return Case("shapes", W0, H0, CAMS2[:1], masks)


def case_ties():
    """Two positions equidistant from a sample (the lower one wins), duplicated rows, a NaN u, a list of NaN alone."""
    one = _single(W0, H0, 50, 40)                                           # centre (50.5, 40.5)
    eq = np.array([[60, 40.5, 9, 0], [48.5, 40.5, 7, 0], [52.5, 40.5, 8, 0], [50.5, 42.5, 6, 0]], np.float32)      # 1, 2 and 3 tie at d2 = 4
    dup = np.array([[50.5, 45.5, 5, 0]] * 3 + [[80, 80, 1, 0]], np.float32)
    nan = np.array([[np.nan, 40.5, 3, 0], [50.5, np.nan, 3, 0], [55.5, 40.5, 11, 0]], np.float32)
    only_nan = np.array([[np.nan, 1, 3, 0]], np.float32)
    big = blob(W0, H0, 40, 30, 60, 50, 11)
    lst = uvd_list(big, 64, 12)
    lst[10, 0], lst[40] = np.nan, lst[3]
    return Case("ties", W0, H0, CAMS2[:1], [_m(one, lst=eq), _m(one, lst=dup), _m(one, lst=nan), _m(one, lst=only_nan), _m(big, "image", lst=lst)])


def case_switches(kept_only=True, max_px=3.0):
    """A mask made unkept, max_px dropping some samples, cameras that cannot be inverted, frame and camera numbers out of range."""
    bad = [camera(2), camera(2), camera(2), camera(2), camera(2)]
    bad[0][45 + 8] = 1.5                # last row of K'
    bad[1][45 + 3] = 0.1                # K10
    bad[2][45 + 0] = 0.0                # K00
    bad[3][45 + 4] = np.inf             # K11
    bad[4][54] = 4                      # a stage count the record cannot hold
    cams = np.stack([np.stack([camera(2), camera(1)] + bad)])
    big = blob(W0, H0, 20, 20, 120, 80, 21)
    sparse = uvd_list(big, 12, 22)
    masks = [_m(big, "rect", lst=sparse), _m(big, "image", lst=sparse, flags=1), _m(big, "stride", lst=sparse, flags=2), _m(big, "rect", c=1, lst=sparse)]
    masks += [_m(big, "rect", c=2 + i, lst=sparse) for i in range(5)] + [_m(big, "rect", c=7, lst=sparse)]
    return Case("switches", W0, H0, cams, masks, max_px=max_px, kept_only=kept_only)


def case_seeds():
    """Two frames with equal masks and lists: different frame seeds give different pixels; the cameras have 3 and 1 stages."""
    big = blob(W0, H0, 10, 10, 150, 90, 31)
    lst = uvd_list(big, 100, 32)
    return Case("seeds", W0, H0, CAMS2, [_m(big, "rect", f=0, c=0, lst=lst), _m(big, "rect", f=0, c=1, lst=lst), _m(big, "rect", f=1, c=0, lst=lst),
                                         _m(big, "rect", f=1, c=1, lst=lst)], frame_seed=[5, 6])


def case_round_trip():
    """Cameras of 1, 2 and 3 stages with t_pre and t_post, at 0 and 2 km, one with K01 != 0, whose rotations are exact in float32."""
    big = blob(W0, H0, 10, 10, 150, 90, 51)
    return Case("round_trip", W0, H0, CAMS_EXACT, [_m(big, "rect", c=c, lst=uvd_list(big, 80, 52 + c)) for c in range(4)])


def case_full_image():
    """One 1600 x 900 full mask with K = 1024: A = 1 440 000 and the largest product, 1024 A = 1.47e9.  The list is short: the test
    takes seconds."""
    W, H = 1600, 900
    full = np.ones((H, W), bool)
    lst = uvd_list(full, 65, 41)
    return Case("full_image", W, H, CAMS2[:1], [_m(full, "image", lst=lst)], per_mask=1024)


def case_wide_products():
    """One 2112 x 2048 full mask with K = 1024: A = 4 325 376, so that (j + 1) A passes 2^32 (from j = 992 on): products of 32 bits
    would wrap.  Rows of 66 words: the row's words take two rounds of the wave."""
    W, H = 2112, 2048
    full = np.ones((H, W), bool)
    lst = uvd_list(full, 65, 43)
    return Case("wide_products", W, H, CAMS2[:1], [_m(full, "image", lst=lst)], per_mask=1024)


def cases():
    return [case_shapes(), case_ties(), case_switches(), case_switches(kept_only=False, max_px=0.0), case_seeds(), case_round_trip()]
