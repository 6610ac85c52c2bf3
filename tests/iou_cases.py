"""Seeded, deterministic box pairs for the rotated-box IoU tests (tests/box_iou_exact.py gives their exact values).

Every family is built in A's own frame and placed at the offsets OFFSETS (global-frame magnitudes) and at the headings
HEADINGS: exactly 0, +-pi/2 and pi (unit vectors without rounding), the rounded cos / sin of pi/2, pi and +-pi/4, and
random ones.  A record is cx, cy, length, width, c, s, cz, height (float64, waymo_eval.BOX_STRIDE); its first six fields
are the cm3d_bev_match record.  pairs() returns (family, a, b) triples."""
import functools
import math
from fractions import Fraction as Q

import numpy as np

from tests import box_iou_exact as X

OFFSETS = (0.0, 1600.0, 10000.0)
_R = np.random.default_rng(20261016)
HEADINGS = (("0", 1.0, 0.0), ("pi/2", 0.0, 1.0), ("-pi/2", 0.0, -1.0), ("pi", -1.0, 0.0),
            ("pi/2~", math.cos(math.pi / 2), math.sin(math.pi / 2)), ("pi~", math.cos(math.pi), math.sin(math.pi)),
            ("pi/4", math.cos(math.pi / 4), math.sin(math.pi / 4)), ("-pi/4", math.cos(-math.pi / 4), math.sin(-math.pi / 4)),
            *((f"rand{i}", math.cos(h), math.sin(h)) for i, h in enumerate(_R.uniform(-math.pi, math.pi, 2))))

# Near-identical pairs with the most clip vertices found by a seeded search of jittered records (fields moved by 1-6
# ulps, headings at multiples of pi/4, offsets 0 / 1.6 km / 10 km).  Exact clipping gives at most 8; the rounded
# predicates of bev_inter_area give up to max_vertices.  Float64 hex literals: cx, cy, l, w, c, s.
HIGH_VERTEX = [
    # (max_vertices, a, b); the first two are the pairs named in the issue that asked for these tests
    (10, ['0x1.2d1f4a8f78cecp+10', '0x1.442e7e8bbe760p+10', '0x1.8789a15326f8ap+0', '0x1.61b0dc287c823p+0', '-0x1.6a09e667f3bccp-1', '0x1.6a09e667f3bcdp-1'],
         ['0x1.2d1f4a8f78cecp+10', '0x1.442e7e8bbe760p+10', '0x1.8789a15326f8ap+0', '0x1.61b0dc287c823p+0', '-0x1.6a09e667f3bcbp-1', '0x1.6a09e667f3bccp-1']),
    (9, ['0x1.26c8844192884p+10', '0x1.aa8f826a11b98p+8', '0x1.8d7d335d04f30p+2', '0x1.46f3be0c967b8p+1', '-0x1.6a09e667f3bccp-1', '0x1.6a09e667f3bcdp-1'],
        ['0x1.26c8844192884p+10', '0x1.aa8f826a11b98p+8', '0x1.8d7d335d04f30p+2', '0x1.46f3be0c967b7p+1', '-0x1.6a09e667f3bccp-1', '0x1.6a09e667f3bcdp-1']),
    (10, ['0x1.484eca56c341ap+5', '0x1.8c86827362ea0p+5', '0x1.6768f2567de90p+2', '0x1.d897ef053d060p-1', '-0x1.6a09e667f3bccp-1', '-0x1.6a09e667f3bcdp-1'],
         ['0x1.484eca56c341ap+5', '0x1.8c86827362ea0p+5', '0x1.6768f2567de90p+2', '0x1.d897ef053d05ep-1', '-0x1.6a09e667f3bccp-1', '-0x1.6a09e667f3bcdp-1']),
    (10, ['0x1.8f790f17b3be5p+10', '0x1.974a0cb54f5acp+10', '0x1.199ef20477167p+2', '0x1.423f93bfee8ebp+0', '-0x1.6a09e667f3bccp-1', '0x1.6a09e667f3bcdp-1'],
         ['0x1.8f790f17b3be5p+10', '0x1.974a0cb54f5acp+10', '0x1.199ef20477167p+2', '0x1.423f93bfee8eap+0', '-0x1.6a09e667f3bccp-1', '0x1.6a09e667f3bcdp-1']),
    (10, ['0x1.38aa7a667041ap+13', '0x1.38e3aeac2e01fp+13', '0x1.6295df6b01bbap+2', '0x1.9db5ed9273cb5p+1', '0x1.6a09e667f3bcdp-1', '-0x1.6a09e667f3bccp-1'],
         ['0x1.38aa7a667041ap+13', '0x1.38e3aeac2e01fp+13', '0x1.6295df6b01bbap+2', '0x1.9db5ed9273cb5p+1', '0x1.6a09e667f3bcdp-1', '-0x1.6a09e667f3bcap-1']),
]


def rec(cx, cy, l, w, c, s, cz=0.0, h=1.5):
    return [float(cx), float(cy), float(l), float(w), float(c), float(s), float(cz), float(h)]


def place(a, u, v, l, w, c, s, cz=None, h=None):
    """Box of size l x w and axis (c, s) centred at A's centre + u A's length axis + v A's width axis (float64)."""
    ca, sa = a[4], a[5]
    return rec(a[0] + (u * ca - v * sa), a[1] + (u * sa + v * ca), l, w, c, s, a[6] if cz is None else cz, a[7] if h is None else h)


def turn(c, s, cr, sr):
    """Axis (c, s) turned by the rotation (cr, sr), float64."""
    return c * cr - s * sr, c * sr + s * cr


def _jitter(rng, r):
    """Every non-zero field moved by 1-6 ulps (up or down: a step of the int64 view)."""
    v = np.array(r, np.float64)
    steps = rng.integers(1, 7, v.size) * rng.choice([-1, 1], v.size)
    out = (v.view(np.int64) + steps).view(np.float64)
    out[v == 0.0] = 0.0
    return [float(x) for x in out]


def _family_pairs(name, a, c, s, rng):
    """Pairs of one family for base box a (heading c, s)."""
    l, w = a[2], a[3]
    out = []
    if name == "identical":
        out.append((a, list(a)))
    elif name == "near_identical":
        for _ in range(3):
            out.append((a, _jitter(rng, a[:6]) + a[6:]))
        out.append((a, a[:4] + _jitter(rng, a[4:6]) + a[6:]))                           # heading only
    elif name == "turned":
        out.append((a, rec(a[0], a[1], l, w, -c, -s, a[6], a[7])))                       # turned by pi
        sq = rec(a[0], a[1], l, l, c, s, a[6], a[7])
        out.append((sq, rec(a[0], a[1], l, l, -s, c, a[6], a[7])))                        # square turned by pi/2
    elif name == "shared_edge":
        out.append((a, place(a, l, 0.0, l, w, c, s)))                                      # full shared end edge
        out.append((a, place(a, 0.0, w, l, w, c, s)))                                      # full shared long edge
        out.append((a, place(a, 0.75 * l, 0.25 * w, 0.5 * l, 0.5 * w, c, s)))              # collinear, partial
        out.append((a, place(a, 0.3 * l, 0.5 * w + 0.25, 0.8 * l, 0.5, c, s)))             # collinear, offset along
        out.append((a, place(a, 0.5 * l - 0.125, 0.0, 0.25, 0.5 * w, c, s)))               # inside, sharing a part of an edge
    elif name == "corner":
        out.append((a, place(a, l, w, l, w, c, s)))                                        # corner on corner
        cr = sr = math.sqrt(0.5)
        b = place(a, 0.5 * l + 0.5, 0.0, 0.5 * math.sqrt(2.0), 0.5 * math.sqrt(2.0), *turn(c, s, cr, sr))
        out.append((a, b))                                                                 # vertex on an edge
        out.append((a, place(a, 0.5 * l + 0.4999, 0.0, 0.5 * math.sqrt(2.0), 0.5 * math.sqrt(2.0), *turn(c, s, cr, sr))))
    elif name == "containment":
        out.append((a, place(a, 0.0, 0.0, 0.5 * l, 0.5 * w, c, s)))
        cr, sr = math.cos(0.3), math.sin(0.3)
        out.append((a, place(a, 0.1 * l, -0.1 * w, 0.25 * min(l, w), 0.2 * min(l, w), *turn(c, s, cr, sr))))
    elif name == "thin":
        cr, sr = math.cos(0.5), math.sin(0.5)
        for tw in (1e-3, 1e-2):
            out.append((rec(a[0], a[1], 4.0, tw, c, s, a[6], a[7]), place(a, 0.1, 0.05, 2.0, 2.0, *turn(c, s, cr, sr))))
        th = 5e-4                                                                          # congruent thin boxes: octagon
        out.append((rec(a[0], a[1], 1.0, 1e-3, c, s, a[6], a[7]),
                    rec(a[0], a[1], 1.0, 1e-3, *turn(c, s, math.cos(th), math.sin(th)), a[6], a[7])))
        out.append((rec(a[0], a[1], 2.0, 2e-3, c, s, a[6], a[7]), place(a, 1e-4, 0.0, 2.0, 2e-3, *turn(c, s, math.cos(-th), math.sin(-th)))))
    elif name == "tiny_overlap":
        for d in (1e-9, 1e-8, 1e-7, 1e-6):
            out.append((a, place(a, l - d, 0.0, l, w, c, s)))
    elif name == "early_out":                                                          # along the diagonal, corners meeting
        for e in (-1e-3, -1e-6, -1e-9, 0.0, 1e-9, 1e-6):
            out.append((a, place(a, l * (1.0 + e), w * (1.0 + e), l, w, c, s)))
    elif name == "z":
        h = a[7]
        out.append((a, rec(a[0], a[1], l, w, c, s, a[6] + h, h)))                          # touching
        out.append((a, rec(a[0], a[1], l, w, c, s, a[6] + 0.25 * h, 0.25 * h)))           # nested
        out.append((a, rec(a[0], a[1], l, w, c, s, a[6] + 0.5 * h, 0.0)))                  # zero height
        out.append((a, rec(a[0], a[1], l, w, c, s, a[6], float(np.nextafter(h, 2 * h)))))  # one ulp apart
        out.append((a, place(a, 0.3 * l, 0.2 * w, l, w, c, s, a[6] + 0.9 * h, 2.0 * h)))   # partial overlap, shifted
    elif name == "random":
        for scale in (0.01, 1.0, 100.0):
            for _ in range(2):
                hb = rng.uniform(-math.pi, math.pi)
                sz = rng.uniform(0.3, 5.0, 2) * scale
                b0 = rec(a[0], a[1], *(rng.uniform(0.3, 5.0, 2) * scale), c, s, a[6], a[7])
                out.append((b0, place(b0, *(rng.uniform(-2.0, 2.0, 2) * scale), *sz, math.cos(hb), math.sin(hb),
                                      a[6] + rng.uniform(-0.5, 0.5) * a[7], a[7] * rng.uniform(0.5, 2.0))))
    else:
        raise KeyError(name)
    return out


FAMILIES = ("identical", "near_identical", "turned", "shared_edge", "corner", "containment", "thin", "tiny_overlap",
            "early_out", "z", "random")


@functools.lru_cache(None)
def pairs():
    """Every family at every offset and heading: a list of (family, a, b)."""
    rng = np.random.default_rng(7)
    out = []
    for off in OFFSETS:
        for hname, c, s in HEADINGS:
            for fam in FAMILIES:
                l, w = (4.5, 2.0) if fam != "identical" else (0.9, 0.8)
                a = rec(off + 0.5, off * 0.75 - 1.25, l, w, c, s, 0.75, 1.5)
                for pa, pb in _family_pairs(fam, a, c, s, rng):
                    out.append((fam, pa, pb))
    for m, a, b in HIGH_VERTEX:
        out.append(("high_vertex", X.fromhex(a) + [0.75, 1.5], X.fromhex(b) + [0.75, 1.5]))
    return out


# ------------------------------------------------------------------------------------------------ threshold straddlers
def straddle(a, thr, delta, along, iou_fn=X.bev_iou):
    """B = A slid along A's length (along=0) or width (along=1) axis so that the exact IoU is thr + delta to about
    1e-13: a float64 bisection on the shift with the exact IoU as the test.  Returns B."""
    target = Q(thr) + Q(delta)
    size = a[2 + along]
    def mk(t):
        return place(a, t, 0.0, a[2], a[3], a[4], a[5]) if along == 0 else place(a, 0.0, t, a[2], a[3], a[4], a[5])
    g = size * (1.0 - float(target)) / (1.0 + float(target))           # same boxes sliding: IoU = (L - t) / (L + t)
    lo, hi = max(g * (1.0 - 1e-5), 0.0), min(g * (1.0 + 1e-5), size)
    if iou_fn(a, mk(lo)) < target:
        lo = 0.0
    if iou_fn(a, mk(hi)) >= target:
        hi = size
    for _ in range(200):
        mid = 0.5 * (lo + hi)
        if mid in (lo, hi):
            break
        if iou_fn(a, mk(mid)) >= target:
            lo = mid
        else:
            hi = mid
    return mk(lo) if delta > 0 else mk(hi)


@functools.lru_cache(None)
def straddlers(thrs=(0.2, 0.5, 0.7), deltas=(1e-9, -1e-9, 1e-6, -1e-6), dim=2):
    """(thr, delta, a, b): exact IoU of a, b within ~1e-13 of thr + delta (above thr for delta > 0, below for delta < 0),
    at every offset, three headings and both sliding axes."""
    out = []
    fn = X.bev_iou if dim == 2 else X.iou3d
    for off in OFFSETS:
        for hname, c, s in (HEADINGS[0], HEADINGS[6], HEADINGS[8]):
            a = rec(off + 0.5, off * 0.75 - 1.25, 4.5, 2.0, c, s, 0.75, 1.5)
            for thr in thrs:
                for d in deltas:
                    for along in (0, 1):
                        out.append((thr, d, a, straddle(a, thr, d, along, fn)))
    return out
