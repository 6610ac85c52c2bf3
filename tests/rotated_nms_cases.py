"""Seeded frames for the rotated-box NMS tests (cm3d_rotated_nms, cm3d_amd.nms.rotated_nms_host) and the exact greedy NMS in
rational arithmetic they are held against (overlaps from tests/box_iou_exact.py).

A case is a dict: name, rec (n, 6) float64 records, score (n,), group (n,) int, thr (one float64 per group), agnostic, measures (the
measures it is meant for), exact (True: the exact-geometry condition below is asserted for it and its result must equal exact_nms),
and optionally want (the expected keep).

The exact-geometry condition (undecidable_pairs finds none): for every pair the rule could compare -- both orders, since either box can be the
lower-scored one -- |measure_exact - thr[group of the lower box]| exceeds the float64 error bound of that pair: X.bev_eval's for the
IoU; for cover = I / A_j the bound dI / A_j + cover * rel(A_j) + 4 u with dI = X.inter_bound and rel(A_j) = u + |c^2 + s^2 - 1| the
relative error of the float64 area l * w against the exact one.  Float64 then decides every pair as exact arithmetic does.  Pairs
whose circumscribed circles are apart by more than a part in 10^3 have the exact overlap 0 without a clip (neighbours)."""
import functools
import math
from fractions import Fraction as Q

import numpy as np

from tests import box_iou_exact as X
from tests import iou_cases as ic

MEASURES = ("iou", "cover")
MAX_BOXES = 1024                       # CM3D_MAX_MASKS_PER_FRAME
CROWD_SIZES = (1, 2, 63, 64, 65, 200, 1024)
CROWD_THR = (0.4, 0.3, 0.5)            # per group
U = X.U


def is_live(r):
    return float(r[2]) * float(r[3]) > 0.0 and math.isfinite(float(r[0])) and math.isfinite(float(r[1]))


def _radius(r):
    return 0.5 * np.hypot(r[..., 2], r[..., 3]) * np.hypot(r[..., 4], r[..., 5])


def neighbours(rec, rows=None):
    """Per box (of `rows`: a dict) the other live boxes whose circumscribed circles are not certainly apart.  Float64 with a margin of a part in 10^3 of
    the radii (live boxes here are at least 0.25 m across, coordinates below 2e4 m: rounding moves a distance by 1e-11 m at most), so
    every pair left out has an empty intersection in exact arithmetic too."""
    rec = np.asarray(rec, np.float64)[:, :6]
    with np.errstate(invalid="ignore"):
        live = (rec[:, 2] * rec[:, 3] > 0.0) & np.isfinite(rec[:, 0]) & np.isfinite(rec[:, 1])          # is_live
    rad = _radius(rec)
    out = {}
    with np.errstate(invalid="ignore"):
        for i in (range(len(rec)) if rows is None else rows):
            d = np.hypot(rec[:, 0] - rec[i, 0], rec[:, 1] - rec[i, 1])
            near = live & live[i] & (d <= (rad + rad[i]) * 1.001 + 1e-6)
            near[i] = False
            out[i] = np.flatnonzero(near)
    return out if rows is not None else [out[i] for i in range(len(rec))]


def _apart(a, b):
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    return bool(np.hypot(b[0] - a[0], b[1] - a[1]) > (_radius(a) + _radius(b)) * 1.001 + 1e-6)


@functools.lru_cache(maxsize=None)
def _inter(a, b):
    """Exact intersection area of two live records (tuples); symmetric in exact arithmetic, cached in one order."""
    return Q(0) if _apart(a, b) else X.inter_area(a, b)


def inter_exact(a, b):
    a, b = tuple(float(v) for v in a[:6]), tuple(float(v) for v in b[:6])
    return _inter(a, b) if a <= b else _inter(b, a)


def exact_measure(a, b, measure):
    """(exact measure of kept box a on lower box b, bound on |float64 value - exact|) for live records."""
    inter = inter_exact(a, b)
    dI = X.inter_bound(a, b)
    area_a, area_b = X.box_area(a), X.box_area(b)
    if measure == "iou":
        uni = area_a + area_b - inter
        iou = inter / uni
        return iou, (dI + float(iou) * (X._dA(a) + X._dA(b) + dI)) / float(uni) + 4 * U        # X.bev_eval's bound
    cover = inter / area_b
    rel = X._dA(b) / (float(b[2]) * float(b[3]))
    return cover, (dI / float(area_b) + float(cover) * rel) * (1.0 + 2.0 * rel) + 4 * U


def cover(a, b):
    """Exact cover as an iou_fn of iou_cases.straddle."""
    return inter_exact(a, b) / X.box_area(b)


def undecidable_pairs(rec, group, thr, agnostic, measures=MEASURES, only=None, factor=1.0):
    """Pairs (kept, lower, measure) of one frame that violate the exact-geometry condition.  only: the pairs with these boxes.
    factor: the condition with that multiple of the bound (for records whose c, s the device may round differently)."""
    bad = []
    n = min(len(rec), MAX_BOXES)
    assert all(float(t) > 8 * U for t in thr)                          # pairs apart: measure 0 against a bound of 4 u
    near = neighbours(rec[:n], only)
    for i in (range(n) if only is None else only):
        for j in near[i]:
            if (only is None and j < i) or not (agnostic or group[i] == group[j]):
                continue
            for m in measures:
                for a, b in ((i, j), (j, i)):
                    v, bound = exact_measure(rec[a], rec[b], m)
                    if not abs(v - Q(float(thr[group[b]]))) > factor * bound:
                        bad.append((a, int(b), m))
    return bad


def exact_nms(rec, score, group, thr, measure, agnostic, take=None):
    """The rule of cm3d_rotated_nms on one frame with exact overlaps: keep (n,) int32."""
    n = len(rec)
    keep = np.zeros(n, np.int32)
    idx = [k for k in range(min(n, MAX_BOXES)) if take is None or take[k]]
    order = sorted(idx, key=lambda k: (-float(score[k]), -k))
    rank = {k: r for r, k in enumerate(order)}
    near = neighbours(rec[:min(n, MAX_BOXES)])
    sup = set()
    for r, i in enumerate(order):
        if i in sup:
            continue
        keep[i] = 1
        for j in near[i]:                                              # (live boxes only; everyone else has overlap 0 with i)
            j = int(j)
            if rank.get(j, -1) <= r or j in sup or not (agnostic or group[j] == group[i]):
                continue
            if exact_measure(rec[i], rec[j], measure)[0] > Q(float(thr[group[j]])):
                sup.add(j)
    return keep


def _case(name, rec, score, group=None, thr=(0.4,), agnostic=False, measures=MEASURES, exact=False, want=None):
    rec = np.array([list(r[:6]) for r in rec], np.float64).reshape(-1, 6)
    rec.setflags(write=False)
    n = len(rec)
    return dict(name=name, rec=rec, score=np.asarray(score, np.float64).reshape(n),
                group=np.zeros(n, np.int32) if group is None else np.asarray(group, np.int32).reshape(n),
                thr=np.asarray(thr, np.float64).reshape(-1), agnostic=bool(agnostic), measures=tuple(measures), exact=exact,
                want=None if want is None else np.asarray(want, np.int32))


# ------------------------------------------------------------------------------------------------ small frames
@functools.lru_cache(None)
def pair_cases():
    """Every pair of iou_cases.pairs() (HIGH_VERTEX among them) as a two-box frame, the first box scored higher."""
    return [_case(f"pair{k}:{fam}", [a, b], [0.9, 0.5]) for k, (fam, a, b) in enumerate(ic.pairs())]


@functools.lru_cache(None)
def cover_straddlers(thrs=(0.1, 0.4), deltas=(1e-9, -1e-9, 1e-6, -1e-6)):
    """iou_cases.straddlers' construction with the exact cover as the measure: (thr, delta, a, b)."""
    out = []
    for off in ic.OFFSETS:
        for hname, c, s in (ic.HEADINGS[0], ic.HEADINGS[6], ic.HEADINGS[8]):
            a = ic.rec(off + 0.5, off * 0.75 - 1.25, 4.5, 2.0, c, s, 0.75, 1.5)
            for thr in thrs:
                for d in deltas:
                    for along in (0, 1):
                        out.append((thr, d, a, ic.straddle(a, thr, d, along, cover)))
    return out


@functools.lru_cache(None)
def straddler_cases():
    """Two-box frames at the threshold they straddle: the lower box goes iff delta > 0."""
    out = []
    for m, rows in (("iou", ic.straddlers()), ("cover", cover_straddlers())):
        for k, (thr, d, a, b) in enumerate(rows):
            out.append(_case(f"straddle:{m}{k}:{thr}{d:+g}", [a, b], [0.9, 0.5], thr=(thr,), measures=(m,), exact=True, want=[1, 0 if d > 0 else 1]))
    return out


def _box(cx, cy, l, w, h):
    return ic.rec(cx, cy, l, w, math.cos(h), math.sin(h))


@functools.lru_cache(None)
def crafted_cases():
    out = []
    # chains: A suppresses B, and B alone would suppress C: C is kept (IoU of neighbours 0.6, of A and C 0.25)
    for off in ic.OFFSETS:
        a = _box(off + 3.0, off - 2.0, 4.0, 2.0, 0.3)
        chain = [a, ic.place(a, 1.0, 0.0, 4.0, 2.0, a[4], a[5])[:6], ic.place(a, 2.0, 0.0, 4.0, 2.0, a[4], a[5])[:6]]
        out.append(_case(f"chain@{off:g}", chain, [0.9, 0.8, 0.7], exact=True, measures=("iou",), want=[1, 0, 1]))
        out.append(_case(f"chain_reversed@{off:g}", chain, [0.7, 0.8, 0.9], exact=True, measures=("iou",), want=[1, 0, 1]))
        out.append(_case(f"chain_middle_first@{off:g}", chain, [0.7, 0.9, 0.8], exact=True, measures=("iou",), want=[0, 1, 0]))
    # score ties: the higher index wins
    b0 = _box(10.0, 20.0, 4.0, 2.0, 1.0)
    b1 = ic.place(b0, 0.5, 0.1, 4.0, 2.0, b0[4], b0[5])[:6]
    out.append(_case("tie2", [b0, b1], [0.5, 0.5], exact=True, want=[0, 1]))
    out.append(_case("tie3", [b0, b1, ic.place(b0, 0.2, -0.1, 4.2, 1.9, b0[4], b0[5])[:6]], [0.5, 0.5, 0.5], exact=True, want=[0, 0, 1]))
    out.append(_case("tie_below_a_better_one", [b0, b1, _box(40.0, 20.0, 4.0, 2.0, 0.0), b1], [0.5, 0.9, 0.5, 0.5], want=[0, 1, 1, 0]))
    # two groups overlapping fully: both kept; one kept when agnostic (the higher score)
    out.append(_case("two_groups", [b0, b0], [0.4, 0.6], group=[0, 1], thr=(0.4, 0.4), want=[1, 1]))
    out.append(_case("two_groups_agnostic", [b0, b0], [0.4, 0.6], group=[0, 1], thr=(0.4, 0.4), agnostic=True, want=[0, 1]))
    # per-group thresholds that differ: the group of the lower box decides (IoU 0.6 between the two)
    pair = [b0, ic.place(b0, 1.0, 0.0, 4.0, 2.0, b0[4], b0[5])[:6]]
    out.append(_case("thr_of_j_low", pair, [0.9, 0.8], group=[0, 1], thr=(0.9, 0.5), agnostic=True, exact=True, measures=("iou",), want=[1, 0]))
    out.append(_case("thr_of_j_high", pair, [0.8, 0.9], group=[0, 1], thr=(0.9, 0.5), agnostic=True, exact=True, measures=("iou",), want=[1, 1]))
    # cover is not symmetric: a small box inside a large one goes, the large one under a small one stays
    big, small = _box(5.0, 5.0, 6.0, 3.0, 0.2), _box(5.2, 5.1, 1.5, 1.0, 0.9)
    out.append(_case("cover_small_inside", [big, small], [0.9, 0.8], exact=True, measures=("cover",), want=[1, 0]))
    out.append(_case("cover_big_under_small", [big, small], [0.8, 0.9], exact=True, measures=("cover",), want=[1, 1]))
    out.append(_case("iou_small_inside", [big, small], [0.9, 0.8], exact=True, measures=("iou",), want=[1, 1]))
    return out


# ------------------------------------------------------------------------------------------------ crowds
def _draw(rng, off, side, rec, group, free):
    """A new box, or (more than half of the time) a second or third detection of an earlier one: `free` lists the boxes that may
    still get one (clusters stay at three boxes, so that the pairs to decide exactly stay a few per box)."""
    if len(free) and rng.random() < 0.6:
        k = free.pop(int(rng.integers(0, len(free))))
        r = rec[k]
        h = math.atan2(r[5], r[4]) + rng.normal(scale=0.1)
        g = group[k] if rng.random() < 0.85 else int(rng.integers(0, len(CROWD_THR)))
        return _box(r[0] + rng.normal(scale=0.06 * r[2]), r[1] + rng.normal(scale=0.06 * r[2]), r[2] * rng.uniform(0.9, 1.1),
                    r[3] * rng.uniform(0.9, 1.1), h)[:6], g, []
    k = len(rec)
    return (_box(off + rng.uniform(0.0, side), 0.75 * off + rng.uniform(0.0, side), rng.uniform(1.0, 6.0), rng.uniform(0.5, 2.5),
                 rng.uniform(-math.pi, math.pi))[:6], int(rng.integers(0, len(CROWD_THR))), [k, k])


@functools.lru_cache(None)
def crowd(n, off, seed=0, tie=False):
    """n boxes of three groups around (off, 0.75 off): random sizes and headings, more than half of them second or third detections of
    an earlier box (jittered centre, size and heading).  A box that would put a pair inside its error bound of a threshold (any group's,
    either measure, class-aware or agnostic) is drawn again here, at construction."""
    rng = np.random.default_rng([20261019, n, int(off), seed])
    side = 10.0 * math.sqrt(n) + 4.0
    rec, group, free, k = np.zeros((n, 6)), [], [], 0
    while k < n:
        rec[k], g, more = _draw(rng, off, side, rec[:k], group, free)
        # (agnostic: every pair, both orders)
        if not undecidable_pairs(rec[:k + 1], group + [g], CROWD_THR, True, only=[k]):
            group.append(g)
            free += more
            k += 1
    score = 0.05 + 0.9 * (rng.permutation(n) + 0.5) / n
    if tie and n >= 40:
        k = int(rng.integers(0, n))
        near = np.argsort(np.hypot(rec[:, 0] - rec[k, 0], rec[:, 1] - rec[k, 1]))[:12]
        score[near] = 0.5123456789
    return rec, score, group


@functools.lru_cache(None)
def crowd_cases():
    out = []
    for n in CROWD_SIZES:
        for off in ic.OFFSETS:
            rec, score, group = crowd(n, off, tie=n in (65, 200))
            for agn in (False, True):
                if agn and n == 1024 and off != ic.OFFSETS[1]:
                    continue                                        # (the agnostic pass over the largest crowd at one offset)
                out.append(_case(f"crowd{n}@{off:g}{'/agnostic' if agn else ''}", rec, score, group, CROWD_THR, agn, exact=True))
    return out


@functools.lru_cache(None)
def special_cases():
    """A zero-area box and a NaN-centre box inside a crowd (each with the top score, so that they would suppress if they could);
    a frame of 1030 boxes: the last 6 get keep 0."""
    out = []
    rec, score, group = crowd(65, 1600.0, seed=5)
    rec, score = rec.copy(), score.copy()
    rec[10][2] = 0.0; score[10] = 0.99
    rec[20][0] = float("nan"); score[20] = 0.98
    rec[30][3] = -1.0; score[30] = 0.001
    rec[40][1] = float("inf"); score[40] = 0.002
    rec[50][2] = float("nan")
    out.append(_case("degenerate_in_crowd", rec, score, group, CROWD_THR, exact=True))
    out.append(_case("degenerate_in_crowd/agnostic", rec, score, group, CROWD_THR, True, exact=True))
    # 1030 boxes: the 1024 of a crowd, then copies of its six best boxes with better scores still -- they would be kept and would
    # suppress their originals if they took part
    rec, score, group = crowd(MAX_BOXES, 0.0)
    top = [int(k) for k in np.argsort(-score)[:6]]
    out.append(_case("beyond_the_frame_limit", np.concatenate([rec, rec[top]]), list(score) + [0.99 + 0.001 * q for q in range(6)],
                     list(group) + [group[k] for k in top], CROWD_THR, exact=True))
    return out


def all_cases():
    return pair_cases() + straddler_cases() + crafted_cases() + crowd_cases() + special_cases()


@functools.lru_cache(None)
def exact_results():
    """{(case name, measure): keep of exact_nms} for the cases marked exact, computed once per process."""
    return {(c["name"], m): exact_nms(c["rec"], c["score"], c["group"], c["thr"], m, c["agnostic"])
            for c in all_cases() if c["exact"] for m in c["measures"]}


def batch(cases, measure):
    """The cases meant for `measure`, class-aware and agnostic apart, each laid out as the frames of one call with an empty frame
    between every two and every case's groups renumbered into one threshold table: {agnostic: (cases, rec, score, group, frame_off, thr)}."""
    out = {}
    for agn in (False, True):
        sel = [c for c in cases if measure in c["measures"] and c["agnostic"] == agn]
        if not sel:
            continue
        off, g0, groups, frame_off = 0, 0, [], [0]
        for c in sel:
            groups.append(c["group"] + g0)
            g0 += len(c["thr"])
            off += len(c["rec"])
            frame_off += [off, off]                                 # the case's frame, then an empty one
        out[agn] = (sel, np.concatenate([c["rec"] for c in sel]), np.concatenate([c["score"] for c in sel]),
                    np.concatenate(groups).astype(np.int32), np.array(frame_off, np.int32), np.concatenate([c["thr"] for c in sel]))
    return out


def split(cases, frame_off, keep):
    """keep of a batch() call back per case."""
    return [keep[frame_off[2 * k]:frame_off[2 * k + 1]] for k in range(len(cases))]
