"""The rotated-box IoU of the CPU oracle (orc_bev_iou, orc_bev_match) and of the host evaluator (waymo_eval.iou3d,
_clip_area) against exact rational geometry (tests/box_iou_exact.py) on the families of tests/iou_cases.py: within the
stated error bound, exact zeros, quantised weights and threshold decisions, clip vertex counts within the buffers."""
import functools
import math
from fractions import Fraction as Q

import numpy as np

from cm3d_amd import waymo_eval as we
from tests import box_iou_exact as X
from tests import iou_cases as C


@functools.lru_cache(None)
def _exact():
    """(family, a, b, exact bev IoU, bev bound, exact 3D IoU, 3D bound) of every pair."""
    return [(fam, a, b, *X.bev_eval(a, b), *X.eval3d(a, b)) for fam, a, b in C.pairs()]


def _rec(a):
    return np.array(a, np.float64)


# ------------------------------------------------------------------------------------------------ the reference itself
def test_exact_known_answers():
    def B(cx, cy, l, w, c, s, cz=0.0, h=1.0):
        return [cx, cy, l, w, c, s, cz, h]
    sq = B(0.0, 0.0, 2.0, 2.0, 1.0, 0.0)
    assert X.bev_iou(sq, sq) == 1
    assert X.bev_iou(sq, B(1.0, 0.0, 2.0, 2.0, 1.0, 0.0)) == Q(1, 3)
    assert X.bev_iou(B(0.0, 0.0, 4.0, 4.0, 1.0, 0.0), B(0.2, -0.1, 1.0, 1.0, 0.0, 1.0)) == Q(1, 16)        # contained
    c, s = math.cos(0.7), math.sin(0.7)            # rounded axes: the exact boxes are squares of area side^2 (c^2 + s^2)
    assert X.bev_iou(B(0.0, 0.0, 4.0, 4.0, c, s), B(0.2, -0.1, 1.0, 1.0, c, s)) == Q(1, 16)
    assert X.bev_iou(sq, B(5.0, 0.0, 2.0, 2.0, math.cos(0.3), math.sin(0.3))) == 0                  # disjoint
    assert X.bev_iou(sq, B(2.0, 0.0, 2.0, 2.0, 1.0, 0.0)) == 0                                      # sharing an edge
    assert X.bev_iou(sq, B(2.0, 2.0, 2.0, 2.0, 1.0, 0.0)) == 0                                      # corner on corner
    assert X.bev_iou(sq, B(0.0, 0.0, 2.0, 2.0, 0.0, 1.0)) == 1                                      # square turned by pi/2
    assert X.bev_iou(B(0.0, 0.0, 4.0, 2.0, 1.0, 0.0), B(0.0, 0.0, 4.0, 2.0, 0.0, 1.0)) == Q(1, 3)
    assert X.bev_iou(B(0.0, 0.0, 4.0, 2.0, 1.0, 0.0), B(0.0, 0.0, 4.0, 2.0, -1.0, 0.0)) == 1         # turned by pi
    c4 = math.cos(math.pi / 4)
    octagon = X.bev_iou(sq, B(0.0, 0.0, 2.0, 2.0, c4, c4))
    oct_area = 8 * (math.sqrt(2) - 1)
    assert abs(float(octagon) - oct_area / (8 - oct_area)) < 1e-15
    assert len(X.intersection(sq, B(0.0, 0.0, 2.0, 2.0, c4, c4))) == 8
    assert X.bev_iou(sq, B(0.0, 0.0, 0.0, 0.0, 1.0, 0.0)) == 0                                      # zeros(D): no box
    # 3D: half the height overlapping, same footprint -> 1/3; touching in z -> 0
    assert X.iou3d(B(0, 0, 2, 2, 1, 0, 0.0, 2.0), B(0, 0, 2, 2, 1, 0, 1.0, 2.0)) == Q(1, 3)
    assert X.iou3d(B(0, 0, 2, 2, 1, 0, 0.0, 2.0), B(0, 0, 2, 2, 1, 0, 2.0, 2.0)) == 0
    # identical records: exactly 1 whatever the heading's rounding
    for fam, a, b, e, *_ in _exact():
        if fam == "identical":
            assert e == 1


def test_exact_equals_rasterisation():
    rng = np.random.default_rng(3)
    n = 2000
    xs = (np.arange(n) + 0.5) / n * 12 - 6
    Xg, Yg = np.meshgrid(xs, xs)
    cell = (12 / n) ** 2

    def inside(r):
        dx, dy = Xg - r[0], Yg - r[1]
        u, v = dx * r[4] + dy * r[5], -dx * r[5] + dy * r[4]
        return (np.abs(u) <= r[2] / 2) & (np.abs(v) <= r[3] / 2)
    for _ in range(6):
        h = rng.uniform(-math.pi, math.pi, 2)
        a = [*rng.uniform(-0.5, 0.5, 2), *rng.uniform(1.0, 4.0, 2), math.cos(h[0]), math.sin(h[0])]
        b = [*rng.uniform(-1.0, 1.0, 2), *rng.uniform(1.0, 4.0, 2), math.cos(h[1]), math.sin(h[1])]
        ia, ib = inside(a), inside(b)
        assert abs(float(X.inter_area(a, b)) - (ia & ib).sum() * cell) < 2e-2
        assert abs(float(X.bev_iou(a, b)) - (ia & ib).sum() / (ia | ib).sum()) < 2e-3


def test_exact_intersection_has_at_most_8_vertices():
    assert max(len(X.intersection(a, b)) for _, a, b in C.pairs()) <= 8


def test_restatement_equals_oracle_bit_for_bit(oracle):
    """The scalar float64 restatement is the oracle's computation: its vertex counts are the device's."""
    for _, a, b in C.pairs():
        assert X.bev_iou_f64(a, b) == oracle.bev_iou(_rec(a[:6]), _rec(b[:6]))


# ------------------------------------------------------------------------------------------------ error bound
def test_oracle_bev_iou_within_bound_of_exact(oracle):
    worst, nonzero_err = 0.0, 0
    for fam, a, b, e, bound, *_ in _exact():
        got = oracle.bev_iou(_rec(a[:6]), _rec(b[:6]))
        err = abs(Q(got) - e)
        assert err <= Q(bound), (fam, a, b, got, float(e), bound)
        worst = max(worst, float(err) / bound)
        nonzero_err += err > 0
    print(f"bev IoU: worst |oracle - exact| / bound = {worst:.4f} over {len(_exact())} pairs")
    assert nonzero_err > 100                   # the families exercise rounding, the check is not vacuous


def test_host_iou3d_within_bound_of_exact():
    ex = _exact()
    a = np.array([r[1] for r in ex])
    b = np.array([r[2] for r in ex])
    got = we.iou3d(a, b)
    ratios = []
    for (fam, ra, rb, _, _, e3, bound3), g in zip(ex, got):
        err = abs(Q(float(g)) - e3)
        assert err <= Q(bound3), (fam, ra, rb, float(g), float(e3), bound3)
        ratios.append(float(err) / bound3)
    print(f"3D IoU: worst |iou3d - exact| / bound = {max(ratios):.4f}")


def test_host_iou3d_straddles_like_exact():
    """Waymo thresholds: 3D IoU >= 0.7 (vehicle), >= 0.5 (other types) decides as exact, 1e-9 and 1e-6 either side."""
    for thr, d, a, b in C.straddlers():
        e = X.iou3d(a, b)
        assert X.passes(e, thr) == (d > 0)
        assert (we.iou3d(_rec(a), _rec(b))[0] >= thr) == (d > 0), (thr, d, a, b)


def test_disjoint_and_touching_give_zero(oracle):
    """Exact zero -> zero weight everywhere; exactly 0.0 unless a heading is a rounded random angle, where a touching
    pair may keep a sliver of order u R^2 (inside the bound)."""
    n_exact = 0
    for fam, a, b, e, bound, e3, bound3 in _exact():
        if e3 == 0:
            assert we.iou3d(_rec(a), _rec(b))[0] <= bound3
        if e != 0:
            continue
        got = oracle.bev_iou(_rec(a[:6]), _rec(b[:6]))
        assert got <= bound and int(got * 1e6) == 0
        assert we.iou3d(_rec(a), _rec(b))[0] <= bound
        if not any(r[4] == c and r[5] == s for r in (a, b) for h, c, s in C.HEADINGS if h.startswith("rand")):
            assert got == 0.0, (fam, a, b, got)
            assert we.iou3d(_rec(a), _rec(b))[0] == 0.0
            n_exact += 1
    assert n_exact > 150


# ------------------------------------------------------------------------------------------------ weights and decisions
def test_oracle_weights_and_decisions_equal_exact(oracle):
    """weight = int(iou * 1e6) equals floor(exact * 1e6) outside the band, either neighbour inside it; the 0.2
    decision of orc_bev_match (weight > 0) equals exact >= 0.2 outside the band."""
    for fam, a, b, e, bound, *_ in _exact():
        pa, pb = _rec(a[:6])[None], _rec(b[:6])[None]
        W = oracle.bev_match(pa, pb, 0.0, want_weights=True)[4]
        assert X.weight_band_ok(int(W[0, 0]), e, bound), (fam, a, b, int(W[0, 0]), float(e))
        if abs(float(e) - 0.2) > 2 * bound:
            W2 = oracle.bev_match(pa, pb, 0.2, want_weights=True)[4]
            assert (W2[0, 0] > 0) == X.passes(e, 0.2), (fam, a, b)
    for thr, d, a, b in C.straddlers():
        e, bound = X.bev_eval(a, b)
        assert X.passes(e, thr) == (d > 0)
        pa, pb = _rec(a[:6])[None], _rec(b[:6])[None]
        pm, gm, iou, total, W = oracle.bev_match(pa, pb, thr, want_weights=True)
        assert (W[0, 0] > 0) == (d > 0) and (pm[0] == 0) == (d > 0), (thr, d, a, b)
        assert W[0, 0] == 0 or X.weight_band_ok(int(W[0, 0]), e, bound)     # thr + 1e-6 lies on an integer weight


def test_weights_near_integers():
    """Pairs whose exact IoU lies just above and below k / 1e6: the quantised weight of the float64 IoU is floor(exact)
    whenever no integer lies within the band."""
    a = C.rec(0.5, -1.25, 4.5, 2.0, 1.0, 0.0)
    checked = 0
    for k in (200000, 500001, 699999, 700000, 999999):
        for d in (3e-12, -3e-12):
            b = C.straddle(a, k / 1e6, d, 0)
            e, bound = X.bev_eval(a, b)
            got = X.bev_iou_f64(a, b)
            assert X.weight_band_ok(int(got * 1e6), e, bound)
            if abs(e * X.KMAX - round(e * X.KMAX)) > Q(bound) * X.KMAX * 4:
                assert int(got * 1e6) == X.weight(e)
                checked += 1
    assert checked >= 6


# ------------------------------------------------------------------------------------------------ clip buffers
def test_vertex_counts_within_buffer_capacity():
    worst = 0
    for _, a, b in C.pairs():
        counts = []
        X.bev_inter_area_f64(a, b, counts)
        n = 4
        for k in counts:                        # the floor(1.5 n) argument of bev_iou.h
            assert k <= (3 * n) // 2
            n = k
        assert all(k <= X.DEVICE_STORED for k in counts[:3])
        worst = max([worst] + counts)
    for m, a, b in C.HIGH_VERTEX:
        counts = []
        X.bev_inter_area_f64(X.fromhex(a), X.fromhex(b), counts)
        assert max(counts) == m
        assert len(X.intersection(X.fromhex(a), X.fromhex(b))) <= 8
    print(f"largest clip vertex count: {worst}")
    assert 10 <= worst < X.CLIP_CAPACITY


def test_host_clip_area_equals_restatement_on_high_vertex_pairs(oracle):
    recs = [(X.fromhex(a), X.fromhex(b)) for _, a, b in C.HIGH_VERTEX] + [(a[:6], b[:6]) for _, a, b in C.pairs()]
    A, B = np.array([r[0] for r in recs]), np.array([r[1] for r in recs])
    got = we._clip_area(A, B)
    for (a, b), g in zip(recs, got):
        assert g == X.bev_inter_area_f64(a, b), (a, b)
    for (a, b) in recs[:len(C.HIGH_VERTEX)]:                                      # and the oracle's IoU from that area
        area_a, area_b = a[2] * a[3], b[2] * b[3]
        inter = X.bev_inter_area_f64(a, b)
        assert oracle.bev_iou(_rec(a), _rec(b)) == min(inter / ((area_a + area_b) - inter), 1.0)


def test_host_clip_area_reads_every_input_vertex():
    """A clip input of more than 8 vertices: the host reads all of them, like the device (seed pair: 8 entering the
    last clip, 10 leaving it; rows of the same call with fewer vertices do not change the result)."""
    m, a, b = C.HIGH_VERTEX[0]
    a, b = X.fromhex(a), X.fromhex(b)
    counts = []
    X.bev_inter_area_f64(a, b, counts)
    assert counts[-1] == m and max(counts[:-1]) >= 8
    sq = [0.0, 0.0, 2.0, 2.0, 1.0, 0.0]
    got = we._clip_area(np.array([a, sq, b]), np.array([b, sq, a]))
    assert got[0] == X.bev_inter_area_f64(a, b) and got[2] == X.bev_inter_area_f64(b, a) and got[1] == 4.0
