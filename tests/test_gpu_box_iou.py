"""GPU: the rotated-box IoU of bev_iou.h, seen through cm3d_bev_match (bird's-eye view, fusion) and cm3d_waymo_metrics
(3D, Waymo evaluator), against exact rational geometry (tests/box_iou_exact.py) on the families of tests/iou_cases.py:
IoUs bit for bit equal to the oracle and within the error bound of exact, matches and threshold decisions as exact
decides them, score cutoffs as numpy decides them."""
import functools
import math
from fractions import Fraction as Q

import numpy as np
import pytest

from cm3d_amd import ops, waymo_eval as we
from tests import box_iou_exact as X
from tests import iou_cases as C

pytestmark = pytest.mark.gpu


def _boxes7(r):
    """Record -> the (7,) box of ops.bev_match: cx, cy, bottom z, length, width, height, heading."""
    return [r[0], r[1], 0.0, r[2], r[3], 1.0, math.atan2(r[5], r[4])]


@functools.lru_cache(None)
def _f32_samples():
    """Family pairs and random pairs at three offsets as ops.bev_match boxes, with the records actually sent."""
    rng = np.random.default_rng(31)
    pb = [_boxes7(a) for _, a, b in C.pairs()]
    gb = [_boxes7(b) for _, a, b in C.pairs()]
    for off in C.OFFSETS:
        for scale in (0.1, 1.0, 10.0):
            n = 300
            c = rng.uniform(-1, 1, (n, 2)) * scale + [off, -off]
            size = rng.uniform(0.3, 5.0, (n, 2, 2)) * scale
            d = rng.uniform(-3, 3, (n, 2)) * scale
            h = rng.uniform(-4, 4, (n, 2))
            for i in range(n):
                pb.append([c[i, 0], c[i, 1], 0.0, size[i, 0, 0], size[i, 0, 1], 1.0, h[i, 0]])
                gb.append([c[i, 0] + d[i, 0], c[i, 1] + d[i, 1], 0.0, size[i, 1, 0], size[i, 1, 1], 1.0, h[i, 1]])
    pr, gr = ops.match_records(np.array(pb)), ops.match_records(np.array(gb))
    return np.array(pb), np.array(gb), pr, gr, [X.bev_eval(a, b) for a, b in zip(pr, gr)]


def _check_returned(res, pr, gr, ex, oracle, thr):
    """Every sample is a 1 x 1 matching: the returned IoU equals the oracle's and lies within the bound of exact; a pair
    is returned iff its weight int(iou * 1e6) is positive and iou >= thr, which exact decides outside the band."""
    n_ret = 0
    for i, ((ids, gids, ious), (e, bound)) in enumerate(zip(res, ex)):
        orc = oracle.bev_iou(pr[i], gr[i])
        if ids.size:
            n_ret += 1
            assert ids.tolist() == [0] and gids.tolist() == [0]
            assert ious[0] == orc, (i, pr[i], gr[i])
            assert abs(Q(float(ious[0])) - e) <= Q(bound), (i, pr[i], gr[i], float(e))
            assert e >= Q(max(thr, 1e-6)) - Q(bound)
        else:
            assert e < Q(max(thr, 1e-6)) + Q(bound), (i, pr[i], gr[i], float(e))
            assert orc < thr or int(orc * 1e6) == 0
    return n_ret


def test_bev_match_as_batched_iou_float32_records(oracle):
    """Thousands of 1 x 1 samples through ops.bev_match at iou=1e-6 (records rounded through float32 on the way in,
    exact values of the records actually sent)."""
    pb, gb, pr, gr, ex = _f32_samples()
    res = ops.bev_match([p[None] for p in pb], [g[None] for g in gb], iou=1e-6)
    assert len(res) == len(pr) > 3000
    n_ret = _check_returned(res, pr, gr, ex, oracle, 1e-6)
    assert 1000 < n_ret < len(pr)


def test_bev_match_float64_records_and_straddlers(oracle):
    """Float64 records passed unrounded (cm3d_bev_match's own input): the high-vertex pairs, every family, and pairs
    whose exact IoU lies 1e-9 and 1e-6 either side of 0.2, at iou=1e-6 and at the fusion threshold 0.2."""
    recs = [(X.fromhex(a), X.fromhex(b)) for _, a, b in C.HIGH_VERTEX] + [(a[:6], b[:6]) for _, a, b in C.pairs()]
    strad = [(a[:6], b[:6], d) for thr, d, a, b in C.straddlers() if thr == 0.2]
    recs += [(a, b) for a, b, _ in strad]
    pr, gr = [np.array(a, np.float64) for a, _ in recs], [np.array(b, np.float64) for _, b in recs]
    ex = [X.bev_eval(a, b) for a, b in recs]
    for thr in (1e-6, 0.2):
        res = ops.bev_match_records([p[None] for p in pr], [g[None] for g in gr], iou=thr)
        _check_returned(res, pr, gr, ex, oracle, thr)
        for (ids, _, _), (a, b, d) in zip(res[len(recs) - len(strad):], strad):
            assert bool(ids.size) == (d > 0 or thr < 0.2), (a, b, d)
    for (ids, _, ious), (m, _, _) in zip(res, C.HIGH_VERTEX):             # identical up to ulps: matched, IoU ~ 1
        assert ids.size and abs(ious[0] - 1.0) < 1e-12


def _waymo_arrays(pairs, types, score=0.5):
    """One prediction and one ground-truth box per frame (pack_arrays layout).  pairs: (a, b) records; types: one each."""
    n = len(pairs)
    pa = np.array([a for a, _ in pairs], np.float64)
    ga = np.array([b for _, b in pairs], np.float64)
    typ = np.asarray(types, np.int32)

    def side(r):
        return dict(box=r, head=np.arctan2(r[:, 5], r[:, 4]).astype(np.float32), type=typ,
                    dist=np.sqrt(r[:, 0] ** 2 + r[:, 1] ** 2 + r[:, 6] ** 2), frame=np.arange(n))
    pred, gt = side(pa), side(ga)
    pred["score"] = np.broadcast_to(np.asarray(score, np.float32), (n,)).copy()
    gt["level"] = (1 + np.arange(n) % 2).astype(np.int32)
    return we.pack_arrays(pred, gt, n)


def test_waymo_metrics_threshold_straddlers():
    """Vehicle pairs straddle 0.7, pedestrian and cyclist pairs 0.5, by 1e-9 and 1e-6; the populations above and below
    run as separate calls so that flips cannot cancel.  TP / FN at cutoff 0 equal the exact counts; every count and
    heading sum equals counts_host."""
    by_side = {True: [], False: []}
    for thr, d, a, b in C.straddlers():
        if thr == 0.7:
            by_side[d > 0].append(((a, b), 1))
        elif thr == 0.5:
            by_side[d > 0].append(((a, b), 2))
            by_side[d > 0].append(((a, b), 4))
    for above, items in by_side.items():
        pairs, types = [p for p, _ in items], [t for _, t in items]
        packed = _waymo_arrays(pairs, types)
        counts, hsum = ops.waymo_metrics(packed)
        hc, hh = we.counts_host(packed)
        assert np.array_equal(counts, hc) and np.array_equal(hsum, hh)
        lvl = 1 + np.arange(len(pairs)) % 2
        for t in (1, 2, 4):
            sel = np.array(types) == t
            tp = sum(X.passes(X.iou3d(a, b), we.IOU_THR[t]) for (a, b), s in zip(pairs, sel) if s)
            assert tp == (int(sel.sum()) if above else 0)
            bd = (t - 1) * 4
            assert counts[bd, 0, 0] == tp and counts[bd, 0, 1] == int(sel.sum()) - tp
            assert counts[bd, 0, 3] == int(sel.sum()) - tp
            assert counts[bd, 0, 2] == (int(np.sum(sel & (lvl == 1))) if not above else 0)


def test_waymo_metrics_score_cutoffs():
    """Prediction scores float32(c * 0.01) exactly and one float32 ulp either side, for all 101 cutoffs: the device's
    TP and FP per cutoff equal numpy's score >= cutoff."""
    cut = we.CUTOFFS
    scores = np.concatenate([cut, np.nextafter(cut, np.float32(-1)), np.nextafter(cut, np.float32(2))]).astype(np.float32)
    n = scores.size
    matched = np.arange(n) % 2 == 0                 # every other prediction lies on its ground truth, the rest far away
    a = C.rec(20.0, 5.0, 4.5, 2.0, 1.0, 0.0)
    far = C.rec(20.0, 15.0, 4.5, 2.0, 1.0, 0.0)
    pairs = [(a, a if m else far) for m in matched]
    packed = _waymo_arrays(pairs, [1] * n, score=scores)
    counts, hsum = ops.waymo_metrics(packed)
    ge = scores[None, :] >= cut[:, None]            # (101, n)
    assert np.array_equal(counts[0, :, 0], (ge & matched).sum(1))
    assert np.array_equal(counts[0, :, 1], (ge & ~matched).sum(1))
    hc, hh = we.counts_host(packed)
    assert np.array_equal(counts, hc) and np.array_equal(hsum, hh)
