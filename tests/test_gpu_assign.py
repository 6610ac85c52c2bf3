"""GPU: the shared one-wave assignment solver (cm3d_amd/csrc/assign.h) on the cases of tests/assign_cases.py -- dense
matrices, one augmenting path through every column, constant matrices at the widest instance, thousands of groups per
weight block -- through its two products: cm3d_bev_match against the oracle (bit for bit) and, independently of the
oracle's solver, against scipy's optimum; cm3d_waymo_metrics against waymo_eval.counts_host and against a fresh solve per
cutoff.  tests/test_assign_cases_host.py proves on the CPU that the cases have the structure they are named for."""
import numpy as np
import pytest

from tests import assign_cases as ac

pytestmark = pytest.mark.gpu


def _device_match(call, thr):
    """One cm3d_bev_match call -> pred_match and match_iou of all predictions, like the oracle's."""
    from cm3d_amd import ops
    po = call["pred_off"]
    got = ops.bev_match_records(np.split(call["pred_rec"], po[1:-1]), np.split(call["gt_rec"], call["gt_off"][1:-1]), thr)
    assert len(got) == call["sizes"].shape[0]
    n = np.array([g[0].size for g in got])
    at = np.repeat(po[:-1], n) + np.concatenate([g[0] for g in got])
    pm, iou = np.full(int(po[-1]), -1, np.int32), np.zeros(int(po[-1]))
    pm[at], iou[at] = np.concatenate([g[1] for g in got]), np.concatenate([g[2] for g in got])
    return pm, iou


def _describe(call, ref, thr, dev_pm, dev_iou, row):
    """Failure text for global prediction index `row`."""
    f = int(np.searchsorted(call["pred_off"], row, "right") - 1)
    P, G = (int(x) for x in call["sizes"][f])
    i = row - int(call["pred_off"][f])
    W = ref["W"][call["pair_off"][f]:call["pair_off"][f + 1]].reshape(P, G)
    d, o = int(dev_pm[row]), int(ref["pred_match"][row])

    def w(j):
        return int(W[i, j]) if j >= 0 else None
    return (f"family {call['family']}, sample {ac.sample_name(call, f)} (P, G) = ({P}, {G}), threshold {thr}: first difference at "
            f"prediction {i}: device partner {d} (weight {w(d)}, IoU {dev_iou[row]!r}), oracle partner {o} (weight {w(o)}, "
            f"IoU {ref['match_iou'][row]!r}); device total of the sample "
            f"{int(sum(W[k, dev_pm[call['pred_off'][f] + k]] for k in range(P) if dev_pm[call['pred_off'][f] + k] >= 0))}, "
            f"oracle {int(ref['total'][f])}, optimum {int(ref['optimum'][f])}")


@pytest.mark.parametrize("family,thr", [("dense", 0.2), ("dense", 0.6), ("chain", 0.2), ("chain", 0.6), ("ties", 0.2), ("seams", 0.2)])
def test_fusion_equals_oracle_and_optimum(oracle, family, thr):
    """One cm3d_bev_match call per family.  Threshold 0.6 zeroes part of the dense matrices (mixed zero and non-zero costs)
    and all of a chain but its last prediction.
    The host reference (oracle and scipy, shared with the CPU tests) takes 0.3 - 7 s a case."""
    call = ac.bev_call(family)
    ref = ac.bev_reference(oracle, family, thr)
    pm, iou = _device_match(call, thr)
    # the oracle's steps: partners and IoUs bit for bit
    bad = np.flatnonzero((pm != ref["pred_match"]) | (iou != ref["match_iou"]))
    assert bad.size == 0, _describe(call, ref, thr, pm, iou, int(bad[0]))
    # independently of the oracle's solver: one to one, positive weights, scipy's optimum on the oracle's weights
    rows = np.flatnonzero(pm >= 0)
    f = np.searchsorted(call["pred_off"], rows, "right") - 1
    col = call["gt_off"][f] + pm[rows]
    assert np.all((pm[rows] < call["sizes"][f, 1])), _describe(call, ref, thr, pm, iou, int(rows[np.argmax(pm[rows] >= call["sizes"][f, 1])]))
    uniq, first, cnt = np.unique(col, return_index=True, return_counts=True)
    assert uniq.size == col.size, "two predictions share a partner: " + _describe(call, ref, thr, pm, iou, int(rows[first[np.argmax(cnt > 1)]]))
    w = ref["W"][call["pair_off"][f] + (rows - call["pred_off"][f]) * call["sizes"][f, 1] + pm[rows]]
    assert np.all(w > 0), "a matched pair below the threshold: " + _describe(call, ref, thr, pm, iou, int(rows[np.argmax(w <= 0)]))
    total = np.zeros(call["sizes"].shape[0], np.int64)
    np.add.at(total, f, w)
    short = np.flatnonzero(total != ref["optimum"])
    assert short.size == 0, "not a maximum-weight assignment: " + _describe(call, ref, thr, pm, iou, int(call["pred_off"][short[0]]))
    assert rows.size > 0


def _first_count_difference(family, what, a, b, ha, hb):
    d = np.argwhere(a != b)
    if d.size:
        bd, c, k = (int(x) for x in d[0])
        return (f"family {family}, {what}: breakdown {bd} (type {bd // 4 + 1}, shard {bd % 4}), cutoff {c}, count "
                f"{('TP', 'FP', 'FN L1', 'FN L2')[k]}: {int(a[bd, c, k])} against {int(b[bd, c, k])}")
    bd, c = (int(x) for x in np.argwhere(ha != hb)[0])
    return (f"family {family}, {what}: breakdown {bd} (type {bd // 4 + 1}, shard {bd % 4}), cutoff {c}, heading sum "
            f"{int(ha[bd, c])} against {int(hb[bd, c])} (TP {int(a[bd, c, 0])})")


@pytest.mark.parametrize("family", ac.FAMILIES)
def test_waymo_counts_equal_host_and_every_cutoff(family):
    """cm3d_waymo_metrics on a family: one solve per group serves all 101 cutoffs (the chains re-route every earlier row at
    a late or an interior cutoff), equal to scipy per prediction subset on the host and to a fresh device solve per cutoff.
    The host reference (counts_host on cached pair weights) takes 1 - 3 s a case, its weights 1 - 17 s (dense: two
    million pairs clipped in numpy)."""
    from cm3d_amd import ops
    packed = ac.waymo_packed(family)
    hc, hh = ac.waymo_reference(family)
    c, h = ops.waymo_metrics(packed)
    assert np.array_equal(c, hc) and np.array_equal(h, hh), _first_count_difference(family, "device against host", c, hc, h, hh)
    pc, ph = ops.waymo_metrics(packed, per_cutoff=True)
    assert np.array_equal(pc, hc) and np.array_equal(ph, hh), _first_count_difference(family, "device per cutoff against host", pc, hc, ph, hh)
    assert np.array_equal(c, pc) and np.array_equal(h, ph)
    assert c[:, 0, 0].sum() > 0
