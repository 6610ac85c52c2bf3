"""CPU: the cases of tests/assign_cases.py have the structure that tests/test_gpu_assign.py relies on -- conditions, not
measurements -- and the oracle's matching (oracle.bev_match, the sequential restatement of assign.h's solver) is a
maximum-weight assignment on every one of them, up to 1024 x 1024, by scipy's linear_sum_assignment."""
import numpy as np
import pytest

from tests import assign_cases as ac

BEV_RUNS = [("dense", 0.2), ("dense", 0.6), ("chain", 0.2), ("chain", 0.6), ("ties", 0.2), ("seams", 0.2)]     # as on the GPU


def _samples(oracle, family, thr=0.2):
    """(name, P, G, pred_match, W, total, optimum) of every sample of a family."""
    call, ref = ac.bev_call(family), ac.bev_reference(oracle, family, thr)
    for f, (P, G) in enumerate(call["sizes"]):
        yield (ac.sample_name(call, f), int(P), int(G), ref["pred_match"][call["pred_off"][f]:call["pred_off"][f + 1]],
               ref["W"][call["pair_off"][f]:call["pair_off"][f + 1]].reshape(P, G), int(ref["total"][f]), int(ref["optimum"][f]))


@pytest.mark.parametrize("family,thr", BEV_RUNS)
def test_oracle_total_is_the_optimum_below_2_30(oracle, family, thr):
    ref = ac.bev_reference(oracle, family, thr)
    bad = np.flatnonzero(ref["total"] != ref["optimum"])
    assert bad.size == 0, f"{family} at {thr}: sample {ac.sample_name(ac.bev_call(family), int(bad[0]))}: oracle {ref['total'][bad[0]]}, scipy {ref['optimum'][bad[0]]}"
    assert ref["total"].max() < 2 ** 30 and ref["total"].max() > 0
    if family != "seams":
        assert np.all(ref["total"] > 0)


def test_dense_bev_is_dense_and_matches_the_whole_smaller_side(oracle):
    sizes = set()
    for name, P, G, pm, W, total, _ in _samples(oracle, "dense"):
        assert np.mean(W > 0) >= 0.99, name
        assert np.sum(pm >= 0) == min(P, G), name
        assert np.unique(W[0]).size > 0.9 * G and np.unique(W[:, 0]).size > 0.9 * P, name      # generic: hardly any equal weights in a line
        sizes.add((P, G))
    assert sizes == set(ac.DENSE_SIZES + ac.BEV_LDS_SEAM)
    assert max(t for *_, t, _ in _samples(oracle, "dense")) > 800 * ac.KMAX            # the 32-bit state under load
    mixed = [np.mean(W > 0) for _, _, _, _, W, _, _ in _samples(oracle, "dense", 0.6)]
    assert 0.05 < min(mixed) and max(mixed) < 0.95                      # threshold 0.6: zero and non-zero costs mixed


def test_chain_bev_shifts_every_prediction(oracle):
    cases = [c for c in ac.bev_cases() if c["family"] == "chain"]
    assert [(c["n"], c["variant"]) for c in cases] == [(n, v) for n in ac.CHAIN_SIZES for v in ac.CHAIN_VARIANTS]
    for c, (name, P, G, pm, W, total, _) in zip(cases, _samples(oracle, "chain")):
        assert name == c["name"] and max(P, G) == c["n"]
        if c["rows"] == "gt":                                           # tall: the sides are swapped, rows are the ground truth
            part = np.full(G, -1)
            part[pm[pm >= 0]] = np.flatnonzero(pm >= 0)
            W = W.T
        else:
            part = pm
        assert np.array_equal(part, c["shifted"]), name                 # all rows matched, the chained ones to column i + 1
        chained = np.flatnonzero(c["shifted"] > 0)
        assert chained.size == c["n_chain"] >= c["n"] - 2
        strong, weak = W[chained, c["shifted"][chained] - 1], W[chained, c["shifted"][chained]]
        assert np.all(strong > weak) and np.all(weak > 200000), name    # a dual update at every step of the path
        assert np.sum(W > 0) == 2 * c["n_chain"] + 1, name              # two neighbours each, and the last prediction's one
    for name, P, G, pm, W, total, _ in _samples(oracle, "chain", 0.6):
        assert np.sum(W > 0) == 1 and np.sum(pm >= 0) == 1, name        # only the last prediction is above 0.6


def test_ties_bev_matrices_are_constant(oracle):
    sizes = []
    for name, P, G, pm, W, total, _ in _samples(oracle, "ties"):
        assert W.min() == W.max() == ac.KMAX, name
        assert total == min(P, G) * ac.KMAX
        sizes.append((P, G))
    assert sizes == ac.TIES_SIZES and {(1024, 1024), (1024, 1000), (257, 1024)} <= set(sizes)


def test_seams_blocks_span_many_groups():
    s = ac.bev_seams()
    sizes = s["sizes"]
    shared, empty_inside, most = ac.block_stats(ac.pair_offsets(sizes))
    assert shared >= 1000 and empty_inside >= 1 and most >= 100
    assert {tuple(x) for x in sizes[:ac.SEAM_TINY_BEFORE]} >= {(1, 1), (1, 2), (2, 1), (0, 1), (0, 3), (1, 0), (3, 0), (0, 0)}
    assert sizes[:ac.SEAM_TINY_BEFORE].max() <= 3 and (sizes[:, 0] * sizes[:, 1])[:ac.SEAM_TINY_BEFORE].max() == 2
    d = ac.SEAM_TINY_BEFORE
    assert [tuple(x) for x in sizes[d:d + len(ac.SEAM_DENSE)]] == ac.SEAM_DENSE and sizes.shape[0] - d - len(ac.SEAM_DENSE) == ac.SEAM_TINY_AFTER
    po = ac.pair_offsets(sizes)
    assert po[d + 1] // ac.BLOCK_PAIRS - po[d] // ac.BLOCK_PAIRS >= 300            # the (300, 300) group crosses hundreds of blocks
    # the Waymo call: the same structure
    packed = ac.waymo_packed("seams")
    wsizes = np.stack([np.diff(packed["pred_off"]), np.diff(packed["gt_off"])], 1)
    shared, empty_inside, most = ac.block_stats(ac.pair_offsets(wsizes))
    assert shared >= 1000 and empty_inside >= 100 and most >= 100
    assert (300, 300) in {tuple(x) for x in wsizes} and len(set(packed["group_bd"].tolist())) == 16


def test_seams_dense_groups_are_dense_and_tiny_groups_mixed(oracle):
    ref, call = ac.bev_reference(oracle, "seams", 0.2), ac.bev_call("seams")
    for f in range(ac.SEAM_TINY_BEFORE, ac.SEAM_TINY_BEFORE + len(ac.SEAM_DENSE)):
        assert np.mean(ref["W"][call["pair_off"][f]:call["pair_off"][f + 1]] > 0) >= 0.99
    tiny = np.concatenate([ref["W"][:call["pair_off"][ac.SEAM_TINY_BEFORE]], ref["W"][call["pair_off"][ac.SEAM_TINY_BEFORE + len(ac.SEAM_DENSE)]:]])
    assert 0.2 < np.mean(tiny > 0) < 0.8                                # matches and non-matches among the tiny groups


def test_every_instance_and_read_path_is_reached():
    bev = {fam: set() for fam in ac.FAMILIES}
    paths = set()
    for fam in ac.FAMILIES:
        for P, G in ac.bev_call(fam)["sizes"]:
            if P and G:
                bev[fam].add(ac.instance_of(P, G))
                if fam == "dense":
                    paths |= {frozenset(ac.bev_read_paths(P, G))}
    for fam in ac.FAMILIES:
        assert bev[fam] >= set(ac.INSTANCES), f"fusion, family {fam}: instances {sorted(bev[fam])}"
    assert paths >= {frozenset({"lds"}), frozenset({"l2"}), frozenset({"lds", "tr"}), frozenset({"l2", "tr"})}
    by = {tuple(s): ac.bev_read_paths(*s) for s in ac.BEV_LDS_SEAM}      # the seam itself: 8192 pairs in LDS, 8256 in L2
    assert by[(64, 128)] == {"lds"} and by[(128, 64)] == {"lds", "tr"} and by[(64, 129)] == {"l2"} and by[(129, 64)] == {"l2", "tr"}
    wm_paths = set()
    for fam in ac.FAMILIES:
        packed = ac.waymo_packed(fam)
        P, G = np.diff(packed["pred_off"]), np.diff(packed["gt_off"])
        live = (P > 0) & (G > 0)
        got = {ac.instance_of(p, g) for p, g in zip(P[live], G[live])}
        assert got >= set(ac.INSTANCES), f"waymo metrics, family {fam}: instances {sorted(got)}"
        if fam == "dense":
            wm_paths = {(int(p), int(g)): ac.wm_read_path(p, g) for p, g in zip(P[live], G[live])}
    assert wm_paths[(64, 64)] == "lds" and wm_paths[(65, 63)] == "lds" and wm_paths[(65, 64)] == "l2"


# ---------------------------------------------------------------------------------------------------- Waymo form
def _group_weights(packed, g):
    from cm3d_amd import waymo_eval as we
    p0, p1, g0, g1 = (int(packed[k][g + d]) for k in ("pred_off", "gt_off") for d in (0, 1))
    ii, jj = np.meshgrid(np.arange(p1 - p0), np.arange(g1 - g0), indexing="ij")
    iou = we.iou3d(packed["pred_box"][p0 + ii.ravel()], packed["gt_box"][g0 + jj.ravel()]).reshape(p1 - p0, g1 - g0)
    return np.where(iou >= we.IOU_THR[int(packed["group_bd"][g]) // 4 + 1], (iou * we.IOU_KMAX).astype(np.int64), 0)


@pytest.mark.parametrize("family", ac.FAMILIES)
def test_waymo_host_counts_do_not_depend_on_the_column_order(family):
    """counts_host takes scipy's choice among equal totals; were there an exact tie in total weight between assignments of
    different TP or heading sum, reversing the ground truth of every group would be likely to show it.  (The first seed
    of the dense family, 711, failed this at breakdown 5, cutoff 24; its second, 721, passes.  The others passed as chosen.)"""
    from cm3d_amd import waymo_eval as we
    hc, hh = ac.waymo_reference(family)
    rc, rh = we.counts_host(ac.reversed_gt(ac.waymo_packed(family)), ac.reversed_weights(ac.waymo_packed(family), ac.waymo_weights(family)))
    assert np.array_equal(hc, rc) and np.array_equal(hh, rh)
    assert hc[:, 0, 0].sum() > 0


def test_waymo_dense_groups_and_score_levels():
    packed = ac.waymo_packed("dense")
    _, _, _, frames = ac.waymo_family("dense")
    assert [(f["P"], f["G"]) for f in frames] == ac.WM_DENSE_SIZES and {f["type"] for f in frames} == {1, 2, 4}
    P, G = np.diff(packed["pred_off"]), np.diff(packed["gt_off"])
    assert P.size == 3 * len(frames)                                    # every frame: its type's shard 0 and two range shards
    from scipy.optimize import linear_sum_assignment
    w, pair_off = ac.waymo_weights("dense")
    for g in range(P.size):
        W = w[pair_off[g]:pair_off[g + 1]].reshape(P[g], G[g])
        assert np.mean(W > 0) >= 0.5, (g, P[g], G[g])
        r, c = linear_sum_assignment(W, maximize=True)
        assert np.sum(W[r, c] > 0) == min(P[g], G[g]), (g, P[g], G[g])      # the whole smaller side is matched, in every group
        assert min(P[g], G[g]) * ac.KMAX < 2 ** 30
        if max(P[g], G[g]) > ac.WM_MANY_LEVELS:                         # one scipy solve per level on the host
            assert np.unique(packed["pred_score"][packed["pred_off"][g]:packed["pred_off"][g + 1]]).size <= 5
    hc, _ = ac.waymo_reference("dense")
    for bd in range(16):                                                # and so counted: TP with every prediction admitted
        assert hc[bd, 0, 0] == sum(min(p, g) for p, g, b in zip(P, G, packed["group_bd"]) if b == bd), bd


def test_waymo_chain_reroutes_at_the_last_predictions_cutoff():
    """Per chain frame (packed alone): at the last cutoff that admits the last prediction every admitted prediction is
    matched, the chained ones to ground truth i + 1; one cutoff higher they sit on ground truth i.  TP moves from n to
    n - 1 and the heading sums are those of the shifted and of the unshifted matching, which differ."""
    from cm3d_amd import waymo_eval as we
    pred, gt, n_frames, frames = ac.waymo_family("chain")
    assert [(f["n"], f["variant"]) for f in frames] == [(n, v) for n in ac.CHAIN_SIZES for v in ac.CHAIN_VARIANTS]
    for f in frames:
        pm, gm = pred["frame"] == f["frame"], gt["frame"] == f["frame"]
        one = we.pack_arrays({k: v[pm] for k, v in pred.items()}, {k: v[gm] for k, v in gt.items()}, n_frames)
        hc, hh = we.counts_host(one)
        bd = (f["type"] - 1) * 4
        assert one["group_bd"][0] == bd and one["pred_off"][1] == f["P"] and one["gt_off"][1] == f["G"]      # group 0: shard 0
        last = 64 if f["variant"] == "mid" else 10                      # the last cutoff that admits the last prediction
        k = we._cutoff_counts(one["pred_score"][:f["P"]])
        W = _group_weights(one, 0)
        li = int(W[:, 0].argmax())                                      # the last prediction's row: it sits on ground truth 0
        assert k[last + 1] <= li < k[last] and W[li, 0] > 800000, f["name"]
        assert np.count_nonzero(W) == 2 * (f["P"] - 1) + 1 - (f["variant"] == "tall"), f["name"]
        head = lambda rows, cols: int(we.heading_accuracy_fixed(one["pred_head"][rows], one["gt_head"][cols]).sum())
        chained = np.array([r for r in range(k[last]) if r != li])      # chained prediction c is row c, or c + 1 behind the last one
        c = chained - (chained > li)
        fits = c + 1 < f["G"]                                           # tall: the end of the chain goes to a padded column
        shifted = head(chained[fits], c[fits] + 1) + head([li], [0])
        unshifted = head(chained, c)
        assert shifted != unshifted + head([li], [0]) and abs(shifted - unshifted) > 30 * 2 ** 32, f["name"]
        tp, tp_next = int(hc[bd, last, 0]), int(hc[bd, last + 1, 0])
        assert tp == int(fits.sum()) + 1 == min(k[last], f["G"]) and int(hh[bd, last]) == shifted, f["name"]
        before = np.arange(k[last + 1])                                 # one cutoff higher: rows before the last prediction, unshifted
        assert tp_next == k[last + 1] and int(hh[bd, last + 1]) == head(before, before), f["name"]
        if f["variant"] in ("square", "wide"):
            assert (tp, tp_next) == (f["P"], f["P"] - 1), f["name"]
        if f["variant"] == "tall":
            assert tp == tp_next == f["G"] == f["n"] - 1, f["name"]     # TP cannot rise: only the heading sum shows the re-route


def test_waymo_ties_are_constant_and_leave_the_counts_unique():
    packed = ac.waymo_packed("ties")
    P, G = np.diff(packed["pred_off"]), np.diff(packed["gt_off"])
    assert {(int(p), int(g)) for p, g in zip(P, G)} == set(ac.WM_TIES_SIZES)
    w, pair_off = ac.waymo_weights("ties")
    assert pair_off[-1] == np.sum(P * G) and w.min() == w.max() == ac.KMAX
    # any maximum assignment gives the same counts only if headings and levels do not tell the boxes apart
    assert np.unique(packed["gt_head"]).size == 1 and np.unique(packed["pred_head"]).size == 1 and np.all(packed["gt_level"] == 1)
