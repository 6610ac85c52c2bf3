"""CPU: the candidate formulation of the SAM3D fusion grid search (fusion.waymo_candidates, waymo_eval.pack_candidates,
waymo_eval.counts_sweep_host) against the per-alpha path it replaces -- fuse, encode, decode, pack, counts_host -- on the G11
fusion inputs and on a crafted set that holds the edge cases.  Match lists come from the CPU oracle's bev_match."""
import numpy as np

from cm3d_amd import waymo_eval as we
from tests import waymo_sweep_cases as cases


def _assert_sweep_equals_loop(inp, alphas):
    counts, hsum = we.counts_sweep_host(inp.packed_candidates(), alphas)
    assert counts.shape == (len(alphas), we.N_BREAKDOWNS, we.N_CUTOFFS, 4) and hsum.shape == counts.shape[:3]
    for a, alpha in enumerate(alphas):
        c, h = we.counts_host(inp.packed_at(alpha))
        assert np.array_equal(counts[a], c), f"counts differ at alpha {alpha}"
        assert np.array_equal(hsum[a], h), f"heading sums differ at alpha {alpha}"
    return counts, hsum


def test_g11_fusion_inputs_every_alpha():
    inp = cases.g11_inputs()
    alphas = cases.g11_alphas(inp)
    assert len(alphas) == len(cases.fixtures()["fusion"]["scores"])
    assert np.sum(inp.candidates()[1] == 1) > 100                          # the fixture's SAM3D boxes: scores move with alpha
    counts, _ = _assert_sweep_equals_loop(inp, alphas)
    assert any(not np.array_equal(counts[0], counts[a]) for a in range(1, len(alphas)))


def _frame_candidates(inp, key):
    objs, kind, p, s = inp.candidates()
    ids = [i for i, o in enumerate(objs) if (o["context_name"], o["timestamp_micros"]) == key]
    return [objs[i] for i in ids], kind[ids], p[ids], s[ids]


def test_crafted_set_holds_its_edge_cases():
    inp = cases.crafted_inputs()
    objs, kind, p, s = inp.candidates()
    n_pairs = sum(len(v) for v in inp.pm.values())
    assert n_pairs > 60 and np.sum(kind == 2) == n_pairs == np.sum(kind == 3)
    assert np.array_equal(np.flatnonzero(kind == 2) + 1, np.flatnonzero(kind == 3))        # a pair's candidates are neighbours
    pair = kind >= 2
    act0, act_hi = we.candidate_scores(kind, p, s, 0.0)[0], we.candidate_scores(kind, p, s, 1000.0)[0]
    assert act0[kind == 2].all() and not act0[kind == 3].any()             # alpha 0: no pair takes the SAM3D box
    assert act_hi[kind == 3].all() and not act_hi[kind == 2].any()         # alpha 1000: every pair does
    assert np.all(s[pair] > 0)
    # range: both pairs matched, their boxes in different range shards
    o, k, _, _ = _frame_candidates(inp, cases.SPECIAL["range"])
    assert list(k) == [2, 3, 2, 3]
    d = [float(np.linalg.norm(x["center"])) for x in o]
    assert d[0] < 30.0 <= d[1] and d[2] < 50.0 <= d[3]
    # scores: equality keeps the prediction, the product above 1 clips
    o, k, pp, ss = _frame_candidates(inp, cases.SPECIAL["scores"])
    assert list(k) == [2, 3, 2, 3] and ss[0] * 2.0 == pp[0] and ss[2] * 2.0 > 1.0
    act, sc = we.candidate_scores(k, pp, ss, 2.0)
    assert list(act) == [True, False, False, True] and sc[3] == np.float32(1.0)
    # tie: a zero SAM3D score, and an unmatched SAM3D box that meets an unmatched prediction's score at alpha 2
    o, k, pp, ss = _frame_candidates(inp, cases.SPECIAL["tie"])
    assert list(k) == [0, 1, 1] and ss[2] == 0.0
    act, sc = we.candidate_scores(k, pp, ss, 2.0)
    assert act.all() and sc[0] == sc[1] and o[0]["type"] == o[1]["type"]
    # type: the SAM3D box goes under the prediction's type
    o, k, _, _ = _frame_candidates(inp, cases.SPECIAL["type"])
    assert list(k) == [2, 3] and o[0]["type"] == o[1]["type"] == 2
    assert inp.ss[cases.SPECIAL["type"]][0]["type"] == 4
    # frames on one side only
    assert cases.SPECIAL["only_sam3d"] not in inp.pb and cases.SPECIAL["only_sam3d"] in inp.sb
    o, k, _, _ = _frame_candidates(inp, cases.SPECIAL["only_sam3d"])
    assert list(k) == [1]
    assert not _frame_candidates(inp, cases.SPECIAL["only_gt"])[0]
    assert any((g["context_name"], g["timestamp_micros"]) == cases.SPECIAL["only_gt"] for g in inp.gt)


def test_tied_scores_share_a_ground_truth_with_equal_weights():
    """The score tie is between two rows whose weights on the one ground-truth box are equal: which of them is matched is
    decided by the row order alone."""
    inp = cases.crafted_inputs()
    pc = inp.packed_candidates()
    full = dict(pred_off=pc["cand_off"], gt_off=pc["gt_off"], pred_box=pc["cand_box"], gt_box=pc["gt_box"], group_bd=pc["group_bd"])
    w, off = we.pair_weights(full)
    objs = inp.candidates()[0]
    hit = 0
    for g in range(pc["group_bd"].size):
        ids = pc["cand_index"][pc["cand_off"][g]:pc["cand_off"][g + 1]]
        rows = [r for r, i in enumerate(ids) if objs[i]["length"] == 1.125]
        if pc["group_bd"][g] == 4 and rows:                                 # the pedestrians' shard 0 of the tie frame
            G = int(pc["gt_off"][g + 1] - pc["gt_off"][g])
            m = w[off[g]:off[g + 1]].reshape(ids.size, G)[rows]
            assert m.shape[0] == 2 and m.max(1)[0] == m.max(1)[1] == 562500 and m.argmax(1)[0] == m.argmax(1)[1]
            hit += 1
    assert hit == 1


def test_crafted_set_every_alpha():
    inp = cases.crafted_inputs()
    counts, _ = _assert_sweep_equals_loop(inp, cases.CRAFTED_ALPHAS)
    assert not np.array_equal(counts[0], counts[-1])


def test_static_flag_marks_groups_of_unmatched_predictions_only():
    for inp in (cases.crafted_inputs(), cases.g11_inputs()):
        pc = inp.packed_candidates()
        co = pc["cand_off"]
        flags = pc["group_static"]
        assert flags.shape == (co.size - 1,)
        for g in range(flags.size):
            assert bool(flags[g]) == bool(np.all(pc["cand_kind"][co[g]:co[g + 1]] == 0))
        assert flags.any() and not flags.all()
        # a static group's counts cannot depend on alpha: its candidates are active with the same score at every alpha
        kinds = pc["cand_kind"]
        a0, s0 = we.candidate_scores(kinds, pc["cand_p"], pc["cand_s"], 0.3)
        a1, s1 = we.candidate_scores(kinds, pc["cand_p"], pc["cand_s"], 3.0)
        static_rows = np.repeat(flags.astype(bool), np.diff(co))
        assert a0[static_rows].all() and a1[static_rows].all() and np.array_equal(s0[static_rows], s1[static_rows])


def test_candidate_boxes_are_what_a_decode_of_the_fused_file_gives():
    inp = cases.crafted_inputs()
    objs, kind, p, s = inp.candidates()
    from cm3d_amd import fusion, waymo as wm
    for alpha in (0.0, 1000.0):
        fused = we.decode_objects(wm.encode_objects(fusion.fuse_waymo(*inp.sides(), alpha)))
        act, sc = we.candidate_scores(kind, p, s, alpha)
        chosen = [objs[i] for i in np.flatnonzero(act)]
        assert len(chosen) == len(fused)
        for c, f in zip(chosen, fused):
            for key in ("center", "length", "width", "height", "heading", "type", "context_name", "timestamp_micros"):
                assert c[key] == f[key], key
        assert np.array_equal(sc[act], np.array([f["score"] for f in fused], np.float32))
