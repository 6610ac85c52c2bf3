"""CPU: the host statement of the point ownership (cm3d_amd.pointowner.point_owner_host) against the brute-force statement of
tests/point_owner_cases.py -- per frame, a dictionary from point to its claimants and the pairwise rule -- on the crafted cases and on
200 seeded random batches; both rules are strict total orders on every frame of the cases; the flags of the entry points and their
errors; the rows of the painted cloud."""
import argparse

import numpy as np
import pytest

from cm3d_amd import pointowner as po
from tests import point_owner_cases as pc

CRAFTED = pc.crafted()
IDS = [c["name"] for c in CRAFTED]


@pytest.fixture(scope="module")
def random_batches():
    return pc.random_cases()


@pytest.mark.parametrize("case", CRAFTED, ids=IDS)
def test_host_statement_equals_brute_force_on_the_crafted_cases(case):
    for rule, min_keep in case["runs"]:
        pc.assert_same(pc.host(case, rule, min_keep), pc.brute(case, rule, min_keep), (case["name"], rule, min_keep))


def test_host_statement_equals_brute_force_on_random_batches(random_batches):
    assert len(random_batches) == 200
    contested = 0
    for case in random_batches:
        F = len(case["mask_off"]) - 1
        assert 1 <= F <= 4 and case["P"] <= 500 and np.diff(case["mask_off"]).max() <= 40
        for m in range(len(case["score"])):
            assert (np.diff(case["hit_idx"][case["hit_off"][m]:case["hit_off"][m + 1]]) > 0).all()          # ascending subsets
        (rule, min_keep), = case["runs"]
        exp = pc.brute(case, rule, min_keep)
        pc.assert_same(pc.host(case, rule, min_keep), exp, (case["name"], rule, min_keep))
        contested += sum(len(c) > 1 for c in exp["claims"].values())
    assert contested > 10000                    # (the batches do contest points)


@pytest.mark.parametrize("case", CRAFTED, ids=IDS)
@pytest.mark.parametrize("rule", po.RULES)
def test_the_rules_are_strict_total_orders(case, rule):
    """Any two different masks: exactly one beats the other; no mask beats itself; and the numbers of masks beaten within a frame are
    0 .. n - 1, each once, which a tournament has only when it is transitive."""
    lists = pc.clamp_lists(case["hit_off"], len(case["hit_idx"]))
    n, s = [hi - lo for lo, hi in lists], case["score"]
    for f in range(len(case["mask_off"]) - 1):
        ms = range(int(case["mask_off"][f]), int(case["mask_off"][f + 1]))
        beaten = []
        for a in ms:
            assert not pc.beats(rule, s[a], n[a], a, s[a], n[a], a)
            w = [pc.beats(rule, s[a], n[a], a, s[b], n[b], b) for b in ms]
            assert all(w[b - ms[0]] != pc.beats(rule, s[b], n[b], b, s[a], n[a], a) for b in ms if b != a)
            beaten.append(sum(w))
        assert sorted(beaten) == list(range(len(ms)))
        if len(ms):
            assert np.array_equal(po.frame_ranks(s, n, ms[0], ms[-1] + 1, rule), beaten)


def test_statuses_and_conditions_of_the_crafted_cases():
    """What the cases are there for does happen in them."""
    by = {c["name"]: c for c in CRAFTED}
    for n in pc.SEAM_SIZES:
        a, b = pc.host(by[f"seam_{n}"], "score", 1), pc.host(by[f"seam_{n}"], "smallest", 1)
        assert a["ow_status"].tolist() == [1, 0] and a["ow_lost"].tolist() == [0, 0] and (a["ow_owner"] == 1).all()
        if n == 1:                              # (A is B: equal lengths, the score decides under both rules)
            assert np.array_equal(a["ow_owner"], b["ow_owner"])
            continue
        assert not np.array_equal(a["ow_owner"], b["ow_owner"])                    # the rules disagree
        assert b["ow_lost"].tolist() == [0, (n + 1) // 2] and b["ow_status"].tolist() == [0, 0]
    r = pc.host(by["min_keep_kept_4"], "score", 5)
    assert r["ow_status"].tolist() == [1, 0] and r["ow_lost"].tolist() == [0, 0] and (r["ow_owner"][4:11] == 1).all()
    r = pc.host(by["min_keep_kept_5"], "score", 5)
    assert r["ow_status"].tolist() == [0, 0] and r["ow_lost"].tolist() == [7, 0]
    r = pc.host(by["min_keep_1_wholly_owned"], "score", 1)
    assert r["ow_status"].tolist() == [1, 0] and int(r["ow_off"][1]) == 6 and (r["ow_owner"][:6] == 1).all()
    r = pc.host(by["same_point_in_two_frames"], "score", 1)
    assert r["ow_owner"].tolist() == [0, 0, 0, 0, 0, 1, 2, 2, 3, 3, 3]
    r = pc.host(by["outside_the_frame"], "score", 1)
    assert r["ow_owner"].tolist() == [0, 0, 0, 0, 1, 1, 0, 1, 1, 2, 2, 2] and not r["ow_lost"][2]
    r = pc.host(by["two_nan_scores"], "score", 1)
    assert r["ow_owner"].tolist() == [0, 1, 1, 1, 1, 1, 1, 0, 1, 1, 3, 3, 3]      # equal NaNs: the shorter list, then the lower index
    r = pc.host(by["claimants_1024"], "score", 1)
    assert r["ow_owner"][:4].tolist() == [0, 8, 8, 8] and (r["ow_status"] == 0).all()      # (8: the first mask of the highest score)


def test_offsets_are_clamped_as_the_header_states():
    case = pc.claimant_cases()[1]
    n = len(case["hit_idx"])
    for cap in (n - 1, n // 2 + 1, 3):
        pc.assert_same(pc.host(case, "score", 2, cap), pc.brute(case, "score", 2, cap), cap)
        assert int(pc.host(case, "score", 2, cap)["ow_off"][-1]) <= cap
    off = case["hit_off"].copy()
    off[0], off[-3:] = -7, [n + 5, 2 ** 31 - 1, 2 ** 31 - 1]
    pc.assert_same(pc.host(case, "smallest", 1, n - 2, off), pc.brute(case, "smallest", 1, n - 2, off), "wild offsets")


def _parser():
    ap = argparse.ArgumentParser()
    po.add_arguments(ap)
    return ap


def test_flags():
    ap = _parser()
    assert po.from_namespace(ap.parse_args([]), ap) is None
    assert po.from_namespace(ap.parse_args(["--point-owner", "off"]), ap) is None
    o = po.from_namespace(ap.parse_args(["--point-owner", "score"]), ap)
    assert (o.rule, o.min_keep, o.code) == ("score", 5, 0) and (po.DEFAULT_RULE, po.DEFAULT_MIN_KEEP) == ("score", 5)
    o = po.from_namespace(ap.parse_args(["--point-owner", "smallest", "--point-owner-min-keep", "2", "--point-labels", "x"]), ap)
    assert (o.rule, o.min_keep, o.code) == ("smallest", 2, 1) and o.params() == dict(rule="smallest", min_keep=2)
    assert po.PointOwner() == po.PointOwner("score", 5)


@pytest.mark.parametrize("argv, message", [
    (["--point-owner-min-keep", "3"], "--point-owner-min-keep needs --point-owner"),
    (["--point-owner", "off", "--point-labels", "d"], "--point-labels needs --point-owner"),
    (["--point-owner", "score", "--point-owner-min-keep", "0"], "min_keep"),
])
def test_flag_errors_exit_2(argv, message, capsys):
    ap = _parser()
    with pytest.raises(SystemExit) as e:
        po.from_namespace(ap.parse_args(argv), ap)
    assert e.value.code == 2 and message in capsys.readouterr().err
    with pytest.raises(ValueError, match=message):
        po.from_namespace(ap.parse_args(argv))
    with pytest.raises(SystemExit):
        ap.parse_args(["--point-owner", "largest"])


def test_switch_errors():
    for kw in (dict(rule="area"), dict(rule=0), dict(min_keep=0), dict(min_keep=2.5)):
        with pytest.raises(ValueError):
            po.PointOwner(**kw)


def test_label_rows(random_batches):
    """Every listed (frame, idx) appears exactly once, ascending, with its owner's fields, and `claims` is the brute-force count."""
    for case in random_batches[:60] + [c for c in CRAFTED if c["name"] in ("claimants_65", "outside_the_frame", "same_point_in_two_frames")]:
        rule, min_keep = case["runs"][0]
        exp, res = pc.brute(case, rule, min_keep), pc.host(case, rule, min_keep)
        M = len(case["score"])
        rng = np.random.default_rng(M)
        cam, cls, flags = rng.integers(0, 6, M).astype(np.int32), rng.integers(0, 10, M).astype(np.int32), rng.integers(0, 8, M).astype(np.int32)
        seen = 0
        for f in range(len(case["mask_off"]) - 1):
            rows = po.label_rows(f, case["hit_idx"], case["hit_xyz"], case["hit_off"], case["mask_off"], res["ow_owner"], cam, cls, case["score"],
                                 flags, case["P"])
            assert tuple(rows) == po.LABEL_FIELDS
            want = sorted(p for (g, p) in exp["claims"] if g == f)
            assert rows["idx"].tolist() == want and rows["idx"].dtype == np.int32
            seen += len(want)
            m0 = int(case["mask_off"][f])
            for r in range(len(want)):
                c = exp["claims"][f, want[r]]
                assert rows["claims"][r] == min(len(c), 255)
                own = m0 + int(rows["mask"][r])
                assert own in c and all(own == b or pc.beats(rule, case["score"][own], *_n(case, own), case["score"][b], *_n(case, b)) for b in c)
                assert (rows["cam"][r], rows["class_id"][r], rows["kept"][r]) == (cam[own], cls[own], int((flags[own] & 3) == 3))
                assert rows["score"][r].tobytes() == np.float32(case["score"][own]).tobytes()
                assert rows["xyz"][r, 0] == np.float32(want[r]) and rows["xyz"][r, 1] == np.float32(own)       # the owner's own row
            assert rows["xyz"].dtype == np.float32 and rows["xyz"].shape == (len(want), 3) and rows["kept"].dtype == np.uint8
            assert rows["claims"].dtype == np.uint8
        assert seen == len(exp["claims"])
    many = [c for c in CRAFTED if c["name"] == "claimants_1024"][0]
    res = pc.host(many, "score", 1)
    z = np.zeros(1024, np.int32)
    rows = po.label_rows(0, many["hit_idx"], many["hit_xyz"], many["hit_off"], many["mask_off"], res["ow_owner"], z, z, many["score"], z, many["P"])
    assert rows["claims"][:3].tolist() == [255, 255, 255] and (rows["claims"][3:] == 1).all() and len(rows["idx"]) == 1027


def _n(case, m):
    return int(case["hit_off"][m + 1] - case["hit_off"][m]), m
