"""CPU tests of the mask case table (tests/mask_cases.py): the plain reference equals the oracle, and every family meets the
condition that makes it reach the branch of csrc/masks.hip it is built for.  These are conditions on the cases, not
measurements of the kernels: if one fails, the case is wrong."""
import dataclasses

import numpy as np
import pytest

from cm3d_amd import rle
from tests import mask_cases as C


def test_plain_erosion_equals_the_oracle_on_every_tiny_mask_and_every_small_f2_size(oracle):
    for W, H, items, name in C.f1_cases():
        exp = C.erode_ref(items)
        for m, e in zip(items, exp):
            assert np.array_equal(oracle.erode3x3(m), e), (name, m.tolist())
    for W, H, items, name in C.f2_cases():
        if H <= 5 and W <= 97:
            exp = C.erode_ref(np.stack(items))
            for i, (m, e) in enumerate(zip(items, exp)):
                assert np.array_equal(oracle.erode3x3(m), e), (name, i)


def test_run_length_codec_round_trips_every_tiny_mask():
    for W, H, items, name in C.f1_cases():
        for m in items:
            c = rle.dense_to_counts(m)
            assert int(c.sum()) == W * H and np.array_equal(rle.counts_to_dense(c, W, H), m), (name, m.tolist())


def test_word_rect_and_unpack_rect_agree_with_the_pixels():
    """The helpers the GPU tests lean on, on masks where the answer can be read off."""
    assert C.word_rect(np.zeros((5, 70), np.uint8)) == (0, 0, 0, 0)
    m = np.zeros((9, 100), np.uint8); m[2:5, 31:65] = 1
    assert C.word_rect(m) == (0, 2, 3, 3)
    m = np.zeros((9, 100), np.uint8); m[8, 96:] = 1
    assert C.word_rect(m) == (3, 8, 1, 1)
    rng = np.random.default_rng(0)
    m = (rng.random((7, 100)) < 0.5).astype(np.uint8)
    w = C.pack_words(m)
    assert w.shape == (7, 4) and not (w[:, 3] >> 4).any()
    assert np.array_equal(C.unpack_rect(w[1:4, 1:4].reshape(-1), (1, 1, 3, 3), 100), m[1:4, 32:100])
    assert np.array_equal(C.unpack_rect(w[:, :2].reshape(-1), (0, 0, 2, 7), 100), m[:, :64])
    assert C.bounds(np.stack([m * 0, m]))[0].tolist() == [C.INT_MAX, C.INT_MAX, -1, -1]


def test_f3_lists_have_their_run_counts_alignments_and_thresholds():
    cases = C.f3_cases()
    for n in C.F3_RUNS:
        c = C.f3_list(n)
        assert c.size == n and int(c.astype(np.int64).sum()) == C.F3_W * C.F3_H
        if n > 3:           # dashes of consecutive rows overlap: the erosion has something to get wrong
            assert (c[1::2] >= 3).all()
    seen = {}
    for k, case in enumerate(cases[:4]):
        sizes = [np.asarray(c).size for c in case[2]]
        assert sizes == [1] * k + C.F3_RUNS
        for s, a in zip(sizes[k:], C.f3_alignments(case)[k:]):
            seen.setdefault(s, set()).add(a)
        # the batch as a whole stays in the wave form when nothing is forced
        assert sum(sizes) <= 1024 * len(sizes)
    assert all(seen[n] == {0, 1, 2, 3} for n in C.F3_RUNS)
    at, above = cases[4], cases[5]
    assert sum(np.asarray(c).size for c in at[2]) == 1024 * len(at[2])
    assert sum(np.asarray(c).size for c in above[2]) == 1024 * len(above[2]) + 1


def test_f3_dashes_leave_eroded_pixels():
    W, H = C.F3_W, C.F3_H
    for n in (129, 4097):
        assert C.erode_ref(rle.counts_to_dense(C.f3_list(n), W, H)).any()


def _frame_with(fr, W, H, lists):
    n = len(lists)
    return dataclasses.replace(fr, width=W, height=H, rles=[{"size": [W, H], "counts": rle.counts_to_string(c)} for c in lists],
                               labels=[fr.labels[0]] * n, scores=[0.5] * n, cam_nums=[0] * n)


def test_f4_lists_are_valid_coco_run_lists_with_zero_length_runs():
    from cm3d_amd import lifting, synthetic as syn
    sizes = set()
    tiny = syn.make_frame(syn.config("tiny"), 0)
    lane = [syn.make_lane_table(tiny.ego_xyz[:2], 50, seed=1)]
    for W, H, items, name in C.f4_cases():
        for c in items:
            assert int(c.astype(np.int64).sum()) == W * H, name
            assert (c[2:] == 0).any(), name
            assert c[0] == 0 and c[1] == 0, name                    # the leading 0, 0
            assert np.array_equal(rle.string_to_counts(rle.counts_to_string(c)), c), name
            sizes.add(c.size)
        hb = lifting.pack_frames([_frame_with(tiny, W, H, items)], lane, [0])
        assert hb.n_masks == len(items)
        with pytest.raises(ValueError):                             # the check is there: a list one pixel too long is refused
            lifting.pack_frames([_frame_with(tiny, W, H, [np.append(items[0], np.uint32(1))])], lane, [0])
    # with the zero-length runs in, one list crosses 512 runs (the wave form's chunk) and one 2048 (the workgroup form's)
    assert 511 + 2 * C.F4_INSERTIONS in sizes and 2047 + 2 * C.F4_INSERTIONS in sizes and C.F4_INSERTIONS >= 1
    # the long lists hold a one-pixel 1-run that abuts the next 1-run across a zero-length 0-run
    for c in C.f4_cases()[-1][2]:
        j = np.arange(1, c.size - 2, 2)
        assert ((c[j] == 1) & (c[j + 1] == 0) & (c[j + 2] > 0)).any(), c.size
    # a first pixel that is clear behind a leading 0, 0, and one that is set
    firsts = {bool(rle.counts_to_dense(c, W, H)[0, 0]) for W, H, items, _ in C.f4_cases() for c in items}
    assert firsts == {False, True}


def test_split_runs_covers_the_stated_positions():
    rng = np.random.default_rng(1)
    c = np.array([5, 3, 7, 2, 8], np.uint32)
    assert C.split_runs(c, [(0, 0)], rng).tolist() == [0, 0, 5, 3, 7, 2, 8]
    assert C.split_runs(c, [(0, 2)], rng).tolist() == [2, 0, 3, 3, 7, 2, 8]
    assert C.split_runs(c, [(4, 8)], rng).tolist() == [5, 3, 7, 2, 8, 0, 0]
    assert C.split_runs(c, [(2, 1), (2, 4)], rng).tolist() == [5, 3, 1, 0, 4, 0, 2, 2, 8]
    for _ in range(20):
        s = C.split_runs(c, [0, 4, 2, 2], rng)
        assert s.size == 13 and np.array_equal(rle.counts_to_dense(s, 5, 5), rle.counts_to_dense(c, 5, 5))


def test_families_reach_their_branches():
    wide = narrow = False
    for W, H, items, name in C.f2_cases():
        Wp = (W + 31) // 32
        r = C.word_rects(np.stack(items))
        wide |= bool(((r[:, 2] >= 64) & (r[:, 2] < Wp)).any())
        narrow |= W < 32
        if Wp > 64:         # both placements, at every such width
            assert ((r[:, 2] >= 64) & (r[:, 2] < Wp) & (r[:, 0] == 0)).any(), name
            assert ((r[:, 2] >= 64) & (r[:, 2] < Wp) & (r[:, 0] + r[:, 2] == Wp)).any(), name
    assert wide and narrow
    assert {W for W, _, _, _ in C.f2_cases()} == set(C.F2_WIDTHS) and len(C.f2_cases()) == len(C.F2_WIDTHS) * len(C.F2_HEIGHTS)
    # F1: 15 360 masks less one per size, no count a multiple of 4
    assert sum(len(items) for _, _, items, _ in C.f1_cases()) == 15360 - len(C.F1_SIZES)
    assert all(len(items) % 4 for _, _, items, _ in C.f1_cases())
    (W, H, items, _), = C.f5_cases()
    assert (W, H) == (4095, 32767) and len(items) == 5
    last = []
    for counts, blocks in items:
        c = counts.astype(np.int64)
        assert int(c.sum()) == W * H
        last.append(int(c[:-1].sum() if c.size % 2 else c.sum()) - 1)             # index of the last set pixel
        # the run list paints the blocks: starts and lengths of its 1-runs
        starts = np.cumsum(c)[0:-1:2][:c.size // 2]
        want = [(y * W + xa, xb - xa + 1) for xa, ya, xb, yb in blocks for y in range(ya, yb + 1)]
        merged = []
        for s, l in want:                                                       # a full-width bar is one run
            if merged and merged[-1][0] + merged[-1][1] == s:
                merged[-1] = (merged[-1][0], merged[-1][1] + l)
            else:
                merged.append((s, l))
        assert list(zip(starts.tolist(), c[1::2].tolist())) == merged
    assert max(last) > 2 ** 24 and sum(l > 2 ** 24 for l in last) >= 4


def test_f5_expected_crop_follows_the_border_rule():
    W, H = C.F5_W, C.F5_H
    rect, e = C.f5_expected([(4055, 32758, 4094, 32766)], W, H)     # last row and column: only the inner edges erode
    assert rect == (126, 32758, 2, 9) and e.shape == (9, 63)
    want = np.zeros((9, 63), np.uint8); want[1:, 4056 - 126 * 32:] = 1
    assert np.array_equal(e, want)
    rect, e = C.f5_expected([(100, 0, 139, 8)], W, H)
    want = np.zeros((9, 64), np.uint8); want[:8, 101 - 96:139 - 96] = 1
    assert rect == (3, 0, 2, 9) and np.array_equal(e, want)


def test_row_of_emulation_equals_integer_division_at_every_row_boundary():
    H = C.F5_H
    y = np.arange(H, dtype=np.int64)
    for W in sorted(set(C.F2_WIDTHS) | {C.F5_W}):
        assert W * H < 2 ** 31
        for d in (-1, 0, 1):
            s = y * W + d
            s = s[(s >= 0) & (s < W * H)]
            assert np.array_equal(C.rw_row_of_emulated(s, W), s // W), (W, d)
