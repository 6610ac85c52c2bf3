"""Host: the rule of the virtual-point stage as cm3d_amd.virtualpoints states it (include/cm3d_hip.h, cm3d_virtual_points), on the cases
of tests/virtual_points_cases.py -- the sampling, the nearest return, the unprojection's round trip, the statuses, the flags of the entry
points and the per-frame file.  Nothing here touches the device."""
import argparse
from fractions import Fraction

import numpy as np
import pytest

from cm3d_amd import virtualpoints as vp
from tests import virtual_points_cases as vc


@pytest.fixture(scope="module")
def results():
    return {c.name + ("" if c.kept_only else "_all"): (c, vp.virtual_points_host(**c.host_args())) for c in vc.cases()}


def _rows(c, res, m):
    return slice(m * c.per_mask, m * c.per_mask + int(res["vp_count"][m]))


def test_every_sampled_pixel_is_a_set_pixel_and_the_pixels_are_distinct(results):
    n = 0
    for c, res in results.values():
        for m in range(c.M):
            pix = res["vp_pix"][_rows(c, res, m)]
            assert c.eroded[m][pix[:, 1], pix[:, 0]].all()
            assert len({tuple(p) for p in pix.tolist()}) == len(pix)
            n += len(pix)
    assert n > 500


def test_every_rank_lies_in_its_stratum():
    for A, K in [(1, 50), (3, 50), (50, 50), (51, 50), (997, 50), (1440000, 1024), (4325376, 1024)]:
        r = vp.sample_ranks(A, K, 7, 11, 3)
        k = min(A, K)
        assert r.size == k and all(j * A // k <= r[j] < (j + 1) * A // k for j in range(k))
        assert np.all(np.diff(r) > 0)


def test_a_mask_of_at_most_k_pixels_is_drawn_whole(results):
    c, res = results["shapes"]
    seen = 0
    for m in range(c.M):
        A = int(c.eroded[m].sum())
        if 0 < A <= c.per_mask and res["vp_status"][m] == 0:
            pix = res["vp_pix"][_rows(c, res, m)]
            ys, xs = np.nonzero(c.eroded[m])
            assert np.array_equal(pix, np.stack([xs, ys], 1))              # every pixel once, in rank order (no limit: nothing dropped)
            seen += 1
    assert seen >= 4                                                        # A = 1, A < K twice, A = K


def test_the_mixer_and_the_ranks_are_the_rules_integers():
    assert vp.mix(0) == 0
    x = 0x12345678
    y = x ^ (x >> 16)
    y = (y * 0x7FEB352D) & 0xFFFFFFFF
    y ^= y >> 15
    y = (y * 0x846CA68B) & 0xFFFFFFFF
    y ^= y >> 16
    assert vp.mix(x) == y
    A, K, seed, fs, kk = 1000, 7, 0xFFFFFFFF, 0xFFFFFFFE, 1023
    h0 = seed ^ ((fs * 0x9E3779B1) % 2 ** 32) ^ ((kk * 0x85EBCA77) % 2 ** 32)
    exp = [j * A // K + vp.mix(h0 ^ ((j * 0xC2B2AE3D) % 2 ** 32)) % ((j + 1) * A // K - j * A // K) for j in range(K)]
    assert vp.sample_ranks(A, K, seed, fs, kk).tolist() == exp


def test_the_frame_seed_not_the_batch_position_decides(results):
    c, res = results["seeds"]
    K = c.per_mask
    pix = res["vp_pix"].reshape(c.M, K, 2)
    assert res["vp_count"].tolist() == [K] * 4
    assert not np.array_equal(pix[0], pix[2]) and not np.array_equal(pix[1], pix[3])       # equal masks, other frame seeds
    assert not np.array_equal(pix[0], pix[1])                                              # other positions in the frame
    # the same frames in the other batch positions, each with its own seed: the same pixels
    a = c.host_args()
    swapped = dict(a, cams=a["cams"][::-1], frame_seed=a["frame_seed"][::-1])
    # (frame 0 now holds what frame 1 held: masks 0, 1 are the old 2, 3)
    res2 = vp.virtual_points_host(**swapped)
    assert np.array_equal(res2["vp_pix"].reshape(c.M, K, 2)[[2, 3, 0, 1]], pix)
    # and another seed of the stage: other pixels
    res3 = vp.virtual_points_host(**dict(a, seed=1))
    assert not np.array_equal(res3["vp_pix"], res["vp_pix"])


def test_fmaf32_is_the_single_rounding():
    rng = np.random.default_rng(5)
    a = (rng.standard_normal(4000) * rng.choice([1e-4, 1.0, 300.0], 4000)).astype(np.float32)
    c = np.square(rng.standard_normal(4000) * rng.choice([1e-4, 1.0, 300.0], 4000)).astype(np.float32)
    # halfway cases made on purpose: a * a + c exactly between two float32
    t = np.float32(1.0) + np.float32(2.0 ** -12)                           # t * t = 1 + 2^-11 + 2^-24: half an ulp above 1 + 2^-11
    a = np.concatenate([a, [t, t, t]]).astype(np.float32)
    c = np.concatenate([c, [0.0, 2.0 ** -40, -2.0 ** -40]]).astype(np.float32)
    got = vp.fmaf32(a, a, c)
    for i in range(a.size):
        ex = Fraction(float(a[i])) ** 2 + Fraction(float(c[i]))
        f = np.float32(float(ex))
        cands = [np.nextafter(f, np.float32(-np.inf)), f, np.nextafter(f, np.float32(np.inf))]
        best = min(cands, key=lambda q: (abs(Fraction(float(q)) - ex), int(q.view(np.uint32)) & 1))
        assert got[i] == best, i
    assert got[-2] > got[-3] == got[-1]                                    # the tie to even, above it, below it


def test_the_lower_of_two_equidistant_positions_wins_and_a_nan_never_does(results):
    c, res = results["ties"]
    K = c.per_mask
    assert res["vp_count"][:4].tolist() == [1, 1, 1, 0] and res["vp_status"][:4].tolist() == [0, 0, 0, 0]
    assert res["vp_src"][0] == 1 and res["vp_d2"][0] == 4.0 and res["vp_depth"][0] == 7.0
    assert res["vp_src"][K] == 0 and res["vp_d2"][K] == 25.0
    assert res["vp_src"][2 * K] == 2 and res["vp_d2"][2 * K] == 25.0
    big = res["vp_src"][_rows(c, res, 4)]
    assert len(big) == K and 10 not in big and 40 not in big               # the NaN row never, the duplicate's second copy never


def _round_trip(c, res):
    """(camera record, pixel error, relative depth error) of every point of a case."""
    for m in range(c.M):
        if res["vp_status"][m] != 0:
            continue
        cam = c.cams[c.mask_frame[m], c.mask_cam[m]]
        for r in range(*_rows(c, res, m).indices(10 ** 9)):
            u, v, d = vc.forward64(cam, res["vp_xyz"][r])
            px, py = res["vp_pix"][r]
            d0 = float(res["vp_depth"][r])
            yield cam, max(abs(u - (px + 0.5)), abs(v - (py + 0.5))), abs(d - d0) / abs(d0)


def test_the_round_trip_lands_on_the_pixel_centre(results):
    """The float64 forward chain of vp_xyz lands within 1e-6 px of (cx, cy) and within 1e-9 relative of d: float64 leaves about six
    orders of headroom at 2 km offsets.  The rule inverts a stage by its transpose, so this is a statement about records whose
    rotations are orthonormal as float32 values: the cameras of this case are quarter turns."""
    c, res = results["round_trip"]
    seen = set()
    for cam, e_px, e_d in _round_trip(c, res):
        assert e_px < 1e-6 and e_d <= 1e-9
        seen.add((int(cam[54]), int(cam[55]), bool(cam[46] != 0), bool(abs(cam[0]) > 1000)))
    assert len(seen) == 4 and {s[0] for s in seen} == {1, 2, 3} and any(s[2] for s in seen) and any(s[3] for s in seen) and any(not s[3] for s in seen)
    assert any(s[1] & 1 for s in seen) and any(s[1] & 2 for s in seen) and any(s[1] & 8 for s in seen)      # t_pre and t_post were there


def test_the_round_trip_through_rounded_rotations_misses_by_their_defect_only(results):
    """A rotation by any other angle has float32 entries off by up to 2^-25 each, so R R^T - I has a norm of up to 6 * 2^-25 = 1.8e-7 and
    the transpose misses the inverse by that much per stage, times the length of the camera-side vector: at most 1.5 depths here (half
    angles of 0.33 and 0.2, translations below a quarter of the least depth, 4 m).  That is a relative depth error of at most
    2.7e-7 per stage and, with fx = 620 and |u - cx| <= 0.33 fx, at most 620 * 1.33 * 2.7e-7 = 2.2e-4 px per stage -- the record's
    own defect, six orders above float64's.  Nothing of it grows with the 1.7 km offsets."""
    n = 0
    for name in ("shapes", "seeds", "switches_all"):
        c, res = results[name]
        for cam, e_px, e_d in _round_trip(c, res):
            ns = int(cam[54])
            assert e_px <= ns * 2.2e-4 and e_d <= ns * 2.7e-7
            n += 1
    assert n > 500


def test_statuses_kept_only_and_max_px(results):
    c, res = results["switches"]
    # kept, bit 1 clear, bit 0 clear, another camera, five cameras that cannot be inverted, a camera number out of range
    assert res["vp_status"].tolist() == [0, 1, 1, 0, 4, 4, 4, 4, 4, 4]
    assert all(res["vp_count"][m] == 0 for m in range(1, c.M) if res["vp_status"][m])
    n0 = int(res["vp_count"][0])
    assert 0 < n0 < c.per_mask                                              # twelve returns, three pixels: some samples have none near
    d2 = res["vp_d2"][:n0]
    assert np.all(d2.astype(np.float64) <= c.max_px ** 2)
    c2, all_masks = results["switches_all"]
    assert all_masks["vp_status"].tolist() == [0, 0, 0, 0, 4, 4, 4, 4, 4, 4] and all_masks["vp_count"][:4].tolist() == [c.per_mask] * 4
    # the kept samples are the unlimited run's, in its order, without holes
    keep = all_masks["vp_d2"][:c.per_mask].astype(np.float64) <= c.max_px ** 2
    assert keep.sum() == n0 and not keep.all()
    for k in ("vp_pix", "vp_src", "vp_depth", "vp_d2", "vp_xyz"):
        assert np.array_equal(all_masks[k][:c.per_mask][keep], res[k][:n0]), k
    c3, shapes = results["shapes"]
    st = shapes["vp_status"].tolist()
    assert st[9] == 2 and st[10] == 2 and st.count(0) == c3.M - 2          # the empty mask, the empty list


def test_records_that_point_outside_the_slot_count_as_empty():
    c = vc.case_shapes()
    a = c.host_args()
    for col, val in ((2, c.W), (3, c.H), (4, -1), (6, 99), (7, c.H + 1), (5, 200)):
        bb = a["bbox"].copy()
        bb[3, col] = val
        res = vp.virtual_points_host(**dict(a, bbox=bb))
        assert res["vp_status"][3] == 2 and res["vp_count"][3] == 0, (col, val)


def test_the_dataclass_and_the_host_statement_refuse_what_the_library_refuses():
    for kw in (dict(per_mask=0), dict(per_mask=1025), dict(max_px=-1.0), dict(max_px=float("nan")), dict(max_px=float("inf")),
               dict(seed=-1), dict(seed=2 ** 32)):
        with pytest.raises(ValueError):
            vp.VirtualPoints(**kw)
    v = vp.VirtualPoints(1024, 2 ** 32 - 1, 2.5, False)
    assert (v.per_mask, v.seed, v.max_px, v.kept_only, v.active) == (1024, 2 ** 32 - 1, 2.5, False, True)
    c = vc.case_ties()
    with pytest.raises(ValueError):
        vp.virtual_points_host(**dict(c.host_args(), per_mask=0))
    with pytest.raises(ValueError):
        vp.virtual_points_host(**dict(c.host_args(), flags=None))


def _parse(argv):
    ap = argparse.ArgumentParser()
    vp.add_arguments(ap)
    return ap.parse_args(argv), ap


def test_from_args():
    args, ap = _parse([])
    assert vp.from_args(args, ap) is None
    args, ap = _parse(["--virtual-points", "out"])
    assert vp.from_args(args, ap) == vp.VirtualPoints()
    args, ap = _parse(["--virtual-points", "out", "--virtual-points-per-mask", "7", "--virtual-points-seed", "9", "--virtual-points-max-px", "2.5",
                       "--virtual-points-all-masks"])
    assert vp.from_args(args, ap) == vp.VirtualPoints(7, 9, 2.5, False)
    for alone in (["--virtual-points-per-mask", "7"], ["--virtual-points-seed", "1"], ["--virtual-points-max-px", "1"], ["--virtual-points-all-masks"]):
        args, ap = _parse(alone)
        with pytest.raises(ValueError, match="needs --virtual-points"):
            vp.from_args(args)
        with pytest.raises(SystemExit):
            vp.from_args(args, ap)
    args, ap = _parse(["--virtual-points", "out", "--virtual-points-per-mask", "2000"])
    with pytest.raises(SystemExit):
        vp.from_args(args, ap)


def test_the_frame_file(tmp_path, results):
    c, res = results["seeds"]
    K = c.per_mask
    class_id, score = np.array([3, 1, 4, 1], np.int32), np.array([0.9, 0.8, 0.7, 0.6], np.float32)
    list_idx = np.arange(1000, 1000 + c.idx_cap, dtype=np.int32)
    rec = vp.frame_records(res, 1, K, c.mask_off, c.mask_cam, class_id, score, c.off, list_idx)
    path = vp.write_frame(str(tmp_path / "vp"), "token1", rec)
    z = np.load(path)
    assert path.endswith("token1.npz") and set(z.files) == {n for n, _ in vp.FILE_FIELDS}
    n = 2 * K
    for name, dtype in vp.FILE_FIELDS:
        assert z[name].dtype == dtype and z[name].shape[0] == n, name
    assert z["xyz"].shape == (n, 3) and z["pixel"].shape == (n, 2)
    assert np.array_equal(z["mask"], np.repeat([0, 1], K)) and np.array_equal(z["cam"], np.repeat([0, 1], K))
    assert np.array_equal(z["class_id"], np.repeat([4, 1], K)) and np.array_equal(z["score"], np.repeat(score[2:], K))
    assert np.array_equal(z["xyz"], res["vp_xyz"][2 * K:4 * K].astype(np.float32)) and np.array_equal(z["pixel"], res["vp_pix"][2 * K:4 * K])
    assert np.array_equal(z["depth"], res["vp_depth"][2 * K:4 * K])
    assert np.array_equal(z["src_idx"], 1000 + np.repeat(c.off[2:4], K) + res["vp_src"][2 * K:4 * K])
    # a frame without a point has no record
    none = dict(res, vp_count=np.zeros_like(res["vp_count"]))
    assert vp.frame_records(none, 0, K, c.mask_off, c.mask_cam, class_id, score, c.off, list_idx) is None
