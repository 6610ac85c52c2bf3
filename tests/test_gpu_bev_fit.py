"""GPU: the yaw fit's kernels (cm3d_bev_fit, cm3d_yaw_select) against their host statements (cm3d_amd/bevfit.py) on the case tables of
tests/bev_fit_cases.py: the fit to the bit, between guard words, and after a simulated capacity overflow; the selection exactly where it
copies and within one float32 ulp at pi where it rounds an atan2."""
import numpy as np
import pytest

from cm3d_amd import bevfit
from tests import bev_fit_cases as cases

pytestmark = pytest.mark.gpu

GUARD = 0x5A5A5A5A


def _expected(lists, K, d0=cases.D0, min_points=cases.MIN_POINTS, min_length=cases.MIN_LENGTH):
    tab = bevfit.angle_table(K)
    r = [bevfit.bev_fit_host(p, K, d0, min_points, min_length, tab) for p in lists]
    return (np.array([x[0] for x in r], np.int32), np.array([x[1] for x in r], np.float64).reshape(-1, 6), np.array([x[2] for x in r], np.int32))


def _guarded_fit(xyz, off, K, idx_cap, d0=cases.D0, min_points=cases.MIN_POINTS, min_length=cases.MIN_LENGTH, poison_from=None):
    """cm3d_bev_fit with every output between guard words; rows of hit_xyz from `poison_from` on are NaN (nothing may read them).
    Returns (fit_k, fit_rect, fit_status)."""
    import torch
    from cm3d_amd import _lib
    L = _lib.lib()
    M = off.size - 1
    G = 8
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda()
    P = np.array(xyz, np.float32)
    if poison_from is not None:
        P[poison_from:] = np.nan
    d_xyz, d_off, d_cs = t(P), t(off), t(bevfit.angle_table(K))
    fk = torch.full((M + 2 * G,), GUARD, dtype=torch.int32, device="cuda")
    fs = torch.full((M + 2 * G,), GUARD, dtype=torch.int32, device="cuda")
    fr = torch.full((6 * M + 2 * G,), -7.25, dtype=torch.float64, device="cuda")
    rc = L.cm3d_bev_fit(d_xyz.data_ptr(), d_off.data_ptr(), M, idx_cap, d_cs.data_ptr(), K, d0, min_points, min_length, fk[G:].data_ptr(),
                        fr[G:].data_ptr(), fs[G:].data_ptr(), torch.cuda.current_stream().cuda_stream)
    assert rc == 0
    torch.cuda.synchronize()
    fk, fs, fr = fk.cpu().numpy(), fs.cpu().numpy(), fr.cpu().numpy()
    for a in (fk, fs):
        assert (a[:G] == GUARD).all() and (a[M + G:] == GUARD).all()
    assert (fr[:G] == -7.25).all() and (fr[6 * M + G:] == -7.25).all()
    return fk[G:M + G], fr[G:6 * M + G].reshape(M, 6), fs[G:M + G]


def _assert_bits(got, exp, names):
    gk, gr, gs = got
    ek, er, es = exp
    bad = [names[i] for i in range(len(names)) if gk[i] != ek[i] or gs[i] != es[i] or not np.array_equal(gr[i].view(np.uint64), er[i].view(np.uint64))]
    assert not bad, bad[:8]


@pytest.mark.parametrize("K", cases.ANGLES)
def test_fit_equals_host_statement_to_the_bit(K):
    tab = cases.standalone()
    names = list(tab)
    lists = [tab[n][0] for n in names]
    xyz, off = cases.pack(lists)
    got = _guarded_fit(xyz, off, K, xyz.shape[0])
    exp = _expected(lists, K)
    assert set(exp[2]) == {0, 1, 2, 3, 4}
    _assert_bits(got, exp, names)
    assert (got[0][got[2] != 0] == -1).all() and not got[1][got[2] != 0].any()


def test_fit_with_other_parameters_and_through_ops():
    from cm3d_amd import ops
    tab = cases.standalone()
    names = [n for n in tab if not n.startswith("car_noisy")]
    lists = [tab[n][0] for n in names]
    xyz, off = cases.pack(lists)
    for K, d0, mp, ml in ((192, 0.1, 2, 0.0), (64, 0.01, 64, 4.45)):
        got = ops.bev_fit(xyz, off, K, d0, mp, ml)
        _assert_bits(got, _expected(lists, K, d0, mp, ml), names)


def test_fit_after_a_capacity_overflow():
    """The offsets describe more than idx_cap points (what cm3d_compact_hits leaves behind when status bit 1 is set): nothing at or
    beyond idx_cap is read -- those rows are NaN here, and a list cut at idx_cap that read one would end with status 4 --, the lists
    that lie whole below idx_cap give the statement's answer, the list that straddles it the answer of its part below."""
    tab = cases.standalone()
    names = ["car_03", "len_65", "len_513", "car_noisy_11", "len_1000", "len_129", "car_20"]
    lists = [tab[n][0] for n in names]
    xyz, off = cases.pack(lists)
    cap = int(off[4]) + 700                        # inside len_1000
    assert off[4] < cap < off[5] and off[-1] > cap
    got = _guarded_fit(xyz, off, 128, cap, poison_from=cap)
    cut = [p for p in lists[:4]] + [lists[4][:700], lists[5][:0], lists[6][:0]]
    exp = _expected(cut, 128)
    assert exp[2].tolist() == [0, 0, 0, 0, 0, 2, 2]
    _assert_bits(got, exp, names)
    # offsets that are no offsets at all: negative, beyond the capacity, descending
    wild = np.array([-5, 40, 2 ** 31 - 1, 100, -(2 ** 31), 30], np.int32)
    got = _guarded_fit(xyz, wild, 64, 300, poison_from=300)
    rng = lambda lo, hi: xyz[max(0, min(lo, 300)):max(max(0, min(lo, 300)), min(hi, 300))]
    exp = _expected([rng(int(wild[m]), int(wild[m + 1])) for m in range(5)], 64)
    _assert_bits(got, exp, [f"wild_{m}" for m in range(5)])


@pytest.mark.parametrize("waymo", [False, True])
def test_select_equals_host_statement(waymo):
    from cm3d_amd import ops
    t = cases.select_table(waymo)
    ulp_at_pi = 2.0 ** -22
    for lmd in cases.LANE_MIN_DISTS:
        yaw, idx, src = ops.yaw_select(t["fit_rect"], t["fit_status"], t["medoid_pos"], t["mask_frame"], t["class_id"], t["is_vehicle"],
                                       t["lane_dist"], t["lane"], t["lane_off"], t["frame_lane"], t["lane_idx"], lmd, t["pose_rt"])
        eyaw, esrc = cases.select_host(t, lmd)
        assert np.array_equal(src, esrc) and np.array_equal(idx, np.arange(len(src)))
        assert set(src) == {0, 1}
        lane = src == 0
        assert np.array_equal(yaw[lane].view(np.uint32), eyaw[lane].view(np.uint32))
        # the two atan2 differ by float64 ulps, and the rounding to float32 can land them one float32 ulp apart
        d = np.abs(yaw[~lane].astype(np.float64) - eyaw[~lane].astype(np.float64))
        print(f"waymo={waymo} lane_min_dist={lmd}: {int((~lane).sum())} fitted yaws, {int((d > 0).sum())} differ, max {d.max():.3g}")
        assert d.max() <= ulp_at_pi


def test_kernel_arguments():
    import torch
    from cm3d_amd import _lib
    L = _lib.lib()
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda()
    st = torch.cuda.current_stream().cuda_stream
    xyz, off, cs = t(np.zeros((32, 4), np.float32)), t(np.array([0, 30, 32], np.int32)), t(bevfit.angle_table(256))
    fk, fr, fs = t(np.zeros(2, np.int32)), t(np.zeros((2, 6))), t(np.zeros(2, np.int32))
    args = [xyz.data_ptr(), off.data_ptr(), 2, 32, cs.data_ptr(), 128, 0.05, 20, 1.0, fk.data_ptr(), fr.data_ptr(), fs.data_ptr(), st]
    assert L.cm3d_bev_fit(*args) == 0
    for k in (0, 1, 4, 9, 10, 11):
        q = list(args); q[k] = None
        assert L.cm3d_bev_fit(*q) == -1, k
    inf, nan = float("inf"), float("nan")
    for k, v in ((2, 0), (2, -1), (3, 0), (5, 0), (5, 32), (5, 100), (5, 320), (5, -64), (6, 0.0), (6, -0.05), (6, nan), (6, inf), (7, 1), (7, 0),
                 (7, -3), (8, -0.5), (8, nan), (8, inf)):
        q = list(args); q[k] = v
        assert L.cm3d_bev_fit(*q) == -1, (k, v)
    for K in (64, 192, 256):
        q = list(args); q[5] = K
        assert L.cm3d_bev_fit(*q) == 0
    M, F = 2, 1
    rect, fst, mp, mf, cls = t(np.zeros((M, 6))), t(np.zeros(M, np.int32)), t(np.zeros(M, np.int32)), t(np.zeros(M, np.int32)), t(np.zeros(M, np.int32))
    veh, ld, lane, lo, fl, li = (t(np.ones(3, np.int32)), t(np.zeros(M)), t(np.zeros((4, 3), np.float32)), t(np.array([0, 4], np.int32)),
                                 t(np.zeros(F, np.int32)), t(np.zeros(M, np.int32)))
    pose = t(np.zeros((F, 12), np.float32))
    tab, idx, src = t(np.zeros((M, 3), np.float32)), t(np.zeros(M, np.int32)), t(np.zeros(M, np.int32))
    args = [rect.data_ptr(), fst.data_ptr(), mp.data_ptr(), mf.data_ptr(), cls.data_ptr(), veh.data_ptr(), 3, ld.data_ptr(), 0.0, lane.data_ptr(),
            lo.data_ptr(), fl.data_ptr(), li.data_ptr(), 1, 4, None, M, F, tab.data_ptr(), idx.data_ptr(), src.data_ptr(), st]
    assert L.cm3d_yaw_select(*args) == 0
    q = list(args); q[15] = pose.data_ptr()
    assert L.cm3d_yaw_select(*q) == 0              # (the pose is the one pointer that may be null)
    for k in (0, 1, 2, 3, 4, 5, 7, 9, 10, 11, 12, 18, 19, 20):
        q = list(args); q[k] = None
        assert L.cm3d_yaw_select(*q) == -1, k
    for k, v in ((6, 0), (13, 0), (14, 0), (16, 0), (17, 0), (16, -2), (8, -1.0), (8, nan)):
        q = list(args); q[k] = v
        assert L.cm3d_yaw_select(*q) == -1, (k, v)
    q = list(args); q[8] = inf
    assert L.cm3d_yaw_select(*q) == 0              # never the fit
    torch.cuda.synchronize()
