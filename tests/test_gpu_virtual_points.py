"""GPU: cm3d_hit_project against the oracle's project_points, and cm3d_virtual_points against cm3d_amd.virtualpoints.virtual_points_host
on the cases of tests/virtual_points_cases.py -- bit for bit in all seven arrays, with every output buffer poisoned before the call.
The expectation is made on the host alone; nothing in it comes from the device."""
import numpy as np
import pytest

from cm3d_amd import virtualpoints as vp
from tests import virtual_points_cases as vc

pytestmark = pytest.mark.gpu
FILL = 0xA5
WIDTH = {"vp_xyz": 3, "vp_pix": 2, "vp_src": 1, "vp_depth": 1, "vp_d2": 1}


def _bits(a):
    a = np.ascontiguousarray(a)
    return a.view({4: np.uint32, 8: np.uint64}[a.dtype.itemsize])


def _poisoned(a):
    return np.all(np.ascontiguousarray(a).view(np.uint8) == FILL)


def _device(c, **over):
    from cm3d_amd import ops
    a = dict(c.host_args(), **over)
    return ops.virtual_points(a["packed"], a["bbox"], a["W"], a["H"], a["cams"], a["mask_off"], a["mask_frame"], a["mask_cam"], a["flags"],
                              a["hit_uvd"], a["off"], a["per_mask"], a["seed"], a["max_px"], a["kept_only"], a["frame_seed"], idx_cap=a["idx_cap"],
                              fill=FILL)


def _same(c, got, exp):
    """All seven arrays: counts and statuses whole, the rows below every count to the bit, the rows behind it untouched."""
    K, M = c.per_mask, c.M
    assert got["vp_count"].dtype == np.int32 and np.array_equal(got["vp_count"][:M], exp["vp_count"])
    assert got["vp_status"].dtype == np.int32 and np.array_equal(got["vp_status"][:M], exp["vp_status"])
    for k, w in WIDTH.items():
        g, e = got[k].reshape(-1, w), exp[k].reshape(-1, w)
        assert got[k].dtype == exp[k].dtype and g.shape[0] >= M * K, k
        for m in range(M):
            n = int(exp["vp_count"][m])
            assert np.array_equal(_bits(g[m * K:m * K + n]), _bits(e[m * K:m * K + n])), (k, m)
            assert _poisoned(g[m * K + n:(m + 1) * K]), (k, m)
    return int(exp["vp_count"].sum())


@pytest.fixture(scope="module")
def expected():
    return {c.name + ("" if c.kept_only else "_all"): (c, vp.virtual_points_host(**c.host_args())) for c in vc.cases()}


@pytest.mark.parametrize("name", ["shapes", "ties", "switches", "switches_all", "seeds", "round_trip"])
def test_the_kernel_equals_the_host_statement(expected, name):
    c, exp = expected[name]
    n = _same(c, _device(c), exp)
    print(f"{name}: {c.M} masks, {n} points, statuses {np.bincount(exp['vp_status'], minlength=5).tolist()}")
    assert n > 0


def test_what_the_cases_reach(expected):
    """The cases are the ones the kernel can go wrong at: every list length next to a wave and next to the LDS stage, every stored form,
    rectangles of one, two and three words per row."""
    c, exp = expected["shapes"]
    assert {0, 1, 63, 64, 65, 257, 300} <= set(np.diff(c.off).tolist())
    A = [int(m.sum()) for m in c.eroded]
    assert 1 in A and c.per_mask in A and any(1 < a < c.per_mask for a in A) and max(A) > 100 * c.per_mask
    words = {int((b[2] >> 5) - (b[0] >> 5) + 1) for b in c.bbox if b[2] >= b[0]}
    assert {1, 2, 3} <= words
    assert {tuple(b[4:6]) == (0, 0) and b[6] == (c.W + 31) // 32 for b in c.bbox} == {True, False}
    c, exp = expected["switches"]
    assert 0 < exp["vp_count"][0] < c.per_mask
    c, exp = expected["seeds"]
    K = c.per_mask
    assert not np.array_equal(exp["vp_pix"][:K], exp["vp_pix"][2 * K:3 * K])


def test_one_full_image_mask_with_1024_points():
    c = vc.case_full_image()
    exp = vp.virtual_points_host(**c.host_args())
    assert exp["vp_count"].tolist() == [1024]
    _same(c, _device(c), exp)


def test_products_beyond_32_bits():
    c = vc.case_wide_products()
    exp = vp.virtual_points_host(**c.host_args())
    A = c.W * c.H
    assert exp["vp_count"].tolist() == [1024] and 1024 * A > 2 ** 32
    r = exp["vp_pix"][:, 1].astype(np.int64) * c.W + exp["vp_pix"][:, 0]
    assert all(j * A // 1024 <= r[j] < (j + 1) * A // 1024 for j in range(1024))
    _same(c, _device(c), exp)


def test_nothing_at_or_beyond_idx_cap_is_read(expected):
    """The rows behind idx_cap hold a return right on every pixel of no list; a smaller idx_cap than the offsets say cuts the lists."""
    c, _ = expected["seeds"]
    cut = c.idx_cap - 130                                                   # the last list loses all its rows, the one before it 30
    uvd = c.hit_uvd.copy()
    uvd[cut:] = np.nan                                                      # whatever is there must not matter
    exp = vp.virtual_points_host(**dict(c.host_args(), idx_cap=cut))
    assert exp["vp_status"].tolist() == [0, 0, 0, 2]
    _same(c, _device(c, idx_cap=cut, hit_uvd=uvd), exp)
    exp0 = vp.virtual_points_host(**dict(c.host_args(), idx_cap=0))
    assert exp0["vp_status"].tolist() == [2, 2, 2, 2]
    _same(c, _device(c, idx_cap=0), exp0)


def test_no_mask_at_all():
    c = vc.Case("none", vc.W0, vc.H0, vc.CAMS2[:1], [])
    got = _device(c)
    assert all(_poisoned(v) for v in got.values())
    from cm3d_amd import ops
    assert _poisoned(ops.hit_project(np.zeros((4, 4), np.float32), [0], [], [], vc.CAMS2[:1], fill=FILL))


def test_argument_errors_leave_the_poison():
    import torch
    from cm3d_amd import _lib
    L = _lib.lib()
    c = vc.case_ties()
    dev = torch.device("cuda:0")
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)
    d = dict(packed=t(c.packed.view(np.int32)), bbox=t(c.bbox), cams=t(c.cams), mask_off=t(c.mask_off), mask_frame=t(c.mask_frame),
             mask_cam=t(c.mask_cam), flags=t(c.flags), uvd=t(c.hit_uvd), off=t(c.off), fs=t(c.frame_seed.view(np.int32)))
    K, M = c.per_mask, c.M
    outs = [torch.full((n,), FILL, dtype=torch.uint8, device=dev) for n in (4 * M, 4 * M, 24 * M * K, 8 * M * K, 4 * M * K, 4 * M * K, 4 * M * K)]
    st = torch.cuda.current_stream().cuda_stream

    def call(per_mask=K, max_px=0.0, H=c.H, n_cams=c.cams.shape[1], flags=d["flags"], M=M):
        return L.cm3d_virtual_points(d["packed"].data_ptr(), d["bbox"].data_ptr(), c.W, H, d["cams"].data_ptr(), n_cams, d["mask_off"].data_ptr(),
                                     d["mask_frame"].data_ptr(), d["mask_cam"].data_ptr(), None if flags is None else flags.data_ptr(),
                                     c.cams.shape[0], M, d["uvd"].data_ptr(), d["off"].data_ptr(), c.idx_cap, per_mask, 0, max_px, 1,
                                     d["fs"].data_ptr(), *[o.data_ptr() for o in outs], st)
    for kw in (dict(per_mask=0), dict(per_mask=1025), dict(max_px=-1.0), dict(max_px=float("nan")), dict(max_px=float("inf")), dict(H=4097),
               dict(H=0), dict(n_cams=9), dict(flags=None), dict(M=-1)):
        assert call(**kw) == -1, kw
    assert L.cm3d_hit_project(d["uvd"].data_ptr(), d["off"].data_ptr(), d["mask_frame"].data_ptr(), d["mask_cam"].data_ptr(), d["cams"].data_ptr(),
                              9, 1, M, c.idx_cap, outs[2].data_ptr(), st) == -1
    assert L.cm3d_hit_project(d["uvd"].data_ptr() + 4, d["off"].data_ptr(), d["mask_frame"].data_ptr(), d["mask_cam"].data_ptr(),
                              d["cams"].data_ptr(), c.cams.shape[1], 1, M, c.idx_cap, outs[2].data_ptr(), st) == -1
    torch.cuda.synchronize()
    assert all(bool((o == FILL).all()) for o in outs)
    assert L.cm3d_virtual_points_check(1, 0.0) == 0 and L.cm3d_virtual_points_check(1024, 1e9) == 0
    assert call() == 0                                                     # the same call with nothing wrong
    torch.cuda.synchronize()
    assert not bool((outs[0] == FILL).all())


# ---- step 1 -----------------------------------------------------------------------------------------------------------------------------
def _projection_case(offset):
    """Lists of three masks under cameras of one, two and three stages at a world offset, in two frames."""
    cams = np.stack([np.stack([vc.camera(1, offset), vc.camera(2, offset)]), np.stack([vc.camera(3, offset), vc.camera(2, offset, skew=3.5)])])
    rng = np.random.default_rng(int(offset) + 3)
    masks = [(0, 0, 70), (0, 1, 1), (0, 1, 0), (1, 0, 129), (1, 1, 64)]     # frame, camera, list length
    lists = []
    for f, c, n in masks:
        uvd = np.stack([rng.uniform(1, 199, n), rng.uniform(1, 119, n), rng.uniform(2.5, 80, n)], 1)
        lists.append(vc.world_points(cams[f, c], uvd))
    off = np.concatenate([[0], np.cumsum([len(x) for x in lists])]).astype(np.int32)
    return cams, masks, np.concatenate(lists), off


@pytest.mark.parametrize("offset", [0.0, 1700.0])
def test_hit_project_equals_the_oracle_bit_for_bit(oracle, offset):
    from cm3d_amd import ops
    cams, masks, xyz, off = _projection_case(offset)
    slack = np.full((5, 4), 7.0, np.float32)
    frames, cam_of = [m[0] for m in masks], [m[1] for m in masks]
    got = ops.hit_project(np.concatenate([xyz, slack]), off, frames, cam_of, cams, idx_cap=len(xyz), fill=FILL)
    assert got.shape == (len(xyz) + 5, 4) and _poisoned(got[len(xyz):])
    stages = set()
    for m, (f, c, n) in enumerate(masks):
        exp = oracle.project_points(xyz[off[m]:off[m + 1]], cams[f, c])
        g = got[off[m]:off[m + 1]]
        assert np.array_equal(_bits(g[:, :3]), _bits(exp)) and np.all(_bits(g[:, 3]) == 0), m
        if n:
            assert np.all((g[:, 0] > 0) & (g[:, 0] < 200) & (g[:, 2] > 2))  # the crafted rows are where they were meant to be
            stages.add(int(cams[f, c][54]))
    assert stages == {1, 2, 3}
    # a capacity below the offsets: the rows from it on are not written; a mask whose camera number is out of range: its rows neither
    cut = int(off[4]) + 10
    got = ops.hit_project(xyz, off, frames, [0, 1, 1, 0, 1], cams, idx_cap=cut, fill=FILL)
    assert _poisoned(got[cut:]) and np.array_equal(_bits(got[off[4]:cut, :3]), _bits(oracle.project_points(xyz[off[4]:cut], cams[1, 1])))
    got = ops.hit_project(xyz, off, frames, [0, 1, 1, 2, 1], cams, fill=FILL)
    assert _poisoned(got[off[3]:off[4]]) and not _poisoned(got[off[4]:])


def test_every_listed_point_of_a_real_pass_lies_on_a_set_bit_of_its_own_mask():
    import torch
    from cm3d_amd import lifting, ops, synthetic as syn
    cfg = syn.config("tiny")
    frames = [syn.make_frame(cfg, i) for i in range(3)]
    lanes = [syn.make_lane_table(frames[0].ego_xyz[:2], 2000, seed=3)]
    hb = lifting.pack_frames(frames, lanes, [0, 0, 0])
    eng = lifting.LiftEngine("cuda:0", virtual=vp.VirtualPoints(8))
    eng.upload(hb)
    eng.run(masks="rle")
    torch.cuda.synchronize()
    got = eng.download(full=True)
    bits = ops.unpack_bits(eng.b.packed, hb.width, eng.b.bbox)
    off, uvd = got["hit_off"], got["hit_uvd"]
    assert uvd.shape == (int(off[-1]), 4) and off[-1] > 100
    for m in range(hb.n_masks):
        u, v = np.floor(uvd[off[m]:off[m + 1], 0]).astype(int), np.floor(uvd[off[m]:off[m + 1], 1]).astype(int)
        assert bits[m][v, u].all(), m
    assert got["vp_count"].sum() > 0
