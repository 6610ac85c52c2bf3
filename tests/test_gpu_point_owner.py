"""GPU: cm3d_point_owner through the raw library call against its host statement (cm3d_amd.pointowner.point_owner_host) on every crafted
case of tests/point_owner_cases.py and on its 200 random batches -- every output TO THE BIT, no tolerance: the rule is made of
comparisons and integers --, every written array between guard words; an idx_cap smaller than what hit_off describes and offsets
outside [0, idx_cap]; a workspace poisoned with 0x7f and with 0xff; every bad-argument call returns its code and launches nothing;
empty batches; the ops binding.  No input provokes a fault: every offset the kernels read is clamped as the header states, and a point
index outside [0, P) touches no table entry."""
import numpy as np
import pytest

from tests import point_owner_cases as pc

pytestmark = pytest.mark.gpu

CRAFTED = pc.crafted()
IDS = [c["name"] for c in CRAFTED]
GUARD = 64
I32_GUARD, F32_GUARD = 0x5A5A1234, -3.5e30
ERR_ARG, ERR_WORKSPACE = -1, -3
OUT_I32 = ("ow_owner", "ow_off", "ow_tile_off", "ow_idx", "ow_status", "ow_lost")
RULE = {"score": 0, "smallest": 1}


def _t(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _ws_bytes(F, P, M, cap):
    return 16 * M + 4 * F * P + cap


def _guarded(M, cap, ws_bytes, ws_fill=0xA5):
    """Every output of idx_cap (or M, M + 1) entries and the workspace between GUARD guard words."""
    import torch
    out = {}
    spec = dict(ow_owner=(cap, "i"), ow_off=(M + 1, "i"), ow_tile_off=(M + 1, "i"), ow_idx=(cap, "i"), ow_xyz=(4 * cap, "f"), ow_status=(M, "i"),
                ow_lost=(M, "i"), ws=((ws_bytes + 3) // 4 * 4, "b"))
    for name, (n, kind) in spec.items():
        dtype, fill = {"i": (torch.int32, I32_GUARD), "f": (torch.float32, F32_GUARD), "b": (torch.uint8, 0xA5)}[kind]
        whole = torch.full((2 * GUARD + n,), fill, dtype=dtype, device="cuda")
        out[name] = (whole, whole[GUARD:GUARD + n], fill)
    out["ws"][1].fill_(ws_fill)
    return out


def _guards_intact(bufs):
    for name, (whole, view, fill) in bufs.items():
        w, n = whole.cpu().numpy(), view.numel()
        assert (w[:GUARD] == np.array(fill).astype(w.dtype)).all() and (w[GUARD + n:] == np.array(fill).astype(w.dtype)).all(), name


def _inputs(case, pad=0, hit_off=None):
    """The lists on the device, `pad` positions of a recognisable filler behind the last (a point number inside the frame: a position
    read from there would claim)."""
    n = len(case["hit_idx"])
    x4 = np.full((n + pad + 1, 4), 7.5e20, np.float32)
    x4[:n] = case["hit_xyz"]
    i4 = np.full(n + pad + 1, 5, np.int32)
    i4[:n] = case["hit_idx"]
    M = len(case["score"])
    return dict(hit_xyz=_t(x4), hit_idx=_t(i4), hit_off=_t(np.asarray(case["hit_off"] if hit_off is None else hit_off, np.int32)),
                mask_off=_t(case["mask_off"]), score=_t(case["score"] if M else np.zeros(1)))


def _call(case, d, bufs, rule, min_keep, cap, **override):
    import torch
    from cm3d_amd import _lib
    M, F, P = len(case["score"]), len(case["mask_off"]) - 1, case["P"]
    a = dict(n_frames=F, n_masks=M, idx_cap=cap, max_pts_per_frame=P, rule=RULE[rule], min_keep=min_keep, ws_bytes=_ws_bytes(F, P, M, cap))
    a.update({k: d[k].data_ptr() for k in ("hit_xyz", "hit_idx", "hit_off", "mask_off", "score")})
    a.update({k: bufs[k][1].data_ptr() for k in OUT_I32 + ("ow_xyz", "ws")})
    a.update({k.rstrip("_"): v for k, v in override.items()})          # (rule_, min_keep_: the raw values of a bad call)
    L = _lib.lib()
    assert L.cm3d_point_owner_workspace_bytes(F, P, M, cap) == (_ws_bytes(F, P, M, cap) if M > 0 and cap > 0 else 0)
    rc = L.cm3d_point_owner(a["hit_xyz"], a["hit_idx"], a["hit_off"], a["mask_off"], a["n_frames"], a["n_masks"], a["idx_cap"],
                            a["max_pts_per_frame"], a["score"], a["rule"], a["min_keep"], a["ow_owner"], a["ow_off"], a["ow_tile_off"], a["ow_idx"],
                            a["ow_xyz"], a["ow_status"], a["ow_lost"], a["ws"], a["ws_bytes"], torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    return rc


def _assert(bufs, exp, what, cap):
    """The outputs are the host statement's, and what lies behind the lists keeps its filler."""
    k, end = int(exp["ow_off"][-1]), len(exp["ow_owner"])
    for name in ("ow_off", "ow_tile_off", "ow_status", "ow_lost"):
        g = bufs[name][1].cpu().numpy()
        assert np.array_equal(g, exp[name]), (what, name, np.flatnonzero(g != exp[name])[:8])
    own, idx, xyz = (bufs[n][1].cpu().numpy() for n in ("ow_owner", "ow_idx", "ow_xyz"))
    assert np.array_equal(own[:end], exp["ow_owner"]), (what, "ow_owner", np.flatnonzero(own[:end] != exp["ow_owner"])[:8])
    assert (own[end:] == I32_GUARD).all(), (what, "ow_owner behind the lists")
    assert np.array_equal(idx[:k], exp["ow_idx"]), (what, "ow_idx")
    assert xyz[:4 * k].tobytes() == np.ascontiguousarray(exp["ow_xyz"], np.float32).tobytes(), (what, "ow_xyz")
    assert (idx[k:] == I32_GUARD).all() and (xyz[4 * k:] == np.float32(F32_GUARD)).all(), (what, "behind the kept lists")
    assert k <= cap and end <= cap
    _guards_intact(bufs)


def _outputs(bufs):
    return {k: v[1].cpu().numpy().tobytes() for k, v in bufs.items() if k != "ws"}


@pytest.mark.parametrize("case", CRAFTED, ids=IDS)
def test_equals_the_host_statement(case):
    M, F, cap = len(case["score"]), len(case["mask_off"]) - 1, len(case["hit_idx"])
    d = _inputs(case)
    for rule, min_keep in case["runs"]:
        exp = pc.host(case, rule, min_keep)
        bufs = _guarded(M, cap, _ws_bytes(F, case["P"], M, cap))
        assert _call(case, d, bufs, rule, min_keep, cap) == 0
        _assert(bufs, exp, (rule, min_keep), cap)
        first = _outputs(bufs)
        for name in OUT_I32 + ("ow_xyz",):                       # two calls in a row: the same bytes
            bufs[name][1].fill_(I32_GUARD if name != "ow_xyz" else F32_GUARD)
        assert _call(case, d, bufs, rule, min_keep, cap) == 0
        assert _outputs(bufs) == first
        assert d["hit_idx"].cpu().numpy()[:cap].tobytes() == case["hit_idx"].tobytes()                # the raw lists stay what they were
        assert d["hit_xyz"].cpu().numpy()[:cap].tobytes() == case["hit_xyz"].tobytes()


def test_random_batches():
    lost = 0
    for case in pc.random_cases():
        (rule, min_keep), = case["runs"]
        M, F, cap = len(case["score"]), len(case["mask_off"]) - 1, max(len(case["hit_idx"]), 1)
        exp = pc.host(case, rule, min_keep)
        bufs = _guarded(max(M, 1), cap, _ws_bytes(F, case["P"], M, cap), ws_fill=0x7F if M % 2 else 0xFF)
        assert _call(case, _inputs(case), bufs, rule, min_keep, cap) == 0
        if M == 0:
            assert all((v[1].cpu().numpy() == np.array(v[2]).astype(v[1].cpu().numpy().dtype)).all() for k, v in bufs.items() if k != "ws")
            continue
        _assert(bufs, exp, case["name"], cap)
        lost += int(exp["ow_lost"].sum())
    assert lost > 5000


@pytest.mark.parametrize("name", ["claimants_65", "seam_257", "outside_the_frame", "empty_frame_between", "min_keep_kept_5"])
def test_workspace_poison(name):
    """0x7f and 0xff in every byte of the workspace -- ranks, frames and table entries above every real one, or negative -- give the
    bytes of a call on a zeroed workspace."""
    case = [c for c in CRAFTED if c["name"] == name][0]
    M, F, cap = len(case["score"]), len(case["mask_off"]) - 1, len(case["hit_idx"])
    d = _inputs(case)
    for rule, min_keep in case["runs"][:2]:
        out = []
        for fill in (0x00, 0x7F, 0xFF):
            bufs = _guarded(M, cap, _ws_bytes(F, case["P"], M, cap), ws_fill=fill)
            assert _call(case, d, bufs, rule, min_keep, cap) == 0
            _assert(bufs, pc.host(case, rule, min_keep), (rule, fill), cap)
            out.append(_outputs(bufs))
        assert out[0] == out[1] == out[2]


@pytest.mark.parametrize("name", ["claimants_33", "seam_257", "same_point_in_two_frames", "outside_the_frame"])
def test_an_idx_cap_below_what_hit_off_describes(name):
    """The call is told a capacity that ends inside a list (and in front of the lists behind it): the offsets are clamped, the lists are
    what is left of them below idx_cap, nothing at or beyond idx_cap is read -- the filler there names a point inside the frame and would
    claim it -- or written."""
    case = [c for c in CRAFTED if c["name"] == name][0]
    M, F, n = len(case["score"]), len(case["mask_off"]) - 1, len(case["hit_idx"])
    d = _inputs(case, pad=8)
    d["hit_idx"][:] = _t(np.concatenate([case["hit_idx"], np.full(9, 5, np.int32)]))
    for cap in (n - 1, n // 2 + 1, 3):
        for rule, min_keep in case["runs"][:2]:
            dd = dict(d, hit_idx=d["hit_idx"].clone(), hit_xyz=d["hit_xyz"].clone())
            dd["hit_idx"][cap:] = 5                      # beyond idx_cap: claims that would show
            dd["hit_xyz"][cap:] = 7.5e20
            bufs = _guarded(M, cap, _ws_bytes(F, case["P"], M, cap))
            assert _call(case, dd, bufs, rule, min_keep, cap) == 0
            _assert(bufs, pc.host(case, rule, min_keep, cap), (cap, rule), cap)


def test_offsets_outside_the_capacity():
    """A negative first offset, offsets beyond idx_cap and INT32_MAX: each is clamped into [0, idx_cap] first."""
    case = [c for c in CRAFTED if c["name"] == "claimants_33"][0]
    M, F, n = len(case["score"]), len(case["mask_off"]) - 1, len(case["hit_idx"])
    off = case["hit_off"].copy()
    off[0], off[-3:] = -7, [n + 5, 2 ** 31 - 1, 2 ** 31 - 1]
    for cap in (n, n - 2, 9):
        bufs = _guarded(M, cap, _ws_bytes(F, case["P"], M, cap))
        assert _call(case, _inputs(case, hit_off=off), bufs, "smallest", 1, cap) == 0
        _assert(bufs, pc.host(case, "smallest", 1, cap, off), cap, cap)


def test_argument_errors_leave_the_poison():
    """Every bad value and every NULL array: CM3D_ERR_ARG (a short workspace: CM3D_ERR_WORKSPACE).  Every output keeps its poison:
    nothing was launched.  An empty batch is CM3D_OK and launches nothing either."""
    from cm3d_amd import _lib
    case = [c for c in CRAFTED if c["name"] == "claimants_33"][0]
    M, F, cap = len(case["score"]), len(case["mask_off"]) - 1, len(case["hit_idx"])
    d, bufs = _inputs(case), _guarded(M, cap, _ws_bytes(F, case["P"], M, cap))
    bad = [dict(rule_=2), dict(rule_=-1), dict(min_keep_=0), dict(min_keep_=-4), dict(n_masks=-1), dict(n_frames=-1), dict(idx_cap=0), dict(idx_cap=-5),
           dict(max_pts_per_frame=-1)]
    bad += [{k: None} for k in ("hit_xyz", "hit_idx", "hit_off", "mask_off", "score", "ws") + OUT_I32 + ("ow_xyz",)]
    bad += [dict(hit_xyz=d["hit_xyz"].data_ptr() + 4), dict(ow_xyz=bufs["ow_xyz"][1].data_ptr() + 4), dict(ws=bufs["ws"][1].data_ptr() + 1)]
    for kw in bad:
        assert _call(case, d, bufs, "score", 5, cap, **kw) == ERR_ARG, kw
    assert _call(case, d, bufs, "score", 5, cap, n_masks=0, hit_idx=None) == ERR_ARG           # hit_idx is needed whatever M is
    assert _call(case, d, bufs, "score", 5, cap, ws_bytes=_ws_bytes(F, case["P"], M, cap) - 1) == ERR_WORKSPACE
    assert _call(case, d, bufs, "score", 5, cap, n_masks=0) == 0                               # no mask: nothing to do, nothing launched
    for name in OUT_I32:
        assert (bufs[name][1].cpu().numpy() == I32_GUARD).all(), name
    assert (bufs["ow_xyz"][1].cpu().numpy() == np.float32(F32_GUARD)).all() and (bufs["ws"][1].cpu().numpy() == 0xA5).all()
    _guards_intact(bufs)
    L = _lib.lib()
    assert [L.cm3d_point_owner_check(r, k) for r, k in ((0, 1), (1, 5), (2, 5), (-1, 5), (0, 0))] == [0, 0, ERR_ARG, ERR_ARG, ERR_ARG]
    assert L.cm3d_point_owner_workspace_bytes(2, 100, 0, 10) == 0 and L.cm3d_point_owner_workspace_bytes(2, 100, 3, 10) == 48 + 800 + 10


def test_the_ops_binding():
    from cm3d_amd import ops
    case = [c for c in CRAFTED if c["name"] == "empty_frame_between"][0]
    for rule, min_keep in case["runs"]:
        exp = pc.host(case, rule, min_keep)
        got = ops.point_owner(case["hit_xyz"], case["hit_idx"], case["hit_off"], case["mask_off"], case["score"], case["P"], rule, min_keep)
        for k in ("ow_owner", "ow_off", "ow_tile_off", "ow_status", "ow_lost", "ow_idx"):
            assert np.array_equal(got[k], exp[k]), k
        assert got["ow_xyz"].tobytes() == np.ascontiguousarray(exp["ow_xyz"], np.float32).tobytes()
    n = len(case["hit_idx"])
    got = ops.point_owner(case["hit_xyz"], case["hit_idx"], case["hit_off"], case["mask_off"], case["score"], case["P"], 1, 1, idx_cap=n - 3)
    assert np.array_equal(got["ow_owner"], pc.host(case, "smallest", 1, n - 3)["ow_owner"])
    none = ops.point_owner(np.zeros((0, 4), np.float32), [], [0], [0], [], 10)
    assert none["ow_off"].tolist() == [0] and none["ow_xyz"].shape == (0, 4) and none["ow_owner"].shape == (0,)
