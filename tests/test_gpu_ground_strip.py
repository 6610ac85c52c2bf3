"""GPU: cm3d_ground_grid and cm3d_ground_strip through the raw library calls against their host statements
(cm3d_amd.groundstrip.ground_grid_host, ground_strip_host) on every case and run of tests/ground_strip_cases.py -- every output TO THE
BIT, no tolerance: the counts are integers and the rule's float64 operations are rounded one by one on both sides --, the grid once
from the cloud the oracle's sweep preparation gives and once from the raw rows in each of the three layouts (rows of five floats, of
four, the quad layout), whose bytes must be the cloud run's; between guard words around every written array; with and without hit_idx;
an idx_cap smaller than what hit_off describes; every bad-argument call returns its code and launches nothing; empty batches; two
calls in a row.  No input provokes a fault: every offset the kernels read is clamped as the header states."""
import numpy as np
import pytest

from tests import ground_strip_cases as gc

pytestmark = pytest.mark.gpu

CASES = gc.all_cases()
IDS = [c["name"] for c in CASES]
GUARD = 64
I32_GUARD, F64_GUARD, F32_GUARD = 0x5A5A1234, -7.25e300, -3.5e30
ROUTES = ("points", "stride5", "stride4", "quads")
ERR_ARG, ERR_WORKSPACE = -1, -3


@pytest.fixture(scope="module")
def clouds(oracle):
    return {c["name"]: gc.cloud(oracle, c) for c in CASES}


@pytest.fixture(scope="module")
def host(clouds):
    return {(c["name"], n): gc.expected(c, *clouds[c["name"]], run) for c in CASES for n, run in enumerate(c["runs"])}


def _guarded(spec):
    """{name: (n, kind)} -> {name: (whole, view)}: every array between GUARD guard words."""
    import torch
    out = {}
    for name, (n, kind) in spec.items():
        dtype, fill = {"i": (torch.int32, I32_GUARD), "d": (torch.float64, F64_GUARD), "f": (torch.float32, F32_GUARD),
                       "b": (torch.uint8, 0xA5)}[kind]
        whole = torch.full((2 * GUARD + n,), fill, dtype=dtype, device="cuda")
        out[name] = (whole, whole[GUARD:GUARD + n], fill)
    return out


def _guards_intact(bufs):
    for name, (whole, view, fill) in bufs.items():
        w, n = whole.cpu().numpy(), view.numel()
        assert (w[:GUARD] == np.array(fill).astype(w.dtype)).all() and (w[GUARD + n:] == np.array(fill).astype(w.dtype)).all(), name


def _t(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _grid_inputs(case, cloud):
    pts = cloud[0] if len(cloud[0]) else np.zeros((1, 4), np.float32)
    d = dict(points=_t(pts), pt_off=_t(cloud[1]), sweep_xf=_t(gc.sweep_xf(case)), sweep_row_off=_t(case["sweep_row_off"]),
             frame_sweep_off=_t(case["frame_sweep_off"]), origin=_t(case["origin"]))
    for name, (raw, stride) in gc.raw_layouts(case).items():
        d[name] = _t(raw if raw.size else np.zeros(12, np.float32))
    d["strides"] = {name: stride for name, (_, stride) in gc.raw_layouts(case).items()}
    return d


def _grid_call(case, route, p, bufs, d, **override):
    import torch
    from cm3d_amd import _lib
    ptr = lambda k: d[k].data_ptr()
    a = dict(p, points=None, pt_off=None, raw=None, raw_stride=4, sweep_xf=ptr("sweep_xf"), sweep_row_off=ptr("sweep_row_off"),
             frame_sweep_off=ptr("frame_sweep_off"), n_sweeps=len(case["sweeps"]), halfw=case["halfw"], n_rows=int(case["sweep_row_off"][-1]),
             origin=ptr("origin"), n_frames=len(case["origin"]), grid_z=bufs["grid_z"][1].data_ptr(), grid_n=bufs["grid_n"][1].data_ptr())
    if route == "points":
        a.update(points=ptr("points"), pt_off=ptr("pt_off"))
    else:
        a.update(raw=ptr(route), raw_stride=d["strides"][route])
    a.update(override)
    rc = _lib.lib().cm3d_ground_grid(a["points"], a["pt_off"], a["raw"], a["raw_stride"], a["sweep_xf"], a["sweep_row_off"], a["frame_sweep_off"],
                                     a["n_sweeps"], a["halfw"], a["n_rows"], a["origin"], a["n_frames"], a["cell"], a["down"], a["up"], a["quantile"],
                                     a["min_points"], a["grid_z"], a["grid_n"], torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    return rc


def _strip_spec(M, cap):
    return dict(gs_off=(M + 1, "i"), gs_tile_off=(M + 1, "i"), gs_idx=(cap, "i"), gs_xyz=(4 * cap, "f"), gs_status=(M, "i"), gs_dropped=(M, "i"),
                ws=(4 * M + cap + 4, "b"))


def _strip_call(d, p, bufs, M, cap, F, with_idx=True, **override):
    import torch
    from cm3d_amd import _lib
    a = dict(p, hit_xyz=d["hit_xyz"].data_ptr(), hit_idx=d["hit_idx"].data_ptr() if with_idx else None, hit_off=d["hit_off"].data_ptr(),
             mask_frame=d["mask_frame"].data_ptr(), n_masks=M, idx_cap=cap, origin=d["origin"].data_ptr(), grid_z=d["grid_z"].data_ptr(), n_frames=F,
             gs_idx=bufs["gs_idx"][1].data_ptr() if with_idx else None, ws_bytes=4 * M + cap)
    a.update({k: bufs[k][1].data_ptr() for k in ("gs_off", "gs_tile_off", "gs_xyz", "gs_status", "gs_dropped", "ws")})
    a.update(override)
    rc = _lib.lib().cm3d_ground_strip(a["hit_xyz"], a["hit_idx"], a["hit_off"], a["mask_frame"], a["n_masks"], a["idx_cap"], a["origin"], a["grid_z"],
                                      a["n_frames"], a["cell"], a["margin"], a["min_keep"], a["gs_off"], a["gs_tile_off"], a["gs_idx"], a["gs_xyz"],
                                      a["gs_status"], a["gs_dropped"], a["ws"], a["ws_bytes"], torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    return rc


def _strip_inputs(case, points, grid_z, pad=0):
    """The lists on the device, 16-byte aligned, `pad` positions of a recognisable filler behind the last."""
    xyz, idx, off, mf = gc.lists(case, points)
    n = len(xyz)
    x4 = np.full((n + pad + 1, 4), 7.5e20, np.float32)
    x4[:n] = xyz
    i4 = np.full(n + pad + 1, 0x7A7A7A7, np.int32)
    i4[:n] = idx
    return dict(hit_xyz=_t(x4), hit_idx=_t(i4), hit_off=_t(off), mask_frame=_t(mf if len(mf) else np.zeros(1, np.int32)), origin=_t(case["origin"]),
                grid_z=_t(grid_z)), n


def _assert_strip(bufs, exp, what, with_idx=True):
    k = int(exp["gs_off"][-1])
    for name in ("gs_off", "gs_tile_off", "gs_status", "gs_dropped"):
        g = bufs[name][1].cpu().numpy()
        assert np.array_equal(g, exp[name]), (what, name, np.flatnonzero(g != exp[name])[:8])
    assert bufs["gs_xyz"][1].cpu().numpy()[:4 * k].tobytes() == exp["gs_xyz"].tobytes(), (what, "gs_xyz")
    if with_idx:
        assert np.array_equal(bufs["gs_idx"][1].cpu().numpy()[:k], exp["gs_idx"]), (what, "gs_idx")
    return k


@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_grid_equals_the_host_statement_from_the_cloud_and_from_the_raw_rows(case, clouds, host):
    F = len(case["origin"])
    bufs, d = _guarded(dict(grid_z=(F * gc.N_CELLS, "d"), grid_n=(F * gc.N_CELLS, "i"))), _grid_inputs(case, clouds[case["name"]])
    for n, run in enumerate(case["runs"]):
        exp, first = host[case["name"], n], None
        for route in ROUTES if n < 2 else ("points", "quads"):
            bufs["grid_z"][1].fill_(1.25), bufs["grid_n"][1].fill_(-77)
            assert _grid_call(case, route, gc.grid_params(run), bufs, d) == 0
            gz, gn = bufs["grid_z"][1].cpu().numpy().reshape(F, -1), bufs["grid_n"][1].cpu().numpy().reshape(F, -1)
            assert np.array_equal(gn, exp["grid_n"]), (run, route, np.argwhere(gn != exp["grid_n"])[:8])
            assert np.array_equal(gc.bits(gz), gc.bits(exp["grid_z"])), (run, route, np.argwhere(gc.bits(gz) != gc.bits(exp["grid_z"]))[:8])
            _guards_intact(bufs)
            if first is None:
                first = (gz.tobytes(), gn.tobytes())
            else:                                    # the raw runs give the bytes of the cloud's run
                assert (gz.tobytes(), gn.tobytes()) == first, route


@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_strip_equals_the_host_statement(case, clouds, host):
    points, _ = clouds[case["name"]]
    M, F = len(case["mask_frame"]), len(case["origin"])
    for n, run in enumerate(case["runs"]):
        exp = host[case["name"], n]
        d, cap = _strip_inputs(case, points, exp["grid_z"])
        for with_idx in (True, False):
            bufs = _guarded(_strip_spec(M, cap))
            assert _strip_call(d, gc.strip_params(run), bufs, M, cap, F, with_idx) == 0
            _assert_strip(bufs, exp, (run, with_idx), with_idx)
            if not with_idx:
                assert (bufs["gs_idx"][1].cpu().numpy() == I32_GUARD).all()
            first = {k: v[1].cpu().numpy().tobytes() for k, v in bufs.items() if k != "ws"}
            assert _strip_call(d, gc.strip_params(run), bufs, M, cap, F, with_idx) == 0            # two calls in a row: the same bytes
            assert first == {k: v[1].cpu().numpy().tobytes() for k, v in bufs.items() if k != "ws"}
            _guards_intact(bufs)
            assert d["hit_xyz"].cpu().numpy()[:cap].tobytes() == gc.lists(case, points)[0].tobytes()           # the raw lists stay what they were


def test_two_grid_calls_give_the_same_bytes(clouds):
    case = CASES[1]
    F = len(case["origin"])
    bufs, d = _guarded(dict(grid_z=(F * gc.N_CELLS, "d"), grid_n=(F * gc.N_CELLS, "i"))), _grid_inputs(case, clouds[case["name"]])
    out = []
    for _ in range(2):
        assert _grid_call(case, "stride5", gc.grid_params({}), bufs, d) == 0
        out.append((bufs["grid_z"][1].cpu().numpy().tobytes(), bufs["grid_n"][1].cpu().numpy().tobytes()))
    assert out[0] == out[1]


@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_an_idx_cap_below_what_hit_off_describes(case, clouds, host):
    """The call is told a capacity that ends inside a list (and in front of the lists behind it): the offsets are clamped, the lists are
    what is left of them below idx_cap, nothing at or beyond idx_cap is read -- the filler there would show in the result -- or written."""
    points, _ = clouds[case["name"]]
    xyz, idx, off, mf = gc.lists(case, points)
    M, F, n = len(mf), len(case["origin"]), len(xyz)
    exp_grid = host[case["name"], 0]["grid_z"]
    from cm3d_amd import groundstrip as gs
    for cap in (n - 1, n // 2 + 1, 3):
        cut = np.minimum(off, cap)
        e_off, e_tile, keep, status, dropped = gs.strip_lists(cut, xyz[:cap], mf, case["origin"], exp_grid)
        exp = dict(gs_off=e_off, gs_tile_off=e_tile, gs_status=status, gs_dropped=dropped, gs_xyz=xyz[:cap][keep], gs_idx=idx[:cap][keep])
        d, _ = _strip_inputs(case, points, exp_grid)
        d["hit_xyz"][cap:] = 7.5e20                   # beyond idx_cap: points that would be kept and would show
        bufs = _guarded(_strip_spec(M, cap))          # outputs of idx_cap entries between guards: nothing beyond is written
        assert _strip_call(d, gc.strip_params({}), bufs, M, cap, F) == 0
        _assert_strip(bufs, exp, cap)
        assert int(e_off[-1]) <= cap
        _guards_intact(bufs)


def test_the_ops_bindings(clouds, host):
    from cm3d_amd import ops
    case = CASES[1]
    points, pt_off = clouds[case["name"]]
    exp = host[case["name"], 0]
    gz, gn = ops.ground_grid(case["origin"], points=points, pt_off=pt_off)
    assert np.array_equal(gc.bits(gz), gc.bits(exp["grid_z"])) and np.array_equal(gn, exp["grid_n"])
    raw, stride = gc.raw_layouts(case)["quads"]
    gz2, gn2 = ops.ground_grid(case["origin"], raw=raw, raw_stride=stride, sweep_xf=gc.sweep_xf(case), sweep_row_off=case["sweep_row_off"],
                               frame_sweep_off=case["frame_sweep_off"], halfw=case["halfw"])
    assert gz2.tobytes() == gz.tobytes() and gn2.tobytes() == gn.tobytes()
    xyz, idx, off, mf = gc.lists(case, points)
    got = ops.ground_strip(xyz, off, mf, case["origin"], gz, hit_idx=idx)
    for k in ("gs_off", "gs_tile_off", "gs_status", "gs_dropped", "gs_idx"):
        assert np.array_equal(got[k], exp[k]), k
    assert got["gs_xyz"].tobytes() == exp["gs_xyz"].tobytes()
    assert ops.ground_strip(xyz, off, mf, case["origin"], gz)["gs_idx"] is None
    none = ops.ground_strip(np.zeros((0, 4), np.float32), [0], [], case["origin"], gz)
    assert none["gs_off"].tolist() == [0] and none["gs_xyz"].shape == (0, 4)
    z0, n0 = ops.ground_grid(np.zeros((0, 3)), points=np.zeros((0, 4), np.float32), pt_off=[0])
    assert z0.shape == (0, gc.N_CELLS) and n0.shape == (0, gc.N_CELLS)


def test_argument_errors_leave_the_poison(clouds, host):
    """Every bad value and every NULL array: CM3D_ERR_ARG (a short workspace: CM3D_ERR_WORKSPACE).  Every output keeps its poison:
    nothing was launched.  Empty batches are CM3D_OK and launch nothing either."""
    case = CASES[0]
    points, _ = clouds[case["name"]]
    F, M = len(case["origin"]), len(case["mask_frame"])
    nan, inf = float("nan"), float("inf")
    bufs, d = _guarded(dict(grid_z=(F * gc.N_CELLS, "d"), grid_n=(F * gc.N_CELLS, "i"))), _grid_inputs(case, clouds[case["name"]])
    bufs["grid_z"][1].fill_(42.0), bufs["grid_n"][1].fill_(42)
    p = gc.grid_params({})
    bad = [dict(cell=0.0), dict(cell=-2.0), dict(cell=nan), dict(cell=inf), dict(down=0.0), dict(down=-1.0), dict(down=nan), dict(down=inf),
           dict(up=0.0), dict(up=nan), dict(up=inf), dict(quantile=-0.01), dict(quantile=1.0000001), dict(quantile=nan), dict(min_points=0),
           dict(min_points=-3), dict(n_frames=-1), dict(n_rows=-1), dict(n_sweeps=-1), dict(origin=None), dict(grid_z=None), dict(grid_n=None)]
    for kw in bad:
        for route in ("points", "quads"):
            assert _grid_call(case, route, p, bufs, d, **kw) == ERR_ARG, (kw, route)
    assert _grid_call(case, "points", p, bufs, d, points=None) == ERR_ARG and _grid_call(case, "points", p, bufs, d, pt_off=None, sweep_xf=None) == ERR_ARG
    for k in ("raw", "sweep_xf", "sweep_row_off", "frame_sweep_off"):
        assert _grid_call(case, "stride5", p, bufs, d, **{k: None}) == ERR_ARG, k
    for stride in (0, 1, 2, -4):
        assert _grid_call(case, "stride5", p, bufs, d, raw_stride=stride) == ERR_ARG, stride
    assert _grid_call(case, "points", p, bufs, d, points=d["points"].data_ptr() + 4) == ERR_ARG
    assert _grid_call(case, "points", p, bufs, d, n_frames=0) == 0                # no frame: nothing to do, nothing launched
    assert (bufs["grid_z"][1].cpu().numpy() == 42.0).all() and (bufs["grid_n"][1].cpu().numpy() == 42).all()
    _guards_intact(bufs)

    exp = host[case["name"], 0]
    d, cap = _strip_inputs(case, points, exp["grid_z"])
    bufs = _guarded(_strip_spec(M, cap))
    for k in ("gs_off", "gs_tile_off", "gs_idx", "gs_status", "gs_dropped"):
        bufs[k][1].fill_(42)
    bufs["gs_xyz"][1].fill_(42.0)
    p = gc.strip_params({})
    bad = [dict(cell=0.0), dict(cell=nan), dict(cell=inf), dict(margin=nan), dict(margin=inf), dict(margin=-inf), dict(min_keep=0), dict(min_keep=-1),
           dict(n_masks=-1), dict(idx_cap=0), dict(idx_cap=-5), dict(n_frames=-1), dict(hit_idx=None), dict(gs_idx=None), dict(origin=None),
           dict(grid_z=None)]
    bad += [{k: None} for k in ("hit_xyz", "hit_off", "mask_frame", "gs_off", "gs_tile_off", "gs_xyz", "gs_status", "gs_dropped", "ws")]
    bad += [dict(hit_xyz=d["hit_xyz"].data_ptr() + 4), dict(gs_xyz=bufs["gs_xyz"][1].data_ptr() + 4), dict(ws=bufs["ws"][1].data_ptr() + 1)]
    for kw in bad:
        assert _strip_call(d, p, bufs, M, cap, F, **kw) == ERR_ARG, kw
    assert _strip_call(d, p, bufs, M, cap, F, ws_bytes=4 * M + cap - 1) == ERR_WORKSPACE
    assert _strip_call(d, p, bufs, M, cap, F, n_masks=0) == 0                     # no mask: nothing to do, nothing launched
    for k in ("gs_off", "gs_tile_off", "gs_idx", "gs_status", "gs_dropped"):
        assert (bufs[k][1].cpu().numpy() == 42).all(), k
    assert (bufs["gs_xyz"][1].cpu().numpy() == 42.0).all()
    # no frame: every frame number is out of range, the strip is the identity (origin and grid_z may be NULL)
    assert _strip_call(d, dict(p, min_keep=1), bufs, M, cap, 0, origin=None, grid_z=None) == 0
    xyz, idx, off, mf = gc.lists(case, points)
    assert np.array_equal(bufs["gs_off"][1].cpu().numpy(), off) and bufs["gs_xyz"][1].cpu().numpy().tobytes() == xyz.tobytes()
    assert np.array_equal(bufs["gs_idx"][1].cpu().numpy(), idx) and not bufs["gs_dropped"][1].cpu().numpy().any()
    _guards_intact(bufs)
