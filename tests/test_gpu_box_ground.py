"""GPU: cm3d_box_ground through the raw library call against its host statement (cm3d_amd.boxground.box_ground_host) on every case and
run of tests/box_ground_cases.py -- all six outputs and box TO THE BIT, no tolerance: the counts are integers and the rule's float64
operations are rounded one by one on both sides --, once from the cloud the oracle's sweep preparation gives and once from the raw rows
in each of the three layouts (rows of five floats, of four, the quad layout), whose bytes must be the cloud run's; between guard words
around every written array; columns other than 2 of box and flags the input's bytes; a second call with zref = ground_zref in the very
array it is written to; every bad-argument call returns its code and launches nothing.  No input provokes a fault: every offset the
kernel reads is clamped as the header states."""
import numpy as np
import pytest

from cm3d_amd import boxground as bg
from tests import box_ground_cases as gc

pytestmark = pytest.mark.gpu

CASES = gc.all_cases()
IDS = [c["name"] for c in CASES]
GUARD = 64
I32_GUARD, F64_GUARD = 0x5A5A1234, -7.25e300
ARRAYS = (("ground_z", 1, "d"), ("ground_n", 1, "i"), ("ground_h", 1, "d"), ("ground_src", 1, "i"), ("ground_status", 1, "i"),
          ("ground_zref", 1, "d"), ("box", gc.BOX_STRIDE, "d"))
PURE = ARRAYS[:6]
ROUTES = ("points", "stride5", "stride4", "quads")


@pytest.fixture(scope="module")
def clouds(oracle):
    return {c["name"]: gc.cloud(oracle, c) for c in CASES}


@pytest.fixture(scope="module")
def host(clouds):
    return {(c["name"], n): bg.box_ground_host(*clouds[c["name"]], c["mask_off"], c["box"], c["flags"], c["prior_wlh"], zref=c["zref"],
                                               vert=c["vert"], **gc.params(run)) for c in CASES for n, run in enumerate(c["runs"])}


def _guarded(M):
    import torch
    out = {}
    for name, width, kind in ARRAYS:
        dtype, fill = (torch.int32, I32_GUARD) if kind == "i" else (torch.float64, F64_GUARD)
        whole = torch.full((2 * GUARD + M * width,), fill, dtype=dtype, device="cuda")
        out[name] = (whole, whole[GUARD:GUARD + M * width])
    return out


def _guards_intact(bufs):
    for name, width, kind in ARRAYS:
        whole, view = bufs[name]
        w = whole.cpu().numpy()
        fill = I32_GUARD if kind == "i" else F64_GUARD
        n = view.numel()
        assert (w[:GUARD] == fill).all() and (w[GUARD + n:] == fill).all(), name


def _poison(bufs):
    for name, _, kind in PURE:
        bufs[name][1].fill_(12345 if kind == "i" else float("nan"))


def _device_inputs(case, cloud):
    """Everything the call reads, on the device: the cloud, the raw rows in the three layouts, the offsets and the per-mask inputs."""
    import torch
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda()
    pts = cloud[0] if len(cloud[0]) else np.zeros((1, 4), np.float32)
    d = dict(points=t(pts), pt_off=t(cloud[1]), sweep_xf=t(gc.sweep_xf(case) if case["sweeps"] else np.zeros((1, 24), np.float32)),
             sweep_row_off=t(case["sweep_row_off"]), frame_sweep_off=t(case["frame_sweep_off"]), mask_off=t(case["mask_off"]),
             flags=t(case["flags"]), prior_wlh=t(case["prior_wlh"]))
    for name, (raw, stride) in gc.raw_layouts(case).items():
        d[name] = t(raw if raw.size else np.zeros(12, np.float32))
    d["strides"] = {name: stride for name, (_, stride) in gc.raw_layouts(case).items()}
    if case["zref"] is not None:
        d["zref"] = t(case["zref"])
    if case["vert"] is not None:
        d["vert_status"], d["vert_z"], d["vert_h"] = t(case["vert"]["vert_status"]), t(case["vert"]["vert_z"]), t(case["vert"]["vert_h"])
    return d


def _raw_call(case, route, p, bufs, d, fill=True, **override):
    """cm3d_box_ground through ctypes on the guarded arrays (box filled from the case unless fill is False): the return code.  route: the
    cloud (`points`) or one of the raw layouts.  override: arguments of the call to replace (a pointer by None)."""
    import torch
    from cm3d_amd import _lib
    L = _lib.lib()
    M = len(case["flags"])
    if fill:
        bufs["box"][1].copy_(torch.from_numpy(case["box"].reshape(-1)).cuda())
    ptr = lambda k: d[k].data_ptr() if k in d else None
    a = dict(p, n_masks=M, n_frames=len(case["mask_off"]) - 1, n_classes=case["prior_wlh"].shape[0], n_sweeps=len(case["sweeps"]),
             n_rows=int(case["sweep_row_off"][-1]), halfw=case["halfw"], max_masks_per_frame=int(np.diff(case["mask_off"]).max()),
             points=None, pt_off=None, raw=None, raw_stride=4, sweep_xf=ptr("sweep_xf"), sweep_row_off=ptr("sweep_row_off"),
             frame_sweep_off=ptr("frame_sweep_off"), mask_off=ptr("mask_off"), flags=ptr("flags"), prior_wlh=ptr("prior_wlh"), zref=ptr("zref"),
             vert_status=ptr("vert_status"), vert_z=ptr("vert_z"), vert_h=ptr("vert_h"))
    if route == "points":
        a.update(points=ptr("points"), pt_off=ptr("pt_off"))
    else:
        a.update(raw=ptr(route), raw_stride=d["strides"][route])
    a.update({name: bufs[name][1].data_ptr() for name, _, _ in ARRAYS})
    a.update(override)
    rc = L.cm3d_box_ground(a["points"], a["pt_off"], a["raw"], a["raw_stride"], a["sweep_xf"], a["sweep_row_off"], a["frame_sweep_off"], a["n_sweeps"],
                           a["halfw"], a["n_rows"], a["mask_off"], a["n_frames"], a["n_masks"], a["max_masks_per_frame"], a["box"], a["flags"],
                           a["prior_wlh"], a["n_classes"], a["zref"], a["vert_status"], a["vert_z"], a["vert_h"], a["radius"], a["quantile"],
                           a["min_points"], a["down"], a["up"], a["lo"], a["hi"], a["ground_z"], a["ground_n"], a["ground_h"], a["ground_src"],
                           a["ground_status"], a["ground_zref"], torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    return rc


def _read(bufs, M):
    out = {}
    for name, width, _ in ARRAYS:
        a = bufs[name][1].cpu().numpy()
        out[name] = a.reshape(M, width) if width > 1 else a
    return out


@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_device_equals_the_host_statement_from_the_cloud_and_from_the_raw_rows(case, clouds, host):
    M = len(case["flags"])
    bufs, d = _guarded(M), _device_inputs(case, clouds[case["name"]])
    others = [c for c in range(gc.BOX_STRIDE) if c != 2]
    for n, run in enumerate(case["runs"]):
        p, exp = gc.params(run), host[case["name"], n]
        first = None
        for route in ROUTES:
            _poison(bufs)
            assert _raw_call(case, route, p, bufs, d) == 0
            got = _read(bufs, M)
            gc.assert_same(got, exp, (case["name"], run, route))
            assert got["box"][:, others].tobytes() == case["box"][:, others].tobytes()
            assert np.array_equal(d["flags"].cpu().numpy(), case["flags"])
            _guards_intact(bufs)
            if first is None:
                first = got
            else:                                    # the raw runs give the bytes of the cloud's run
                assert all(got[k].tobytes() == first[k].tobytes() for k in first), route
        if n < 2:
            # a second call on what the first left, with zref = ground_zref in the very array it is written to: the same arrays
            keep = {k: v.copy() for k, v in got.items()}
            for name, _, kind in PURE:
                if name != "ground_zref":
                    bufs[name][1].fill_(12345 if kind == "i" else float("nan"))
            assert _raw_call(case, "quads", p, bufs, d, fill=False, zref=bufs["ground_zref"][1].data_ptr()) == 0
            again = _read(bufs, M)
            assert all(again[k].tobytes() == keep[k].tobytes() for k in keep)
            _guards_intact(bufs)


def test_an_understated_max_masks_per_frame_is_still_computed(clouds, host):
    """The header: max_masks_per_frame sizes the grid, and a frame with more masks is computed by its workgroups in turn.  Told 20 and
    8, the launch of the 128-frame shape takes chunks of 10 and 8 and one and two workgroups less per frame than the frame of 130
    needs: the same bytes as with the true count."""
    from cm3d_amd import _lib
    case = next(k for k in CASES if k["name"] == "many_chunk64")
    M = len(case["flags"])
    bufs, d = _guarded(M), _device_inputs(case, clouds[case["name"]])
    L = _lib.lib()
    for told, chunk in ((20, 10), (8, 8), (1, 8), (0, 64)):
        assert int(L.cm3d_box_ground_chunk(len(case["mask_off"]) - 1, told)) == chunk
        for route in ("points", "quads"):
            _poison(bufs)
            assert _raw_call(case, route, gc.params({}), bufs, d, max_masks_per_frame=told) == 0
            gc.assert_same(_read(bufs, M), host[case["name"], 0], (told, route))
            _guards_intact(bufs)


def test_the_ops_binding_and_an_empty_batch(clouds):
    from cm3d_amd import ops
    c = next(k for k in CASES if k["name"] == "many")
    pts, pt_off = clouds["many"]
    exp = bg.box_ground_host(pts, pt_off, c["mask_off"], c["box"], c["flags"], c["prior_wlh"], zref=c["zref"], vert=c["vert"])
    got = ops.box_ground(c["box"], c["flags"], c["prior_wlh"], c["mask_off"], points=pts, pt_off=pt_off, zref=c["zref"], vert=c["vert"])
    gc.assert_same(got, exp, "points")
    raw, stride = gc.raw_layouts(c)["quads"]
    got = ops.box_ground(c["box"], c["flags"], c["prior_wlh"], c["mask_off"], raw=raw, raw_stride=stride, sweep_xf=gc.sweep_xf(c),
                         sweep_row_off=c["sweep_row_off"], frame_sweep_off=c["frame_sweep_off"], halfw=c["halfw"], zref=c["zref"],
                         vert=c["vert"], zref_aliases=True)
    gc.assert_same(got, exp, "quads")
    none = ops.box_ground(np.zeros((0, gc.BOX_STRIDE)), [], c["prior_wlh"], [0, 0], points=np.zeros((0, 4), np.float32), pt_off=[0, 0])
    assert all(v.shape[0] == 0 for v in none.values())


def test_argument_errors_leave_the_poison(clouds):
    """Every bad value and every NULL array: CM3D_ERR_ARG.  Every pure output keeps its poison and box its bytes: nothing was launched."""
    case = next(k for k in CASES if k["name"] == "apply")
    M = len(case["flags"])
    bufs, d = _guarded(M), _device_inputs(case, clouds["apply"])
    ERR_ARG = -1
    for name, _, _ in PURE:
        bufs[name][1].fill_(42)
    nan, inf = float("nan"), float("inf")
    p = dict(gc.DEFAULTS)
    bad = [dict(radius=0.0), dict(radius=-3.0), dict(radius=nan), dict(radius=inf), dict(quantile=-0.01), dict(quantile=1.0000001), dict(quantile=nan),
           dict(min_points=0), dict(min_points=-3), dict(down=0.0), dict(down=-1.0), dict(down=nan), dict(down=inf), dict(up=-0.01), dict(up=nan),
           dict(up=inf), dict(lo=0.0), dict(lo=-1.0), dict(lo=nan), dict(hi=nan), dict(hi=inf), dict(lo=1.3, hi=0.7),
           dict(n_masks=-1), dict(n_frames=-1), dict(n_rows=-1), dict(n_sweeps=-1), dict(n_classes=-1), dict(n_classes=0), dict(max_masks_per_frame=-1),
           dict(n_frames=0), dict(vert_z=None), dict(vert_status=None, vert_z=None)]
    bad += [{k: None} for k in ("mask_off", "box", "flags", "prior_wlh", "ground_z", "ground_n", "ground_h", "ground_src", "ground_status", "ground_zref")]
    for kw in bad:
        for route in ("points", "quads"):
            assert _raw_call(case, route, p, bufs, d, **kw) == ERR_ARG, (kw, route)
    # neither a cloud nor raw rows; raw rows without their tables; a stride that is no layout
    assert _raw_call(case, "points", p, bufs, d, points=None) == ERR_ARG and _raw_call(case, "points", p, bufs, d, pt_off=None, sweep_xf=None) == ERR_ARG
    for k in ("raw", "sweep_xf", "sweep_row_off", "frame_sweep_off"):
        assert _raw_call(case, "stride5", p, bufs, d, **{k: None}) == ERR_ARG, k
    for stride in (0, 1, 2, -4):
        assert _raw_call(case, "stride5", p, bufs, d, raw_stride=stride) == ERR_ARG, stride
    for name, _, _ in PURE:
        assert (bufs[name][1].cpu().numpy() == 42).all(), name
    assert _read(bufs, M)["box"].tobytes() == case["box"].tobytes()
    _guards_intact(bufs)
    assert _raw_call(case, "points", p, bufs, d, n_masks=0) == 0                 # no mask: nothing to do, nothing launched
    assert (bufs["ground_src"][1].cpu().numpy() == 42).all()
    assert _raw_call(case, "points", p, bufs, d) == 0                            # and the same arguments, whole, run
    assert not (bufs["ground_src"][1].cpu().numpy() == 42).any()
    _guards_intact(bufs)
