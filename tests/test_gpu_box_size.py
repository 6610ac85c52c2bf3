"""GPU: cm3d_box_size through the raw library call against its host statement (cm3d_amd.boxsize.box_size_host) on every rule table and
hostile case of tests/box_size_cases.py with every run of the case -- all six outputs, box and status TO THE BIT, no tolerance: the
rule has no library call and float64 division is correctly rounded on both sides; a NaN counts as the host's NaN, whose sign and
payload IEEE 754 leaves open --, between guard words around every written array
and behind the workspace; columns 2 to 9 and flags the input's bytes; the hostile cases end with their pinned status and intact
guards (well-formed launches that must terminate); a second call on the arrays the first one left; the identity with lo = hi = 1
against the device outputs of cm3d_box_velocity and cm3d_box_tracks themselves; every bad-argument call returns its code and
launches nothing."""
import numpy as np
import pytest

from cm3d_amd import boxsize as bs
from tests import box_size_cases as sc

pytestmark = pytest.mark.gpu

CASES = sc.all_cases()
IDS = [c["name"] for c in CASES]
GUARD = 64
I32_GUARD, F64_GUARD = 0x5A5A1234, -7.25e300
WS_GUARD = 4096
ARRAYS = (("size_wlh", 3, "d"), ("size_src", 1, "i"), ("size_ratio", 2, "d"), ("size_obs", 2, "i"), ("size_placed", 2, "d"), ("size_vel", 2, "d"),
          ("box", sc.BOX_STRIDE, "d"), ("flags", 1, "i"))
PURE = ARRAYS[:6]
DEFAULTS = dict(thin=sc.THIN, max_dt=sc.MAX_DT, smooth_window=0, q=0.75, min_obs=2, lo=0.6, hi=1.5)


@pytest.fixture(scope="module")
def host():
    return {(c["name"], n): bs.box_size_host(*sc.args_of(c), **dict(DEFAULTS, **run)) for c in CASES for n, run in enumerate(c["runs"])}


def _guarded(M):
    import torch
    out = {}
    for name, width, kind in ARRAYS:
        dtype, fill = (torch.int32, I32_GUARD) if kind == "i" else (torch.float64, F64_GUARD)
        whole = torch.full((2 * GUARD + max(M, 1) * width,), fill, dtype=dtype, device="cuda")
        out[name] = (whole, whole[GUARD:GUARD + max(M, 1) * width])
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


def _device_inputs(case):
    import torch
    M = len(case["flags"])
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a if a.size else np.zeros(1, a.dtype))).cuda()
    d = {k: t(case[k]) for k in ("mask_frame", "place_src", "next_match", "prev_match", "track_id", "track_pos", "track_len", "frame_time", "prior_wlh")}
    d["fit_rect"] = t(case["fit_rect"].reshape(-1) if M else np.zeros(6))
    d["ego_xyz"] = None if case["ego_xyz"] is None else t(case["ego_xyz"])
    return d


def _raw_call(case, run, bufs, d=None, fill=True, ws_extra=WS_GUARD, **override):
    """cm3d_box_size through ctypes on the guarded arrays (box and flags filled from the case unless fill is False), the workspace
    followed by guard bytes: (return code, status).  override: arguments of the call to replace (a pointer by None)."""
    import torch
    from cm3d_amd import _lib
    L = _lib.lib()
    M, F = len(case["flags"]), len(case["frame_time"])
    d = d or _device_inputs(case)
    if M and fill:
        bufs["box"][1].copy_(torch.from_numpy(case["box"].reshape(-1)).cuda()); bufs["flags"][1].copy_(torch.from_numpy(case["flags"]).cuda())
    status = torch.zeros(1, dtype=torch.int32, device="cuda")
    ws_bytes = int(L.cm3d_box_size_workspace_bytes(M))
    ws = torch.full((ws_bytes + ws_extra,), 0xA5, dtype=torch.uint8, device="cuda")
    a = dict(DEFAULTS, **run)
    a.update(n_masks=M, n_frames=F, n_classes=case["prior_wlh"].shape[0], waymo=int(case["ego_xyz"] is None), ws=ws.data_ptr(), ws_bytes=ws_bytes,
             status=status.data_ptr(), ego_xyz=None if d["ego_xyz"] is None else d["ego_xyz"].data_ptr())
    a.update({k: d[k].data_ptr() for k in d if k != "ego_xyz"})
    a.update({name: bufs[name][1].data_ptr() for name, _, _ in ARRAYS})
    a.update(override)
    rc = L.cm3d_box_size(a["box"], a["flags"], a["mask_frame"], a["fit_rect"], a["place_src"], a["prior_wlh"], a["n_classes"], a["ego_xyz"],
                         a["waymo"], a["thin"], a["next_match"], a["prev_match"], a["track_id"], a["track_pos"], a["track_len"], a["frame_time"],
                         a["n_masks"], a["n_frames"], a["max_dt"], a["smooth_window"], a["q"], a["min_obs"], a["lo"], a["hi"], a["size_wlh"],
                         a["size_src"], a["size_ratio"], a["size_obs"], a["size_placed"], a["size_vel"], a["status"], a["ws"], a["ws_bytes"],
                         torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    assert (ws[ws_bytes:].cpu().numpy() == 0xA5).all(), "bytes behind the workspace"
    return rc, int(status.item())


def _read(bufs, M, status):
    out = dict(status=status)
    for name, width, _ in ARRAYS:
        a = bufs[name][1].cpu().numpy()[:M * width]
        out[name] = a.reshape(M, width) if width > 1 else a
    return out


@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_device_equals_the_host_statement(case, host):
    M = len(case["flags"])
    bufs, d = _guarded(M), _device_inputs(case)
    for n, run in enumerate(case["runs"]):
        exp = host[case["name"], n]
        _poison(bufs)
        rc, status = _raw_call(case, run, bufs, d)
        assert rc == 0 and status == case["status"]
        got = _read(bufs, M, status)
        sc.assert_same(got, exp, (case["name"], run))
        assert got["box"][:, 2:].tobytes() == case["box"][:, 2:].tobytes() and np.array_equal(got["flags"], case["flags"])
        _guards_intact(bufs)
        if n == 0:
            # a second call on the arrays the first one left: the same box, and the entry centres are now the first call's
            _poison(bufs)
            rc, status2 = _raw_call(case, run, bufs, d, fill=False)
            again = _read(bufs, M, status2)
            assert rc == 0 and status2 == status and again["box"].tobytes() == got["box"].tobytes()
            assert again["size_placed"].tobytes() == got["box"][:, :2].tobytes() and again["size_wlh"].tobytes() == got["size_wlh"].tobytes()
            assert np.array_equal(sc._bits(again["size_vel"]), sc._bits(got["size_vel"]))
            _guards_intact(bufs)


def test_closed_form_answers_on_the_device():
    from cm3d_amd import ops
    c = sc.by_name("dyadic_exact_velocity_and_a_span_over_max_dt")
    for W, vel in c["expect"]["vel"].items():
        got = ops.box_size(*sc.args_of(c), thin=sc.THIN, max_dt=sc.MAX_DT, smooth_window=W)
        assert np.array_equal(got["size_vel"], np.asarray(vel, np.float64)) and (got["size_wlh"][:9] == c["expect"]["wlh"]).all()
    c = sc.by_name("equal_ratios_position_decides")
    for q, r in c["expect"]["ratio_by_q"].items():
        assert (ops.box_size(*sc.args_of(c), thin=sc.THIN, max_dt=sc.MAX_DT, q=q)["size_ratio"] == list(r)).all()


def test_identity_against_the_velocity_and_the_track_stage_on_the_device():
    """lo = hi = 1 on extents that never equal the prior: nothing is observed, box keeps its bytes, the sizes are the prior rows, and
    size_vel is what cm3d_box_velocity (W = 0) and cm3d_box_tracks (W = 1, 3) themselves wrote for the same arrays."""
    from cm3d_amd import ops
    c = sc.chain_case()
    v = ops.box_velocity(c["box"], c["flags"], c["mask_off"], c["class_id"], c["frame_next"], c["frame_time"], c["track_group"], c["max_speed"],
                         sc.MAX_DT)
    assert v["status"] == 0 and np.array_equal(v["next_match"], c["next_match"])
    for W in (0, 1, 3):
        tr = ops.box_tracks(c["box"], c["flags"], c["mask_frame"], v["next_match"], v["prev_match"], c["frame_time"], smooth_window=W)
        got = ops.box_size(c["box"], c["flags"], c["mask_frame"], c["fit_rect"], c["place_src"], c["prior_wlh"], c["ego_xyz"], v["next_match"],
                           v["prev_match"], tr["track_id"], tr["track_pos"], tr["track_len"], c["frame_time"], thin=sc.THIN, max_dt=sc.MAX_DT,
                           smooth_window=W, lo=1.0, hi=1.0)
        assert got["status"] == 0 and got["box"].tobytes() == c["box"].tobytes() and not got["size_src"].any()
        assert got["size_wlh"].tobytes() == c["prior_wlh"][c["class_id"]].tobytes()
        assert got["size_vel"].tobytes() == (tr["vel_smooth"] if W else v["vel"]).tobytes(), W
    for case in sc.identity_cases()[:2]:
        for W in (1, 3):
            tr = ops.box_tracks(case["box"], case["flags"], case["mask_frame"], case["next_match"], case["prev_match"], case["frame_time"], smooth_window=W)
            got = ops.box_size(*sc.args_of(case), thin=sc.THIN, max_dt=sc.MAX_DT, smooth_window=W, lo=1.0, hi=1.0)
            assert got["box"].tobytes() == case["box"].tobytes() and got["size_vel"].tobytes() == tr["vel_smooth"].tobytes()


def test_argument_and_workspace_errors_leave_the_poison():
    """Every bad value and every NULL array: CM3D_ERR_ARG; a workspace one byte short or NULL: CM3D_ERR_WORKSPACE.  Every pure output
    keeps its poison and box its bytes: nothing was launched."""
    import torch
    from cm3d_amd import _lib
    case = sc.by_name("place_src_0_head_inside_end")
    M = len(case["flags"])
    bufs, d = _guarded(M), _device_inputs(case)
    ERR_ARG, ERR_WS = -1, -3
    ws_bytes = int(_lib.lib().cm3d_box_size_workspace_bytes(M))
    assert ws_bytes == M * 52
    for name, _, kind in PURE:
        bufs[name][1].fill_(42)
    nan, inf = float("nan"), float("inf")
    bad = [dict(n_masks=-1), dict(n_frames=0), dict(n_frames=-2), dict(n_classes=0), dict(q=-0.25), dict(q=1.0000001), dict(q=nan), dict(min_obs=0),
           dict(min_obs=-1), dict(lo=0.0), dict(lo=-1.0), dict(lo=nan), dict(hi=nan), dict(hi=inf), dict(lo=1.5, hi=0.6), dict(thin=-0.5), dict(thin=inf),
           dict(thin=nan), dict(max_dt=0.0), dict(max_dt=nan), dict(smooth_window=-1), dict(ego_xyz=None)]
    bad += [{k: None} for k in ("box", "flags", "mask_frame", "fit_rect", "place_src", "prior_wlh", "next_match", "prev_match", "track_id", "track_pos",
                                "track_len", "frame_time", "size_wlh", "size_src", "size_ratio", "size_obs", "size_placed", "size_vel", "status")]
    for kw in bad:
        rc, status = _raw_call(case, {}, bufs, d, **kw)
        assert rc == ERR_ARG and status == 0, kw
    assert _raw_call(case, {}, bufs, d, ws_bytes=ws_bytes - 1)[0] == ERR_WS and _raw_call(case, {}, bufs, d, ws=None)[0] == ERR_WS
    torch.cuda.synchronize()
    for name, _, _ in PURE:
        assert (bufs[name][1].cpu().numpy() == 42).all(), name
    got = _read(bufs, M, 0)
    assert np.array_equal(got["flags"], case["flags"]) and got["box"].tobytes() == case["box"].tobytes()
    _guards_intact(bufs)
    assert _raw_call(case, {}, bufs, d) == (0, 0)                              # and the same arguments, whole, run
    assert not (bufs["size_src"][1].cpu().numpy() == 42).any()
    assert _raw_call(case, {}, bufs, d, waymo=1, ego_xyz=None)[0] == 0         # the Waymo form needs no ego_xyz
