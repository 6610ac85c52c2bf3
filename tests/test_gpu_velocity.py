"""GPU: cm3d_box_velocity (ops.box_velocity) against its host statement (cm3d_amd.velocity.track_velocity_host) on every case of
tests/velocity_cases.py -- matches and vel_src exact, velocities to the bit --, with guard words around every output, a poisoned
second call, the status of a bad frame_next, and the argument errors that must return before any launch."""
import numpy as np
import pytest

from cm3d_amd import velocity as V
from tests import velocity_cases as vc

pytestmark = pytest.mark.gpu

CASES = vc.all_cases()
IDS = [c["name"] for c in CASES]
GUARD = 64                      # words in front of and behind every output
I32_GUARD, F64_GUARD = 0x5A5A1234, -7.25e300


@pytest.fixture(scope="module")
def host():
    return {c["name"]: V.track_velocity_host(*vc.args_of(c)) for c in CASES}


def _guarded(M):
    """Device outputs of M masks inside guard words: name -> (whole tensor, the view cm3d_box_velocity writes)."""
    import torch
    out = {}
    for name, width, dtype, fill in (("next_match", 1, torch.int32, I32_GUARD), ("prev_match", 1, torch.int32, I32_GUARD),
                                     ("vel_src", 1, torch.int32, I32_GUARD), ("vel", 2, torch.float64, F64_GUARD)):
        whole = torch.full((2 * GUARD + max(M, 1) * width,), fill, dtype=dtype, device="cuda")
        out[name] = (whole, whole[GUARD:GUARD + max(M, 1) * width])
    return out


def _guards_intact(bufs, M):
    for name, (whole, view) in bufs.items():
        w = whole.cpu().numpy()
        fill = F64_GUARD if name == "vel" else I32_GUARD
        n = view.numel() if M else 0
        assert (w[:GUARD] == fill).all() and (w[GUARD + n:] == fill).all(), name


def _assert_equal(got, exp):
    for k in ("next_match", "prev_match", "vel_src"):
        assert np.array_equal(got[k], exp[k]), k
    assert got["vel"].tobytes() == exp["vel"].tobytes()
    assert got["status"] == exp["status"]


@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_device_equals_the_host_statement(case, host):
    import torch
    from cm3d_amd import ops
    exp = host[case["name"]]
    M = len(case["flags"])
    bufs = _guarded(M)
    views = {k: v[1] for k, v in bufs.items()}
    got = ops.box_velocity(*vc.args_of(case), out=views)
    _assert_equal(got, exp)
    _guards_intact(bufs, M)
    # poisoned outputs, same call: the first launch initialises everything, so the bytes are the same
    views["next_match"].fill_(12345); views["prev_match"].fill_(-99); views["vel_src"].fill_(77); views["vel"].fill_(float("nan"))
    again = ops.box_velocity(*vc.args_of(case), out=views)
    torch.cuda.synchronize()
    for k in ("next_match", "prev_match", "vel_src", "vel"):
        assert again[k].tobytes() == got[k].tobytes(), k
    assert again["status"] == got["status"]
    _guards_intact(bufs, M)


def test_bad_frame_next_changes_only_the_status(host):
    """The link of the bad entry is ignored and nothing else differs from the same batch with -1 in its place."""
    from cm3d_amd import ops
    case = vc.by_name("frame_next_out_of_range_7")
    fixed = dict(case, frame_next=np.where(case["frame_next"] == 7, -1, case["frame_next"]).astype(np.int32))
    bad, good = ops.box_velocity(*vc.args_of(case)), ops.box_velocity(*vc.args_of(fixed))
    assert bad["status"] == 1 and good["status"] == 0
    for k in ("next_match", "prev_match", "vel_src", "vel"):
        assert bad[k].tobytes() == good[k].tobytes(), k
    assert (bad["next_match"] >= 0).sum() == 2                     # the other scene's link is there


def test_argument_errors_return_before_any_launch():
    """Negative counts, a wrong link count, a bad max_dt: CM3D_ERR_ARG; a workspace one byte short: CM3D_ERR_WORKSPACE.  The outputs
    keep their poison: nothing was launched."""
    import torch
    from cm3d_amd import _lib
    L = _lib.lib()
    case = vc.by_name("last_frame")
    M, F = len(case["flags"]), len(case["mask_off"]) - 1
    pair_off = V.link_table(case["mask_off"], case["frame_next"], case["frame_time"], case["max_dt"], M)[2]
    total = int(pair_off[-1])
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda()
    d = {k: t(case[k]) for k in ("box", "flags", "mask_off", "class_id", "track_group", "max_speed", "frame_next", "frame_time")}
    d_pair = t(pair_off)
    bufs = _guarded(M)
    for _, view in bufs.values():
        view.fill_(42)
    status = torch.zeros(1, dtype=torch.int32, device="cuda")
    ws_bytes = int(L.cm3d_box_velocity_workspace_bytes(total, M))
    assert ws_bytes >= 4 * (total + M)
    ws = torch.empty(ws_bytes, dtype=torch.uint8, device="cuda")
    st = torch.cuda.current_stream().cuda_stream

    def call(n_frames=F, n_masks=M, n_links=F, total_pairs=total, max_dt=case["max_dt"], bytes_=ws_bytes, n_classes=4, n_groups=3):
        return L.cm3d_box_velocity(d["box"].data_ptr(), d["flags"].data_ptr(), d["mask_off"].data_ptr(), n_frames, n_masks,
                                   d["class_id"].data_ptr(), d["track_group"].data_ptr(), d["max_speed"].data_ptr(), n_classes, n_groups,
                                   d["frame_next"].data_ptr(), d["frame_time"].data_ptr(), float(max_dt), d_pair.data_ptr(), n_links,
                                   total_pairs, bufs["next_match"][1].data_ptr(), bufs["prev_match"][1].data_ptr(),
                                   bufs["vel"][1].data_ptr(), bufs["vel_src"][1].data_ptr(), status.data_ptr(), ws.data_ptr(), bytes_, st)
    ERR_ARG, ERR_WS = -1, -3
    assert call(n_frames=-1) == ERR_ARG and call(n_frames=0) == ERR_ARG and call(n_masks=-1) == ERR_ARG
    assert call(total_pairs=-1) == ERR_ARG and call(n_links=F - 1) == ERR_ARG
    assert call(max_dt=0.0) == ERR_ARG and call(max_dt=float("nan")) == ERR_ARG
    assert call(n_classes=0) == ERR_ARG and call(n_groups=-2) == ERR_ARG
    assert call(bytes_=ws_bytes - 1) == ERR_WS
    torch.cuda.synchronize()
    for name, (whole, view) in bufs.items():
        assert (view.cpu().numpy() == 42).all(), name
    assert int(status.item()) == 0
    assert call() == 0                                   # and the same arguments, whole, run
    torch.cuda.synchronize()
    assert bufs["next_match"][1].cpu().numpy().tolist() == case["expect"]["next_match"]
