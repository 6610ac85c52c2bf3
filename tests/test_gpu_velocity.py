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


def test_over_capacity_sets_the_status_and_leaves_the_third_scene_alone(host):
    """(the parametrised test above holds the case to the host statement with guard words; this one says what the case is)"""
    from cm3d_amd import ops
    case = vc.by_name("over_capacity")
    got = ops.box_velocity(*vc.args_of(case))
    m4 = int(case["mask_off"][4])
    assert got["status"] == 2 and (got["next_match"][:m4] == -1).all() and (got["prev_match"][:m4] == -1).all()
    assert (got["next_match"][m4:] >= 0).sum() == 3 and not got["vel_src"][:m4].any()


WS_GUARD = 4096                 # bytes behind the workspace the call is told of


def _raw_call(case, pair_off, total_pairs):
    """cm3d_box_velocity through ctypes with a pair_off and a total_pairs of the caller's choosing, the workspace sized by that total:
    (outputs as numpy, status).  Asserts the guard words around the four outputs and the guard bytes behind the workspace."""
    import torch
    from cm3d_amd import _lib
    L = _lib.lib()
    M, F = len(case["flags"]), len(case["mask_off"]) - 1
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda()
    d = {k: t(case[k]) for k in ("box", "flags", "mask_off", "class_id", "track_group", "max_speed", "frame_next", "frame_time")}
    d_pair = t(np.asarray(pair_off, np.int64))
    bufs = _guarded(M)
    for _, view in bufs.values():
        view.fill_(42)
    status = torch.zeros(1, dtype=torch.int32, device="cuda")
    ws_bytes = int(L.cm3d_box_velocity_workspace_bytes(int(total_pairs), M))
    ws = torch.full((ws_bytes + WS_GUARD,), 0xA5, dtype=torch.uint8, device="cuda")
    rc = L.cm3d_box_velocity(d["box"].data_ptr(), d["flags"].data_ptr(), d["mask_off"].data_ptr(), F, M, d["class_id"].data_ptr(),
                             d["track_group"].data_ptr(), d["max_speed"].data_ptr(), case["track_group"].size, case["max_speed"].size,
                             d["frame_next"].data_ptr(), d["frame_time"].data_ptr(), float(case["max_dt"]), d_pair.data_ptr(), F,
                             int(total_pairs), bufs["next_match"][1].data_ptr(), bufs["prev_match"][1].data_ptr(), bufs["vel"][1].data_ptr(),
                             bufs["vel_src"][1].data_ptr(), status.data_ptr(), ws.data_ptr(), ws_bytes, torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    assert rc == 0
    _guards_intact(bufs, M)
    assert (ws[ws_bytes:].cpu().numpy() == 0xA5).all()
    out = {k: v[1].cpu().numpy() for k, v in bufs.items()}
    out["vel"] = out["vel"].reshape(-1, 2)
    return out, int(status.item())


@pytest.mark.parametrize("variant", ["slot_claims_too_many", "total_ends_inside_the_last_slot"])
def test_a_slot_that_disagrees_loses_its_link_and_nothing_else(variant):
    """pair_off comes from the caller.  A slot that does not hold exactly M_f * M_n pairs inside [0, total_pairs] sets status bit 1 and
    holds no match; every other output byte is the host statement of the batch without that link.  pair_off stays monotone: the header
    promises nothing for overlapping slots."""
    case = vc.by_name("three_link_chain")
    pair_off = V.link_table(case["mask_off"], case["frame_next"], case["frame_time"], case["max_dt"])[2]
    assert pair_off.tolist() == [0, 30, 54, 82, 82]
    if variant == "slot_claims_too_many":          # slot 1 claims 7 pairs too many; the slots behind it are shifted but consistent
        bad, total = 1, int(pair_off[-1]) + 7
        pair_off = pair_off + np.array([0, 0, 7, 7, 7])
    else:                                          # the total ends inside the last link's slot
        bad, total = 2, int(pair_off[2]) + 10
    assert (np.diff(pair_off) >= 0).all()
    got, status = _raw_call(case, pair_off, total)
    nxt = case["frame_next"].copy()
    nxt[bad] = -1
    exp = V.track_velocity_host(*vc.args_of(dict(case, frame_next=nxt)))
    whole = V.track_velocity_host(*vc.args_of(case))
    assert status & 2 and exp["status"] == 0
    f0, f1 = int(case["mask_off"][bad]), int(case["mask_off"][bad + 1])
    assert (whole["next_match"][f0:f1] >= 0).any() and (got["next_match"][f0:f1] == -1).all()
    for k in ("next_match", "prev_match", "vel_src", "vel"):
        assert got[k].tobytes() == exp[k].tobytes(), k
    assert (got["next_match"] >= 0).sum() == (exp["next_match"] >= 0).sum() >= 7         # the other two links are there


@pytest.mark.parametrize("pair", vc.clamp_cases(), ids=[c["name"] for c, _ in vc.clamp_cases()])
def test_mask_off_is_read_clamped(pair):
    """A last mask_off entry far beyond the masks, a negative first one: every frame's range is clamped into [0, M] before it indexes
    anything, so the outputs are the host statement on the clamped offsets and the guard words stand."""
    from cm3d_amd import ops
    raw, clamped = pair
    M = len(raw["flags"])
    exp = V.track_velocity_host(*vc.args_of(clamped))
    bufs = _guarded(M)
    got = ops.box_velocity(*vc.args_of(raw), out={k: v[1] for k, v in bufs.items()})
    _assert_equal(got, exp)
    _guards_intact(bufs, M)
    assert got["status"] == 0 and (got["next_match"] >= 0).sum() == 4


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
