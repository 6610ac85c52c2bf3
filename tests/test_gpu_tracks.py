"""GPU: cm3d_box_tracks (ops.box_tracks) against its host statement (cm3d_amd.tracks.box_tracks_host) on every case of
tests/tracks_cases.py with every settings triple of the case -- ids, positions, lengths and flags exact, statistics, smoothed
velocities and box rows to the bit --, between guard words around all seven written arrays and behind the workspace; a second run on
restored inputs and poisoned outputs; the status cases; and the errors that must return before any launch."""
import numpy as np
import pytest

from cm3d_amd import tracks as T
from tests import tracks_cases as tc

pytestmark = pytest.mark.gpu

CASES = tc.all_cases()
IDS = [c["name"] for c in CASES]
GUARD = 64                      # words in front of and behind every written array
I32_GUARD, F64_GUARD = 0x5A5A1234, -7.25e300
WS_GUARD = 4096                 # bytes behind the workspace the call is told of
ARRAYS = (("track_id", 1, "i"), ("track_pos", 1, "i"), ("track_len", 1, "i"), ("flags", 1, "i"), ("track_stat", 4, "d"), ("vel_smooth", 2, "d"),
          ("box", tc.BOX_STRIDE, "d"))
INT_KEYS = ("track_id", "track_pos", "track_len", "flags")
F64_KEYS = ("track_stat", "vel_smooth", "box")


@pytest.fixture(scope="module")
def host():
    return {(c["name"], st): T.box_tracks_host(*tc.args_of(c), *st) for c in CASES for st in c["settings"]}


def _guarded(M):
    """The seven arrays the call writes, of M masks, inside guard words: name -> (whole tensor, the view handed to the call)."""
    import torch
    out = {}
    for name, width, kind in ARRAYS:
        dtype, fill = (torch.int32, I32_GUARD) if kind == "i" else (torch.float64, F64_GUARD)
        whole = torch.full((2 * GUARD + max(M, 1) * width,), fill, dtype=dtype, device="cuda")
        out[name] = (whole, whole[GUARD:GUARD + max(M, 1) * width])
    return out


def _guards_intact(bufs, M):
    for name, width, kind in ARRAYS:
        whole, view = bufs[name]
        w = whole.cpu().numpy()
        fill = I32_GUARD if kind == "i" else F64_GUARD
        n = view.numel()                                 # (M = 0: a view of one element, which is the test's and no guard)
        assert (w[:GUARD] == fill).all() and (w[GUARD + n:] == fill).all(), name


def _poison(bufs):
    for name in ("track_id", "track_pos", "track_len"):
        bufs[name][1].fill_(12345)
    bufs["track_stat"][1].fill_(float("nan")); bufs["vel_smooth"][1].fill_(float("nan"))


def _raw_call(case, st, bufs, ws_extra=WS_GUARD, **override):
    """cm3d_box_tracks through ctypes on the guarded arrays (box and flags filled from the case), the workspace followed by guard
    bytes: (return code, status).  override: arguments of the call to replace."""
    import torch
    from cm3d_amd import _lib
    L = _lib.lib()
    M, F = len(case["flags"]), len(case["frame_time"])
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a if a.size else np.zeros(1, a.dtype))).cuda()
    d = {k: t(case[k]) for k in ("mask_frame", "next_match", "prev_match", "frame_time")}
    if M:
        bufs["box"][1].copy_(t(case["box"]).view(-1)); bufs["flags"][1].copy_(t(case["flags"]))
    status = torch.zeros(1, dtype=torch.int32, device="cuda")
    ws_bytes = int(L.cm3d_box_tracks_workspace_bytes(M))
    ws = torch.full((ws_bytes + ws_extra,), 0xA5, dtype=torch.uint8, device="cuda")
    a = dict(n_masks=M, n_frames=F, min_length=st[0], score_mode=T.score_code(st[1]), smooth_window=st[2],
             vel_smooth=bufs["vel_smooth"][1].data_ptr(), ws=ws.data_ptr(), ws_bytes=ws_bytes)
    a.update(override)
    rc = L.cm3d_box_tracks(bufs["box"][1].data_ptr(), bufs["flags"][1].data_ptr(), d["mask_frame"].data_ptr(), d["next_match"].data_ptr(),
                           d["prev_match"].data_ptr(), d["frame_time"].data_ptr(), a["n_masks"], a["n_frames"], a["min_length"],
                           a["score_mode"], a["smooth_window"], bufs["track_id"][1].data_ptr(), bufs["track_pos"][1].data_ptr(),
                           bufs["track_len"][1].data_ptr(), bufs["track_stat"][1].data_ptr(), a["vel_smooth"], status.data_ptr(), a["ws"],
                           a["ws_bytes"], torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    assert (ws[ws_bytes:].cpu().numpy() == 0xA5).all(), "bytes behind the workspace"
    return rc, int(status.item())


def _read(bufs, M):
    out = {}
    for name, width, kind in ARRAYS:
        a = bufs[name][1].cpu().numpy()[:M * width]
        out[name] = a.reshape(M, width) if width > 1 else a
    return out


def _assert_equal(got, exp, what):
    for k in INT_KEYS:
        assert np.array_equal(got[k], exp[k]), (what, k)
    for k in F64_KEYS:
        assert got[k].tobytes() == exp[k].tobytes(), (what, k)


@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_device_equals_the_host_statement(case, host):
    M = len(case["flags"])
    bufs = _guarded(M)
    for st in case["settings"]:
        exp = host[case["name"], st]
        _poison(bufs)
        rc, status = _raw_call(case, st, bufs)
        assert rc == 0 and status == exp["status"] == case["status"]
        got = _read(bufs, M)
        _assert_equal(got, exp, st)                      # (W = 0 with a vel_smooth given: zeros)
        _guards_intact(bufs, M)
        tc.check_pinned(case, st, got)
        # inputs restored (by _raw_call), outputs poisoned, the same call: the same bytes
        _poison(bufs)
        rc, status2 = _raw_call(case, st, bufs)
        again = _read(bufs, M)
        assert rc == 0 and status2 == status
        for k in INT_KEYS + F64_KEYS:
            assert again[k].tobytes() == got[k].tobytes(), (st, k)
        _guards_intact(bufs, M)


@pytest.mark.parametrize("case", [c for c in CASES if c["settings"] and len(c["flags"])][:6], ids=lambda c: c["name"])
def test_ops_wrapper_returns_the_statement(case, host):
    from cm3d_amd import ops
    st = case["settings"][1]
    got, exp = ops.box_tracks(*tc.args_of(case), *st), host[case["name"], st]
    for k in INT_KEYS:
        assert np.array_equal(got[k], exp[k]), k
    for k in ("track_stat", "box") + (("vel_smooth",) if st[2] else ()):
        assert got[k].tobytes() == exp[k].tobytes(), k
    assert got["status"] == exp["status"] and ("vel_smooth" in got) == (st[2] > 0)


@pytest.mark.parametrize("case", [c for c in CASES if c["fixed"] is not None], ids=lambda c: c["name"])
def test_a_status_case_changes_only_what_the_rule_says(case):
    """The device on the offending arrays against the device on the arrays as the rule reads them: the status differs, the five pure
    outputs do not, and box / flags differ only where the case itself does."""
    from cm3d_amd import ops
    for st in case["settings"]:
        bad, good = ops.box_tracks(*tc.args_of(case), *st), ops.box_tracks(*tc.args_of(case["fixed"]), *st)
        assert bad["status"] == case["status"] and good["status"] == 0
        for k in ("track_id", "track_pos", "track_len", "track_stat") + (("vel_smooth",) if st[2] else ()):
            assert bad[k].tobytes() == good[k].tobytes(), (st, k)
        same = case["flags"] == case["fixed"]["flags"]
        assert np.array_equal(bad["flags"][same], good["flags"][same]) and np.array_equal(bad["box"][same], good["box"][same])
        assert np.array_equal(bad["flags"][~same], case["flags"][~same]) and np.array_equal(bad["box"][~same], case["box"][~same])


def test_argument_and_workspace_errors_leave_the_poison():
    """Negative counts, no frame, min_length 0, a score mode outside 0..2, a negative window, a window without vel_smooth:
    CM3D_ERR_ARG; a workspace one byte short or NULL: CM3D_ERR_WORKSPACE.  Every written array keeps its poison: nothing was launched."""
    import torch
    case = tc.by_name("lengths_1_2_3_F")
    M, st = len(case["flags"]), (2, "mean", 1)
    bufs = _guarded(M)
    ERR_ARG, ERR_WS = -1, -3
    ws_bytes = M * 16

    def call(**kw):
        rc, status = _raw_call(case, st, bufs, **kw)
        assert status == 0
        return rc
    for name in ("track_id", "track_pos", "track_len", "track_stat", "vel_smooth"):
        bufs[name][1].fill_(42)
    for kw in (dict(n_masks=-1), dict(n_frames=0), dict(n_frames=-3), dict(min_length=0), dict(min_length=-1), dict(score_mode=3),
               dict(score_mode=-1), dict(smooth_window=-1), dict(vel_smooth=None)):
        assert call(**kw) == ERR_ARG, kw
    assert call(ws_bytes=ws_bytes - 1) == ERR_WS and call(ws=None) == ERR_WS
    torch.cuda.synchronize()
    for name in ("track_id", "track_pos", "track_len", "track_stat", "vel_smooth"):
        assert (bufs[name][1].cpu().numpy() == 42).all(), name
    got = _read(bufs, M)
    assert np.array_equal(got["flags"], case["flags"]) and got["box"].tobytes() == case["box"].tobytes()
    _guards_intact(bufs, M)
    assert call() == 0                                   # and the same arguments, whole, run
    assert _read(bufs, M)["track_len"].tolist() == case["expect"][st]["track_len"]
    assert call(smooth_window=0, vel_smooth=None) == 0   # W = 0 needs no vel_smooth
