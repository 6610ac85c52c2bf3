"""GPU: cm3d_box_place against its host statement (cm3d_amd.boxplace.box_place_host) on the case tables of tests/box_place_cases.py, in
the nuScenes and the Waymo form: the placed centres, place_src, place_pushed, flags and column 9 to the bit -- the rule has no library
call, so there is no tolerance --, everything else byte-identical to the input, every output between guard words; with a launch bound of
64 (registers and ballots) and of 1024 (LDS for the frames of more than 64 masks); and the bad-argument calls, which launch nothing."""
import itertools

import numpy as np
import pytest

from cm3d_amd import boxplace
from tests import box_place_cases as pc

pytestmark = pytest.mark.gpu

GUARD = 0x5A5A5A5A
G = 16


def _place(t, thin, bound):
    """cm3d_box_place on a table, every array it writes between guard words.  Returns the dict of box_place_host."""
    import torch
    from cm3d_amd import _lib
    L = _lib.lib()
    M = t["flags"].size
    F = t["mask_off"].size - 1
    dev = lambda a: torch.from_numpy(np.array(a)).cuda()                  # (a copy: the tables are read-only)

    def guarded(a, fill):
        a = np.ascontiguousarray(a).reshape(-1)
        return dev(np.concatenate([np.full(G, fill, a.dtype), a, np.full(G, fill, a.dtype)]))
    box, flags = guarded(t["box"], -7.25), guarded(t["flags"], GUARD)
    src, pushed = guarded(np.full(M, GUARD, np.int32), GUARD), guarded(np.full(2 * M, -7.25), -7.25)
    off, rect, ysrc = dev(t["mask_off"]), dev(t["fit_rect"]), dev(t["yaw_src"])
    prior, grp, thr = dev(t["prior_wlh"]), dev(t["nms_group"]), dev(t["nms_thr"])
    ego = None if t["ego_xyz"] is None else dev(t["ego_xyz"])
    rc = L.cm3d_box_place(box[G:].data_ptr(), flags[G:].data_ptr(), off.data_ptr(), F, M, rect.data_ptr(), ysrc.data_ptr(), prior.data_ptr(),
                          grp.data_ptr(), thr.data_ptr(), len(pc.PRIOR_WLH), None if ego is None else ego.data_ptr(), int(ego is None), thin, bound,
                          src[G:].data_ptr(), pushed[G:].data_ptr(), torch.cuda.current_stream().cuda_stream)
    assert rc == 0
    torch.cuda.synchronize()
    out = {}
    for key, a, n, fill in (("box", box, 10 * M, -7.25), ("flags", flags, M, GUARD), ("place_src", src, M, GUARD), ("place_pushed", pushed, 2 * M, -7.25)):
        a = a.cpu().numpy()
        assert (a[:G] == fill).all() and (a[G + n:] == fill).all(), key
        out[key] = a[G:G + n]
    out["box"], out["place_pushed"] = out["box"].reshape(M, 10), out["place_pushed"].reshape(M, 2)
    return out


def _host(t, thin, bound):
    return boxplace.box_place_host(t["box"], t["flags"], t["mask_off"], t["fit_rect"], t["yaw_src"], t["prior_wlh"], t["nms_group"], t["nms_thr"],
                                   t["ego_xyz"], thin, bound)


def _check(t, got, exp):
    for key in ("box", "flags", "place_src", "place_pushed"):
        assert got[key].dtype == exp[key].dtype and got[key].shape == exp[key].shape, key
    bad = [m for m in range(len(exp["flags"])) if got["box"][m].tobytes() != exp["box"][m].tobytes() or got["flags"][m] != exp["flags"][m]
           or got["place_src"][m] != exp["place_src"][m] or got["place_pushed"][m].tobytes() != exp["place_pushed"][m].tobytes()]
    assert not bad, [(m, t["names"][m]) for m in bad[:8]]
    # what the launch may not touch, against the input itself
    assert got["box"][:, 2:9].tobytes() == t["box"][:, 2:9].tobytes()
    off = got["place_src"] == 0
    assert got["box"][off, :9].tobytes() == t["box"][off, :9].tobytes() and got["place_pushed"].tobytes() == t["box"][:, :2].tobytes()
    assert np.array_equal(got["box"][:, 9], got["flags"].astype(np.float64)) and np.array_equal(got["flags"] & 1, t["flags"] & 1)


@pytest.mark.parametrize("waymo", [False, True], ids=["nusc", "waymo"])
@pytest.mark.parametrize("table", ["rule", "nms"])
def test_place_equals_host_statement_to_the_bit(table, waymo):
    t = pc.rule_table(waymo) if table == "rule" else pc.nms_table(waymo)
    seen = np.zeros(4, int)
    for thin, bound in itertools.product(pc.THINS, pc.BOUNDS):
        exp = _host(t, thin, bound)
        _check(t, _place(t, thin, bound), exp)
        seen += np.bincount(exp["place_src"], minlength=4)
    assert seen.min() > 0 and (t["ego_xyz"] is None) == waymo
    if table == "nms":
        exp = _host(t, pc.THIN, 1024)
        assert all(exp["flags"][j] == (1 if goes else 3) for _, j, goes in t["pairs"])
        assert not np.array_equal(exp["flags"], _host(t, pc.THIN, 64)["flags"])         # the bound matters on the frames of 65 and 130


def test_a_second_call_places_nothing_twice():
    """The launch is IN/OUT on box and flags: a second call on its own output finds the placed centres where the rule puts them again
    (the rule reads fit_rect, not the centre), keeps the verdict, and reports the first call's centres as the pushed ones."""
    t = pc.nms_table(False)
    first = _place(t, pc.THIN, 1024)
    again = _place(dict(t, box=first["box"], flags=first["flags"]), pc.THIN, 1024)
    assert again["box"].tobytes() == first["box"].tobytes() and np.array_equal(again["flags"], first["flags"])
    assert again["place_pushed"].tobytes() == first["box"][:, :2].tobytes() and np.array_equal(again["place_src"], first["place_src"])


def test_mask_off_outside_the_batch_is_clamped():
    """Offsets that leave [0, n_masks] address nothing outside the arrays: the guard words stand, and the frames are what the clamped
    offsets describe."""
    t = pc.rule_table(False)
    wild = t["mask_off"].copy()
    wild[0], wild[-1] = -9, 2 ** 30
    exp = _host(dict(t, mask_off=wild), pc.THIN, 1024)
    same = _host(t, pc.THIN, 1024)
    assert exp["box"].tobytes() == same["box"].tobytes()
    _check(t, _place(dict(t, mask_off=wild), pc.THIN, 1024), exp)


def test_bad_arguments_launch_nothing():
    import torch
    from cm3d_amd import _lib
    L = _lib.lib()
    t = pc.rule_table(False)
    M, F = t["flags"].size, t["mask_off"].size - 1
    dev = lambda a: torch.from_numpy(np.array(a)).cuda()                  # (a copy: the tables are read-only)
    arr = {k: dev(t[k]) for k in ("box", "flags", "mask_off", "fit_rect", "yaw_src", "prior_wlh", "nms_group", "nms_thr", "ego_xyz")}
    src, pushed = torch.full((M,), GUARD, dtype=torch.int32, device="cuda"), torch.full((M, 2), -7.25, dtype=torch.float64, device="cuda")
    p = lambda k: arr[k].data_ptr()
    st = torch.cuda.current_stream().cuda_stream
    ok = [p("box"), p("flags"), p("mask_off"), F, M, p("fit_rect"), p("yaw_src"), p("prior_wlh"), p("nms_group"), p("nms_thr"), len(pc.PRIOR_WLH),
          p("ego_xyz"), 0, pc.THIN, 1024, src.data_ptr(), pushed.data_ptr(), st]
    calls = [[None if i == k else v for i, v in enumerate(ok)] for k in (0, 1, 2, 5, 6, 7, 8, 9, 11, 15, 16)]
    calls += [[bad if i == k else v for i, v in enumerate(ok)] for k in (3, 4, 10, 14) for bad in (0, -1)]
    calls += [[bad if i == 13 else v for i, v in enumerate(ok)] for bad in (float("nan"), -0.25, float("inf"))]
    for args in calls:
        assert L.cm3d_box_place(*args) == -1
    torch.cuda.synchronize()
    assert arr["box"].cpu().numpy().tobytes() == t["box"].tobytes() and np.array_equal(arr["flags"].cpu().numpy(), t["flags"])
    assert (src.cpu().numpy() == GUARD).all() and (pushed.cpu().numpy() == -7.25).all()
    # Waymo: ego_xyz may be NULL, and is not read when it is given
    waymo = [None if i == 11 else 1 if i == 12 else v for i, v in enumerate(ok)]
    assert L.cm3d_box_place(*waymo) == 0
    torch.cuda.synchronize()
    assert (src.cpu().numpy() != GUARD).all()
