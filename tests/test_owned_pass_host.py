"""CPU: the call sequence of the owned pass (cm3d_lift_pass_owned), traced over stubs by the stand-alone program of the stripped pass
(tests/pass_strip_sim.cpp, its owned.* cases; built with the address and undefined-behaviour sanitizers by
tests/test_ground_strip_host.py) and compared with the sequence include/cm3d_hip.h states: head; ownership between its events; strip
between its events; clustering; tail; filter; yaw; placement; NMS.  And the composer behind it (cm3d_lift_pass_composed): for every
presence combination its trace is, line for line, the trace of the entry point that takes the same arguments."""
import itertools

from tests.test_ground_strip_host import CODE as STRIP_CODE, sim

CODE = dict(STRIP_CODE, cm3d_point_owner=-3)

REFUSED = ["null_owner", "owner_size", "owner_no_ow_owner", "owner_no_ow_off", "owner_no_ow_tile_off", "owner_no_ow_idx", "owner_no_ow_xyz",
           "owner_no_ow_status", "owner_no_ow_lost", "owner_no_ws", "rule_2", "min_keep_0", "pass_no_hit_idx", "strip_no_gs_idx", "strip_param",
           "place_without_yaw", "raw_lists_behind_owner", "ow_lists_behind_strip"]


def owned_sequence(s, c, f, y, p, n, waymo=False, cloud=False, ev=True):
    """include/cm3d_hip.h's statement of cm3d_lift_pass_owned for one presence combination."""
    rec = lambda e: [f"record {e:#x}"]
    part = lambda name, lists, work: f"{name} hit_off={lists}_off tile_off={lists}_tile_off hit_idx={lists}_idx hit_xyz={lists}_xyz tile_work={work}"
    out = ["cm3d_lift_pass_head hit_off=hit_off tile_off=tile_off hit_idx=hit_idx hit_xyz=hit_xyz tile_work=tile_work"] + (rec(0x20) if ev else [])
    out += ["cm3d_point_owner in=hit_xyz,hit_idx,hit_off off=mask_off score=score n=3,7,4096,3000 par=1,5 "
            "out=ow_owner,ow_off,ow_tile_off,ow_idx,ow_xyz,ow_status,ow_lost ws=ow_ws,16"] + (rec(0x21) if ev else [])
    lists = "ow"
    if s:
        out += (rec(0x30) if ev else [])
        out += [f"cm3d_ground_grid cloud={'points,pt_off' if cloud else 'null,null'} raw=raw,5 rest=set n=6,5000,3 halfw=1.5 origin=ego par=2,4,3,0.1,8 "
                "out=grid_z,grid_n",
                "cm3d_ground_strip in=ow_xyz,ow_idx,ow_off frame=set n=7,4096,3 origin=ego grid=grid_z par=2,0.3,5 "
                "out=gs_off,gs_tile_off,gs_idx,gs_xyz,gs_status,gs_dropped ws=gs_ws,16"] + (rec(0x31) if ev else [])
        lists = "gs"
    if c:
        out += rec(0x50) + [f"cm3d_depth_cluster in={lists}_xyz,{lists}_idx,{lists}_off origin=origin out=cl_off,cl_tile_off,cl_idx,cl_xyz,cl_status ws=cl_ws"]
        out += rec(0x51)
        lists = "cl"
    out += [part("cm3d_lift_pass_tail", lists, "null")]
    pos = "kept" if f else "medoid_pos"
    if f:
        out += rec(0x40) + ["cm3d_stage2_filter pos=medoid_pos out=kept"] + rec(0x41) + ["cm3d_box_nms_bounded pos=kept lane=lane out=box,flags"]
    if y:
        out += rec(0x60) + [f"cm3d_bev_fit in={lists}_xyz,{lists}_off out=fit_rect", f"cm3d_yaw_select pos={pos} out=yaw_tab"] + rec(0x61)
        out += [f"cm3d_box_nms_bounded pos={pos} lane=yaw_tab out=box,flags"]
    if p:
        out += rec(0x70) + [f"cm3d_box_place io=box,flags in=fit_rect,yaw_src waymo={int(waymo)} thin=0.5 out=place_src,place_pushed"] + rec(0x71)
    if n:
        out += [f"cm3d_box_rotated_nms io=box,flags waymo={int(waymo)}"]
    return out


def assert_pass(trace, want, name):
    calls, rc, fails = trace
    assert calls == want, (name, calls, want)
    assert rc == [0], name
    assert fails == [(k, CODE[c.split()[0]], k + 1) for k, c in enumerate(calls)], name       # ends at the first error, with its code


def test_owned_pass_sequence():
    got = sim()
    seen = 0
    for on in itertools.product((False, True), repeat=6):
        s, c, f, y, p, n = on
        if p and not y:
            continue
        name = "owned.combo." + "".join(ch if o else "-" for ch, o in zip("scfypn", on))
        assert_pass(got[name], owned_sequence(*on), name)
        seen += 1
    assert seen == 48
    assert_pass(got["owned.combo_waymo.scfypn"], owned_sequence(True, True, True, True, True, True, waymo=True), "waymo")
    assert_pass(got["owned.ok.null_opt"], owned_sequence(False, False, False, False, False, False), "null opt")
    assert_pass(got["owned.ok.cloud"], owned_sequence(True, False, False, False, False, False, cloud=True), "cloud")
    assert_pass(got["owned.ok.no_events"], owned_sequence(True, True, False, False, False, False, ev=False), "no events of the ownership's or the strip's")
    assert_pass(got["owned.rule.ow_lists"], owned_sequence(False, False, False, True, False, False), "the fit's own statement of the exclusive lists")
    assert_pass(got["owned.rule.gs_lists"], owned_sequence(True, False, False, True, False, False), "the fit's own statement of the stripped lists")


def test_owned_pass_makes_no_call_on_a_bad_descriptor():
    got = sim()
    bad = {k: v for k, v in got.items() if k.startswith("owned.bad.")}
    assert set(bad) == {"owned.bad." + n for n in REFUSED}
    for name, trace in bad.items():
        assert trace == ([], [-1], []), name                             # CM3D_ERR_ARG and no call at all
    owned = [k for k in got if k.startswith("owned.")]
    assert len(owned) == 48 + 6 + len(REFUSED)
    assert not any("descriptor was changed" in line for k in owned for line in got[k][0])


def test_composed_pass_is_the_entry_point_with_the_same_arguments_line_for_line():
    """cm3d_lift_pass_composed beside cm3d_lift_pass_owned (with an ownership), else _stripped (with a strip), else _placed (with a
    placement), else cm3d_lift_pass_opt: the same calls with the same arguments, the same result, and with every call failing in turn the
    same code after the same number of calls."""
    got = sim()
    seen = 0
    for on in itertools.product((False, True), repeat=8):
        o, w, s, c, f, y, p, n = on
        if (p and not y) or (not o and (c or f or y or p or n)):
            continue
        which = "".join(ch if x else "-" for ch, x in zip("owscfypn", on))
        old, new = got["equiv.old." + which], got["equiv.new." + which]
        assert new == old, which
        calls, rc, fails = new
        assert rc == [0] and calls and len(fails) == len(calls) and all(r < 0 and k == i + 1 for i, r, k in fails), which
        assert ("cm3d_point_owner " in " ".join(calls)) == w and any(line.startswith("cm3d_ground_strip ") for line in calls) == s, which
        assert any(line.startswith("cm3d_box_place ") for line in calls) == p, which
        seen += 1
    assert seen == 96 + 4
    assert len([k for k in got if k.startswith("equiv.")]) == 2 * seen
    assert not any("descriptor was changed" in line for k in got if k.startswith("equiv.") for line in got[k][0])
