"""The stand-alone trace of csrc/pass_options.cpp (tests/pass_options_sim.cpp) for the host tests: built once per session with the
address and undefined-behaviour sanitizers linked in, run once, and parsed; and the sequences include/cm3d_hip.h states, one function
per stage, from which the tests compose what a pass must have called."""
import functools
import os
import shutil
import subprocess
import tempfile

import pytest

from tests.test_pipe_sched_host import SANITIZED

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# the stubs' own error codes: a pass hands the failing call's on
CODE = {"cm3d_lift_pass": -2, "cm3d_lift_pass_head": -2, "cm3d_lift_pass_tail": -2, "record": -2, "cm3d_depth_cluster": -3,
        "cm3d_stage2_filter": -2, "cm3d_bev_fit": -1, "cm3d_yaw_select": -3, "cm3d_box_nms_bounded": -2, "cm3d_box_rotated_nms": -3}


@functools.lru_cache(maxsize=None)
def _run():
    tmp = tempfile.mkdtemp(prefix="pass_options_sim")
    try:
        exe = os.path.join(tmp, "pass_options_sim")
        rocm = os.environ.get("ROCM_PATH", "/opt/rocm")
        r = subprocess.run(SANITIZED + ["-D__HIP_PLATFORM_AMD__", "-isystem", os.path.join(rocm, "include"),
                                        os.path.join(ROOT, "tests", "pass_options_sim.cpp"),
                                        os.path.join(ROOT, "cm3d_amd", "csrc", "pass_options.cpp"), "-o", exe], capture_output=True, text=True)
        assert r.returncode == 0, r.stderr
        r = subprocess.run([exe], capture_output=True, text=True)
        assert r.returncode == 0 and r.stdout.endswith("pass_options_sim done\n"), r.stdout + r.stderr
    finally:
        shutil.rmtree(tmp, ignore_errors=True)
    got = {}
    for line in r.stdout.splitlines()[:-1]:
        if line.startswith("case "):
            assert line[5:] not in got, line
            calls, rc, fails = got[line[5:]] = ([], [], [])
        elif line.startswith("rc "):
            rc.append(int(line[3:]))
        elif line.startswith("fail "):
            fails.append(tuple(int(x) for x in line.split()[1:]))
        else:
            calls.append(line)            # a stub's line -- or the program's complaint that a descriptor was written to
    return got


def traces():
    """case name -> (the clean pass's lines, [rc], [(k, rc, calls made) for a failing call k])."""
    rocm = os.environ.get("ROCM_PATH", "/opt/rocm")
    if shutil.which("g++") is None or not os.path.exists(os.path.join(rocm, "include", "hip", "hip_runtime_api.h")):
        pytest.skip("no g++ or no HIP headers")
    return _run()


def group(prefix):
    """The cases of one group, without the prefix."""
    return {name[len(prefix) + 1:]: t for name, t in traces().items() if name.startswith(prefix + ".")}


def assert_refused(trace, name):
    assert trace == ([], [-1], []), name                     # CM3D_ERR_ARG and no call at all


def assert_pass(trace, want, name):
    """A clean pass made exactly the calls `want`; and whichever of them fails, the pass ends there with that call's code."""
    calls, rc, fails = trace
    assert calls == want, name
    assert rc == [0], name
    assert fails == [(k, CODE[c.split()[0]], k + 1) for k, c in enumerate(calls)], name


RAW = dict(off="hit_off", tile="tile_off", idx="hit_idx", xyz="hit_xyz", work="tile_work")
CL = dict(off="cl_off", tile="cl_tile_off", idx="cl_idx", xyz="cl_xyz", work="null")


def part(name, lists=RAW):
    return "{} size=ok hit_off={off} tile_off={tile} hit_idx={idx} hit_xyz={xyz} tile_work={work} n_masks=7".format(name, **lists)


def records(ev, i):
    return [f"record {ev + i:#x}"] if ev else []


def plain_sequence():
    return [part("cm3d_lift_pass")]


def cluster_sequence(ev=0, eps="1", mp=20, pick=0, idx="hit_idx", cl_idx="cl_idx"):
    """The clustered pass in place of the plain one: head, the clustering from the raw lists into the cl_* arrays, tail on those."""
    return ([part("cm3d_lift_pass_head", dict(RAW, idx=idx))] + records(ev, 0)
            + [f"cm3d_depth_cluster in=hit_xyz,{idx},hit_off frame=set n=7,4096,3 origin=set eps={eps} min={mp} pick={pick} "
               f"out=cl_off,cl_tile_off,{cl_idx},cl_xyz status=set ws=set,16"]
            + records(ev, 1) + [part("cm3d_lift_pass_tail", dict(CL, idx=cl_idx))])


def box_line(pos, lane="lane,lane_off,frame_lane,lane_idx", pose_inv="null", bound=96):
    return f"cm3d_box_nms_bounded pos={pos} lane={lane} dist=lane_dist rest=set n=3,7,10 pose_inv={pose_inv} bound={bound} out=box,flags"


def filter_sequence(ev=0, polygons=False, tables=0, pose_inv="null", bound=96):
    """Behind the pass: the filter on the pass's medoid positions, the boxes again on the kept ones."""
    s = "set" if polygons else "null"
    return (records(ev, 0)
            + [f"cm3d_stage2_filter in=centroid,medoid_pos,lane_dist rest=set n=7,3,10 polygons={s} tables={tables} needs_road={s} thr=20,4 "
               "out=kept,on_road"]
            + records(ev, 1) + [box_line("kept", pose_inv=pose_inv, bound=bound)])


def yaw_sequence(ev=0, lists="hit_xyz,hit_off", pos="medoid_pos", K=128, d0="0.05", mn="20,1", lmd="0", pose="null", pose_inv="null", bound=96):
    """The fit on `lists`, the selection on the pass's lane results and `pos`, the boxes with the yaw table where the lane tables stood."""
    return (records(ev, 0)
            + [f"cm3d_bev_fit in={lists} n=7,4096 cs=set K={K} d0={d0} min={mn} out=set,set,set",
               f"cm3d_yaw_select pos={pos} rest=set classes=10 dist=lane_dist,{lmd} lane=lane,lane_off,frame_lane,lane_idx n=2,900 pose={pose} "
               "n=7,3 out=yaw_tab,yaw_idx,set"]
            + records(ev, 1) + [box_line(pos, "yaw_tab,tab_off,tab_frame,yaw_idx", pose_inv, bound)])


def nms_sequence(waymo=0, bound=96):
    return [f"cm3d_box_rotated_nms io=box,flags off=mask_off rest=set n=3,7,10 thr=rot_thr,10 measure=1 agnostic=1 waymo={waymo} bound={bound}"]


def composed_sequence(cluster, filt, yaw, nms, waymo=False):
    """include/cm3d_hip.h's statement of cm3d_lift_pass_opt for one presence combination, every event set: the per-stage sequences in
    the header's order, the fit on the clustered lists behind a clustering and on the kept positions behind a filter."""
    w = dict(pose_inv="pose_inv", bound=1024) if waymo else {}
    return ((cluster_sequence(ev=0x50) if cluster else plain_sequence())
            + (filter_sequence(ev=0x40, **w) if filt else [])
            + (yaw_sequence(ev=0x60, lists="cl_xyz,cl_off" if cluster else "hit_xyz,hit_off", pos="kept" if filt else "medoid_pos",
                            pose="pose_rt" if waymo else "null", **w) if yaw else [])
            + (nms_sequence(int(waymo), 1024 if waymo else 96) if nms else []))
