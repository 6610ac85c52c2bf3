"""CPU: the policy that hands a LiftPipeline's passes to streams (cm3d_amd/csrc/pipe_sched.h), simulated by a stand-alone program
(tests/pipe_sched_sim.cpp) built with the address and undefined-behaviour sanitizers; what cm3d_lift_pass enqueues for every kind of
pass, traced over stubs by another (tests/lift_pass_sim.cpp); and the C-ABI around them."""
import ctypes
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_pipe_sched_simulation_under_sanitizers(tmp_path):
    """depth 1..8 x executing streams 1..8 x queue counts 1..32, round robin / always slot 0 / seeded random: (i) consecutive passes of a
    slot share a stream or the later one waits, (ii) round robin loads the streams evenly, (iii) enough streams: stream == slot and
    never a wait, (iv) the policy's values."""
    if shutil.which("g++") is None:
        pytest.skip("no g++")
    exe = tmp_path / "pipe_sched_sim"
    r = subprocess.run(SANITIZED + ["-I", os.path.join(ROOT, "cm3d_amd", "csrc"), os.path.join(ROOT, "tests", "pipe_sched_sim.cpp"), "-o", str(exe)],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    r = subprocess.run([str(exe)], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "pipe_sched ok" in r.stdout


SANITIZED = ["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Wextra", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
             "-static-libasan", "-static-libubsan"]      # the runtimes inside the program: it runs whatever else the loader brings


def _pass_sequence(dense=False, fused=True, separate_reset=False, mask_wh=False, pose=False, obb=False, lane_ready=False, events=False,
                   points=False, planes=1, md_flags=0):
    """The lines tests/lift_pass_sim.cpp prints for a pass: the sequence include/cm3d_hip.h states at cm3d_lift_pass."""
    ev_stage = lambda i: [f"record {0x10 + i:#x}"] if events else []
    ev = "ev=0x20,0x21" if events else "ev=0,0"
    cloud = "points=set" if points else "points=null"
    on_masks = not dense and fused and not separate_reset
    out = [] if on_masks else ["cm3d_batch_begin"]
    out += ev_stage(0)
    if not fused:
        out.append(f"cm3d_sweep_prep max_rows=77 {cloud}")
    if dense:
        out.append("cm3d_erode_pack dense=set")
    else:
        out.append("cm3d_rle_erode_pack" + ("_sized" if mask_wh else "") + ("_begin" if on_masks else "") + (" mask_wh=set" if mask_wh else ""))
    out.append(f"cm3d_sweep_project_hits {cloud} {ev}" if fused else f"cm3d_project_hits {cloud} {ev}")
    from_raw = "null" if points else "set"                   # raw rows only when there is no cloud
    out.append(f"cm3d_compact_hits raw={from_raw} intensity={from_raw} sweep_xf={from_raw} {cloud}")
    out += ev_stage(1)
    out.append(f"cm3d_medoid2 flags={md_flags}")
    out += ev_stage(2)
    if lane_ready:
        out.append("wait 0x30")
    if pose:
        out.append("cm3d_centroid_transform pose_rt=set")
    out.append("cm3d_lane_nn")
    out += ev_stage(3)
    out.append(f"cm3d_box_nms_bounded bound={min(32 * planes, 1024)} pose_inv={'set' if pose else 'null'}")
    out += ev_stage(4)
    if obb:
        out.append("cm3d_obb yaw=set")
    return out


LIFT_PASS_CASES = {
    "plain": {}, "separate_reset": dict(separate_reset=True), "mask_wh": dict(mask_wh=True),
    "mask_wh+separate_reset": dict(mask_wh=True, separate_reset=True), "dense": dict(dense=True),
    "not_fused": dict(fused=False, points=True, planes=2), "not_fused+dense": dict(fused=False, points=True, dense=True),
    "pose": dict(pose=True, planes=32), "obb": dict(obb=True), "lane_ready": dict(lane_ready=True), "events": dict(events=True),
    "md_hint_feedback_0": dict(md_flags=1), "md_hint_feedback_1": dict(md_flags=0),
}


def test_lift_pass_sequence_under_sanitizers(tmp_path):
    """cm3d_lift_pass (csrc/pipeline.cpp) over stubs of the stage entry points and the runtime: for every kind of pass the calls it makes,
    their order and the arguments that select a route are those the header states; a descriptor of another size makes no call; and
    whichever call fails, the pass ends there with that call's error."""
    rocm = os.environ.get("ROCM_PATH", "/opt/rocm")
    if shutil.which("g++") is None or not os.path.exists(os.path.join(rocm, "include", "hip", "hip_runtime_api.h")):
        pytest.skip("no g++ or no HIP headers")
    exe = tmp_path / "lift_pass_sim"
    r = subprocess.run(SANITIZED + ["-D__HIP_PLATFORM_AMD__", "-isystem", os.path.join(rocm, "include"),
                                    os.path.join(ROOT, "tests", "lift_pass_sim.cpp"), os.path.join(ROOT, "cm3d_amd", "csrc", "pipeline.cpp"),
                                    "-o", str(exe)], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    r = subprocess.run([str(exe)], capture_output=True, text=True)
    assert r.returncode == 0 and r.stdout.endswith("lift_pass_sim done\n"), r.stdout + r.stderr
    got = {}
    for line in r.stdout.splitlines()[:-1]:
        if line.startswith("case "):
            calls, rc, fails = got.setdefault(line[5:], ([], [], []))
        elif line.startswith("rc "):
            rc.append(int(line[3:]))
        elif line.startswith("fail "):
            fails.append(tuple(int(x) for x in line.split()[1:]))
        else:
            calls.append(line)
    assert got.pop("wrong_size") == ([], [-1], [])               # CM3D_ERR_ARG and no call
    assert got.pop("not_fused_without_cloud") == ([], [-1], [])  # (the separate launches would hand each other a cloud that is not there)
    assert set(got) == set(LIFT_PASS_CASES)
    for name, kw in LIFT_PASS_CASES.items():
        calls, rc, fails = got[name]
        assert calls == _pass_sequence(**kw), name
        assert rc == [0], name
        # call k answers an error: CM3D_ERR_LAUNCH comes back, and call k was the pass's last
        assert fails == [(k, -2, k + 1) for k in range(len(calls))], name
    assert len(got["events"][0]) == len(got["plain"][0]) + 5 and "record 0x14" in got["events"][0]


def test_abi_version_is_still_5():
    from cm3d_amd import _lib
    assert _lib.ABI_VERSION == 5
    assert "#define CM3D_ABI_VERSION 5\n" in open(os.path.join(ROOT, "include", "cm3d_hip.h")).read()


def test_policy_header_has_no_hip():
    src = open(os.path.join(ROOT, "cm3d_amd", "csrc", "pipe_sched.h")).read()
    assert "#include <hip" not in src and "hipStream" not in src


def test_exec_streams_policy_through_the_library(monkeypatch):
    from cm3d_amd import _lib
    L = _lib.lib()
    assert [L.cm3d_pipe_exec_streams_for(d, q) for d, q in ((4, 4), (4, 8), (8, 16), (1, 32), (3, 4), (4, 2), (4, 1))] == [3, 4, 4, 1, 3, 1, 1]
    for value, want in (("4", 3), ("8", 4), ("2", 1), ("junk", 3)):
        monkeypatch.setenv("GPU_MAX_HW_QUEUES", value)
        assert L.cm3d_pipe_exec_streams_for(4, 0) == want, value
    monkeypatch.delenv("GPU_MAX_HW_QUEUES")
    assert L.cm3d_pipe_exec_streams_for(4, 0) == 3          # unset: the runtime's default of four queues
    assert os.environ.get("GPU_MAX_HW_QUEUES") is None      # read, never set


def test_descriptor_layout_matches_the_header(tmp_path):
    """The ctypes structure and the C struct agree field for field (a C program prints the offsets)."""
    if shutil.which("gcc") is None:
        pytest.skip("no gcc")
    from cm3d_amd import _lib
    names = [n for n, _ in _lib.LiftPassDesc._fields_]
    src = tmp_path / "t.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "cm3d_hip.h"\nint main(void) {\n'
                   + "".join(f'printf("%zu\\n", offsetof(cm3d_lift_pass_desc, {n}));\n' for n in names)
                   + 'printf("%zu\\n", sizeof(cm3d_lift_pass_desc)); return 0; }\n')
    exe = tmp_path / "t"
    r = subprocess.run(["gcc", "-std=c99", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    got = [int(x) for x in subprocess.run([str(exe)], capture_output=True, text=True).stdout.split()]
    assert got == [getattr(_lib.LiftPassDesc, n).offset for n in names] + [ctypes.sizeof(_lib.LiftPassDesc)]


def test_bad_arguments_never_launch():
    from cm3d_amd import _lib
    L = _lib.lib()
    d = _lib.LiftPassDesc()
    assert L.cm3d_lift_pass(None, None) == -1
    assert L.cm3d_lift_pass(ctypes.byref(d), None) == -1          # size field not filled: another layout
    assert L.cm3d_pipe_create(0, 0, None) is None and L.cm3d_pipe_create(2, 0, None) is None
    assert L.cm3d_pipe_submit(None, 0, ctypes.byref(d)) == -1 and L.cm3d_pipe_acquire(None, 0) == -1
    assert L.cm3d_pipe_release(None, 0) == -1 and L.cm3d_pipe_wait(None, 0) == -1 and L.cm3d_pipe_pin(None) == -1
    L.cm3d_pipe_destroy(None)
