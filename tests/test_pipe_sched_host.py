"""CPU: the policy that hands a LiftPipeline's passes to streams (cm3d_amd/csrc/pipe_sched.h), simulated by a stand-alone program
(tests/pipe_sched_sim.cpp) built with the address and undefined-behaviour sanitizers; and the C-ABI around it."""
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
    r = subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Wextra", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                        "-static-libasan", "-static-libubsan",      # the runtimes inside the program: it runs whatever else the loader brings
                        "-I", os.path.join(ROOT, "cm3d_amd", "csrc"), os.path.join(ROOT, "tests", "pipe_sched_sim.cpp"), "-o", str(exe)],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    r = subprocess.run([str(exe)], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "pipe_sched ok" in r.stdout


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
