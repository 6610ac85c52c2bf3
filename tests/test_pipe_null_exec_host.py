"""CPU: the executors of a LiftPipeline with the null stream among them (cm3d_amd/csrc/pipe_sched.h pipe_exec_plan; csrc/pipeline.cpp
cm3d_pipe_create2, cm3d_pipe_null_exec), checked by a stand-alone program (tests/pipe_null_exec_sim.cpp: pipeline.cpp over stubs of the
stage entry points and the runtime, built with the address and undefined-behaviour sanitizers, runtimes linked statically)."""
import functools
import os
import shutil
import subprocess
import tempfile

import pytest

from tests.test_pipe_sched_host import SANITIZED

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NULL, ERR_LAUNCH = 0, -2


@functools.lru_cache(maxsize=None)
def _sim():
    """The program's output (built and run once): its own checks passed, and the lines it prints for the tests below."""
    rocm = os.environ.get("ROCM_PATH", "/opt/rocm")
    if shutil.which("g++") is None or not os.path.exists(os.path.join(rocm, "include", "hip", "hip_runtime_api.h")):
        pytest.skip("no g++ or no HIP headers")
    with tempfile.TemporaryDirectory() as tmp:
        exe = os.path.join(tmp, "pipe_null_exec_sim")
        r = subprocess.run(SANITIZED + ["-D__HIP_PLATFORM_AMD__", "-isystem", os.path.join(rocm, "include"),
                                        os.path.join(ROOT, "tests", "pipe_null_exec_sim.cpp"),
                                        os.path.join(ROOT, "cm3d_amd", "csrc", "pipeline.cpp"), "-o", exe], capture_output=True, text=True)
        assert r.returncode == 0, r.stderr
        env = {k: v for k, v in os.environ.items() if k not in ("GPU_MAX_HW_QUEUES", "CM3D_PIPE_NULL_EXEC")}
        r = subprocess.run([exe], capture_output=True, text=True, env=env)
    assert r.returncode == 0 and r.stdout.endswith("pipe_null_exec_sim ok\n"), r.stdout[-2000:] + r.stderr[-4000:]
    return r.stdout.splitlines()


def _lines(kind):
    return [line.split()[1:] for line in _sim() if line.startswith(kind + " ")]


def test_plan_values():
    """The program holds pipe_exec_plan over depth 1-8 x queues -2...64 to: never more than min(depth, 4) executors, a null executor exactly
    where the old policy stopped at the queues, one more executor there and the old count everywhere else.  The listed values:"""
    plans = {(int(d), int(q)): (int(n), bool(int(null))) for d, q, n, null in _lines("plan")}
    assert plans[4, 4] == (4, True) and plans[3, 4] == (3, False) and plans[4, 8] == (4, False) and plans[4, 2] == (2, True)
    assert plans[1, 1] == plans[1, 4] == plans[1, 64] == (1, False)
    assert plans[2, 4] == (2, False) and plans[8, 4] == (4, True) and plans[4, 1] == (2, True) and plans[4, 5] == (4, False)


def test_create2_and_pin():
    """cm3d_pipe_create never makes a null executor, an explicit exec_streams makes none, CM3D_PIPE_NULL_EXEC=0 makes none, null_exec = 1
    makes the last of at least two executors the null stream; cm3d_pipe_pin ends it behind an event wait (the program's own checks)."""
    out = _sim()
    assert "create ok" in out and "pin ok" in out


@pytest.mark.parametrize("depth,queues,n_exec,null_exec", [(4, 4, 4, 3), (4, 2, 2, 1), (3, 4, 3, -1), (3, -2, 2, 1)],
                         ids=["4_slots_4_queues", "4_slots_2_queues", "3_slots_4_queues", "3_slots_on_stream0_and_null"])
def test_pass_trace(depth, queues, n_exec, null_exec):
    """13 round-robin passes: the executor of each (the program has checked that every call of the pass and the record of the slot's event
    received that executor's handle, and that a pass whose slot last ran elsewhere first waits for the slot's event there)."""
    rows = [[int(x, 0) for x in r] for r in _lines("pass") if int(r[0]) == depth and int(r[1]) == queues]
    assert [r[2] for r in rows] == list(range(13))
    last = {}
    for _, _, k, slot, e, handle, waited in rows:
        assert slot == k % depth and e == (slot if n_exec >= depth else k % n_exec)
        assert (handle == NULL) == (e == null_exec)                       # handle 0: the null executor's and nobody else's
        assert handle == NULL or handle == 0x1000 + 0x10 * e             # executor i is streams[i]
        assert bool(waited) == (slot in last and last[slot] != e)
        last[slot] = e
    if null_exec >= 0:
        assert sum(r[5] == NULL for r in rows) == len([k for k in range(13) if (k % depth if n_exec >= depth else k % n_exec) == null_exec])
    else:
        assert all(r[5] != NULL for r in rows)
    if (depth, queues) == (3, -2):
        assert any(r[6] for r in rows)                                    # this is the trace in which slots change executor


def test_an_error_at_each_call_position():
    """A pass of the null executor behind a wait: the wait, each of the pass's six calls and the record of the slot's event answer an error in
    turn.  CM3D_ERR_LAUNCH every time, the pass ends at that call, and the slot's event is recorded behind whatever the pass did enqueue
    (a failed wait enqueues nothing, so nothing is recorded)."""
    fails = [tuple(int(x) for x in r) for r in _lines("fail")]
    n = 1 + 6 + 1
    assert fails == [(0, ERR_LAUNCH, 1, 0)] + [(k, ERR_LAUNCH, k + 2, 1) for k in range(1, n - 1)] + [(n - 1, ERR_LAUNCH, n, 1)]


def test_new_symbols_inside_abi_5():
    from cm3d_amd import _lib
    header = open(os.path.join(ROOT, "include", "cm3d_hip.h")).read()
    assert _lib.ABI_VERSION == 5 and "#define CM3D_ABI_VERSION 5\n" in header
    assert "cm3d_pipe_create2(" in header and "cm3d_pipe_null_exec(" in header
    L = _lib.lib()
    assert L.cm3d_pipe_create2(2, 0, None, -1) is None and L.cm3d_pipe_null_exec(None) == -1
    assert [L.cm3d_pipe_exec_streams_for(d, q) for d, q in ((4, 4), (3, 4), (4, 8), (4, 2))] == [3, 3, 4, 1]      # the old policy stays
