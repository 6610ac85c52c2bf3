"""LiftPipeline with the legacy null stream as its last executor (cm3d_pipe_create2, cm3d_pipe_null_exec): whichever
executor a pass lands on, every slot's download is byte for byte that of a lone LiftEngine.run; the executor indices are those of the
plan; and every stream the pipeline and its engines create is non-blocking, so that the null stream never waits for one implicitly."""
import ctypes
import functools

import pytest

from tests.test_gpu_pipe_sched import _batch, _lone, _same, _sentinels

pytestmark = pytest.mark.gpu


@functools.lru_cache(maxsize=None)
def _four():
    """Four different tiny batches of 2, 3, 2 and 3 frames and their lone results (computed once, never written to)."""
    hbs = [_batch(20 + k, 2 + k % 2) for k in range(4)]
    want = [_lone(hb) for hb in hbs]
    assert all(w["hit_idx"].size > 20 for w in want)
    return hbs, want


def _clean(pipe):
    for slot in range(pipe.depth):
        pipe.check_status(slot)                          # raises on any error flag of the slot's passes


def _thirteen(pipe, want_exec, between=None):
    """Four submits and 13 round-robin reruns, sentinels before every slot's last pass; `want_exec(n_pass, slot)`: the executor of pass
    number n_pass."""
    hbs, want = _four()
    depth = pipe.depth
    for k in range(depth):
        assert pipe.submit(hbs[k], "rle") == k
        assert pipe.last_stream(k) == want_exec(k, k)
    n_pass = depth
    for k in range(13):
        if k == 13 - depth:
            _sentinels(pipe)
            before = pipe.native_passes
        if between is not None:
            between()
        pipe.rerun(k % depth)
        assert pipe.last_stream(k % depth) == want_exec(n_pass, k % depth)
        n_pass += 1
    assert pipe.native_passes == before + depth
    for slot in range(depth):
        got_hb, got = pipe.collect(slot)
        assert got_hb is hbs[slot]
        _same(got, want[slot], f"slot {slot} of {depth}, executor {pipe.last_stream(slot)}")
    _clean(pipe)


@pytest.mark.parametrize("default_stream_busy", [False, True], ids=["passes_only", "torch_ops_on_the_default_stream"])
def test_slot_3_runs_on_the_null_stream(default_stream_busy):
    """depth 4 with the null executor: slot 3's passes run on the null stream, every slot gets its lone result -- also with a torch
    operation on the default stream between the reruns, and with new batches submitted behind them (slot 3's upload and first pass on the
    null executor)."""
    import torch
    from cm3d_amd import lifting
    hbs, want = _four()
    pipe = lifting.LiftPipeline("cuda:0", depth=4, null_exec=True)
    assert pipe.exec_streams == 4 and pipe.null_exec == 3 and len(pipe.streams) == 4
    assert int(pipe.lib.cm3d_pipe_null_exec(pipe._h)) == 3
    assert pipe.exec_stream(3) == torch.cuda.default_stream(pipe.dev) and pipe.exec_stream(3).cuda_stream == 0
    assert [pipe.exec_stream(i) for i in range(3)] == pipe.streams[:3]
    acc = torch.zeros(4096, device="cuda:0")

    def bump():
        acc.add_(1.0)                                    # on the default stream: in order with slot 3's passes, beside everyone else's

    _thirteen(pipe, lambda n_pass, slot: slot, between=bump if default_stream_busy else None)
    if default_stream_busy:
        torch.cuda.synchronize()
        assert float(acc.min()) == float(acc.max()) == 13.0
    # every slot collected: the batches once more, shifted by one, so that each slot holds a new one
    for slot in range(4):
        assert pipe.submit(hbs[(slot + 1) % 4], "rle") == slot and pipe.last_stream(slot) == slot
    for slot in range(4):
        _same(pipe.collect(slot)[1], want[(slot + 1) % 4], f"new batch in slot {slot}")
    _clean(pipe)


@pytest.mark.parametrize("kw,n_exec", [(dict(null_exec=False), None), (dict(exec_streams=3), 3), (dict(exec_streams=3, null_exec=False), 3)],
                         ids=["null_exec_False", "exec_streams_3", "both"])
def test_without_the_null_executor_the_mapping_is_todays(kw, n_exec):
    from cm3d_amd import lifting
    pipe = lifting.LiftPipeline("cuda:0", depth=4, **kw)
    if n_exec is None:
        n_exec = int(pipe.lib.cm3d_pipe_exec_streams_for(4, 0))      # the old policy on this process's queues
    assert pipe.exec_streams == n_exec and pipe.null_exec == -1
    assert [pipe.exec_stream(i) for i in range(4)] == pipe.streams
    _thirteen(pipe, lambda n_pass, slot: slot if n_exec >= 4 else n_pass % n_exec)


def test_the_default_follows_the_plan(monkeypatch):
    """Nothing asked: one executor more than the old policy, the null stream, exactly where the old policy stopped at the queues;
    CM3D_PIPE_NULL_EXEC=0 gives the old plan."""
    from cm3d_amd import lifting
    L = lifting.LiftEngine("cuda:0").lib
    for depth in (1, 3, 4):
        old = int(L.cm3d_pipe_exec_streams_for(depth, 0))
        pipe = lifting.LiftPipeline("cuda:0", depth=depth)
        want = (old + 1, old) if old < min(depth, 4) else (old, -1)
        assert (pipe.exec_streams, pipe.null_exec) == want, depth
    monkeypatch.setenv("CM3D_PIPE_NULL_EXEC", "0")
    pipe = lifting.LiftPipeline("cuda:0", depth=4)
    assert (pipe.exec_streams, pipe.null_exec) == (int(L.cm3d_pipe_exec_streams_for(4, 0)), -1)


def test_depth_2_with_timing_events_on_the_null_executor():
    """depth 2, executor 1 the null stream: the results, then one pass with per-stage events (through LiftEngine.run on the default stream)
    and one with a pair around the projection kernel (through cm3d_pipe_submit) on it."""
    import torch
    from cm3d_amd import lifting
    hbs, want = _four()
    pipe = lifting.LiftPipeline("cuda:0", depth=2, null_exec=True)
    assert pipe.exec_streams == 2 and pipe.null_exec == 1
    _thirteen(pipe, lambda n_pass, slot: slot)
    assert pipe.submit(hbs[2], "rle") == 0
    ev = []
    assert pipe.submit(hbs[3], "rle", stage_events=ev) == 1 and pipe.last_stream(1) == 1
    _same(pipe.collect(1)[1], want[3], "stage_events on the null executor")
    assert len(ev) == 5 and all(a.elapsed_time(b) >= 0 for a, b in zip(ev, ev[1:]))
    pe = (torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True))
    _sentinels(pipe)
    n0 = pipe.native_passes
    pipe.rerun(1, project_events=pe)
    pipe.rerun(0)
    assert pipe.native_passes == n0 + 2 and pipe.last_stream(1) == 1
    _same(pipe.collect(1)[1], want[3], "project_events on the null executor")
    _same(pipe.collect(0)[1], want[2], "beside it")
    assert pe[0].elapsed_time(pe[1]) > 0
    _clean(pipe)


def test_graph_capture_ends_the_null_executor():
    """A graph captured on slot 0's stream: from then on slot s runs on streams[s], slot 3 too, behind the pass the null stream ran for it;
    replays interleaved with reruns give the eager results."""
    import torch
    from cm3d_amd import lifting
    hbs, want = _four()
    pipe = lifting.LiftPipeline("cuda:0", depth=4, null_exec=True)
    for hb in hbs:
        pipe.submit(hb, "rle")
    for k in range(6):
        pipe.rerun(k % 4)
    assert pipe.null_exec == 3 and pipe.last_stream(3) == 3
    torch.cuda.synchronize()
    with torch.cuda.stream(pipe.streams[0]):
        g = pipe.engines[0].capture_graph(masks="rle")
    torch.cuda.synchronize()
    _sentinels(pipe)
    for k in range(9):
        slot = k % 4
        if slot == 0 and k % 8 == 0:
            with torch.cuda.stream(pipe.streams[0]):
                g.replay()
        else:
            pipe.rerun(slot)
            assert pipe.last_stream(slot) == slot and pipe.exec_stream(slot) is pipe.streams[slot]
    assert pipe.null_exec == -1
    torch.cuda.synchronize()
    for slot in range(4):
        _same(pipe.collect(slot)[1], want[slot], f"slot {slot}")
    _clean(pipe)


def _hip_runtime():
    """The HIP runtime this process already has loaded, by its path (another copy must not be loaded beside it)."""
    for line in open("/proc/self/maps"):
        path = line.split()[-1]
        if "/" in path and path.rsplit("/", 1)[1].startswith("libamdhip64.so"):
            return ctypes.CDLL(path)
    pytest.fail("no libamdhip64.so among the process's mappings")


def test_every_stream_is_non_blocking():
    """The null stream synchronises implicitly with blocking streams: none of the pipeline's or the engines' may be one."""
    from cm3d_amd import lifting
    pipe = lifting.LiftPipeline("cuda:0", depth=4, null_exec=True)
    hip = _hip_runtime()
    hip.hipStreamGetFlags.argtypes = [ctypes.c_void_p, ctypes.POINTER(ctypes.c_uint)]
    hip.hipStreamGetFlags.restype = ctypes.c_int
    streams = list(pipe.streams) + [e.side for e in pipe.engines] + [lifting.LiftEngine("cuda:0").side]
    assert len(streams) == 9
    for st in streams:
        flags = ctypes.c_uint(0xFFFF)
        assert st.cuda_stream != 0
        assert hip.hipStreamGetFlags(ctypes.c_void_p(st.cuda_stream), ctypes.byref(flags)) == 0
        assert flags.value & 1 == 1, "a blocking stream"      # hipStreamNonBlocking
