"""LiftPipeline on fewer executing streams than slots (cm3d_pipe_*, csrc/pipe_sched.h) and the native pass submitter (cm3d_lift_pass):
whatever stream a pass lands on and whoever enqueues it, every slot's download is byte for byte that of a lone LiftEngine.run."""
import functools

import numpy as np
import pytest

from cm3d_amd import synthetic as syn

pytestmark = pytest.mark.gpu


def _batch(k, n_frames, lane_points=3000):
    from cm3d_amd import lifting
    cfg = syn.config("tiny")
    frames = [syn.make_frame(cfg, 100 * k + i) for i in range(n_frames)]
    lanes = [syn.make_lane_table(frames[0].ego_xyz[:2], lane_points + 100 * k, seed=k)]        # every batch its own lane table (and index)
    return lifting.pack_frames(frames, lanes, [0] * n_frames)


def _lone(hb, masks="rle", **kw):
    import torch
    from cm3d_amd import lifting
    eng = lifting.LiftEngine(**kw)
    eng.upload(hb)
    if masks == "dense":
        eng.decode_masks_dense()
    eng.run(masks=masks)
    torch.cuda.synchronize()
    return eng.download()


@functools.lru_cache(maxsize=None)
def _four():
    """Four different batches of 2, 3, 4 and 5 frames and their lone results (computed once, never written to)."""
    hbs = [_batch(k, 2 + k) for k in range(4)]
    return hbs, [_lone(hb) for hb in hbs]


def _same(got, want, what):
    assert set(got) == set(want), what
    for k in want:
        assert got[k].dtype == want[k].dtype and got[k].shape == want[k].shape, (what, k)
        assert got[k].tobytes() == want[k].tobytes(), (what, k)        # byte-equal, NaNs included


def _sentinels(pipe):
    import torch
    torch.cuda.synchronize()
    for e in pipe.engines:
        e.b.hit_idx.fill_(-7); e.b.box.fill_(0)          # whatever the last pass does not rewrite would show
    torch.cuda.synchronize()


@pytest.mark.parametrize("exec_streams", [1, 2, 3, 4])
def test_rotation_gives_every_slot_its_lone_result(exec_streams):
    """depth 4 on 1, 2, 3 and 4 executing streams: 13 round-robin reruns (a multiple of neither 3 nor 4) of four different batches."""
    from cm3d_amd import lifting
    hbs, want = _four()
    assert all(w["hit_idx"].size > 20 for w in want)
    pipe = lifting.LiftPipeline("cuda:0", depth=4, exec_streams=exec_streams)
    assert pipe.exec_streams == exec_streams and len(pipe.streams) == 4 and len(pipe.engines) == 4
    for k in range(4):
        assert pipe.submit(hbs[k], "rle") == k
    n_pass = 4

    def rerun(k):
        nonlocal n_pass
        pipe.rerun(k % 4)
        assert pipe.last_stream(k % 4) == (k % 4 if exec_streams == 4 else n_pass % exec_streams)
        n_pass += 1
    for k in range(9):
        rerun(k)
    _sentinels(pipe)
    before = pipe.native_passes
    for k in range(9, 13):                               # every slot's last pass
        rerun(k)
    assert pipe.native_passes == before + 4              # the lane indices are complete by now: steady-state passes
    for slot in range(4):
        got_hb, got = pipe.collect(slot)
        assert got_hb is hbs[slot]
        _same(got, want[slot], f"slot {slot} on {exec_streams} streams")


def test_slot_reuse_with_uploads():
    """depth 3 on 2 executing streams: eight batches of different frame counts and lane tables through submit / collect."""
    from cm3d_amd import lifting
    hbs4, want4 = _four()
    hbs = list(hbs4) + [_batch(10 + k, n) for k, n in enumerate((1, 3, 2, 4))]
    want = list(want4) + [_lone(hb) for hb in hbs[4:]]
    pipe = lifting.LiftPipeline("cuda:0", depth=3, exec_streams=2)
    pending = []
    for j, hb in enumerate(hbs):
        if len(pending) == pipe.depth:
            slot, i = pending.pop(0)
            got_hb, got = pipe.collect(slot)
            assert got_hb is hbs[i]
            _same(got, want[i], f"batch {i} in slot {slot}")
        slot = pipe.submit(hb, "rle")
        assert slot == j % 3 and pipe.last_stream(slot) == j % 2
        pending.append((slot, j))
    for slot, i in pending:
        _same(pipe.collect(slot)[1], want[i], f"batch {i} in slot {slot}")


def test_native_pass_equals_python_pass():
    """cm3d_lift_pass against LiftEngine.run on one engine; through a pipeline the plain batch counts as a native pass (with or without a pair
    of events around the projection kernel), and dense masks, per-stage timing events, a Waymo batch with poses, a mixed-mask-size batch and
    the OBB fit each go through `run` -- with equal results."""
    import torch
    from cm3d_amd import lifting
    from cm3d_amd._lib import check
    from tests import mixed_size_cases as X
    hbs, want = _four()
    hb, ref = hbs[2], want[2]
    eng = lifting.LiftEngine()
    eng.upload(hb)
    eng.run(masks="rle")
    torch.cuda.synchronize()
    _same(eng.download(), ref, "python pass")
    assert eng.native_pass_ready("rle") and not eng.native_pass_ready("dense")
    eng.b.hit_idx.fill_(-7); eng.b.box.fill_(0)
    check(eng.lib.cm3d_lift_pass(eng.refresh_pass_descriptor(), torch.cuda.current_stream().cuda_stream), "cm3d_lift_pass")
    torch.cuda.synchronize()
    _same(eng.download(), ref, "native pass")

    def through(pipe, hb, want, native, masks="rle", submit_kw=None, rerun_kw=None, what=""):
        slot = pipe.submit(hb, masks, **(submit_kw or {}))
        _same(pipe.collect(slot)[1], want, what + ": first pass")
        n0 = pipe.native_passes
        pipe.engines[slot].b.hit_idx.fill_(-7); pipe.engines[slot].b.box.fill_(0)
        torch.cuda.synchronize()
        pipe.rerun(slot, **(rerun_kw or {}))
        assert pipe.native_passes == n0 + (1 if native else 0), what
        _same(pipe.collect(slot)[1], want, what + ": second pass")

    pipe = lifting.LiftPipeline("cuda:0", depth=2, exec_streams=1)
    through(pipe, hb, ref, True, what="plain")
    n0 = pipe.native_passes
    slot = pipe.submit(hb, "rle")                    # the lane tables are cached and their index complete: the upload's pass is native too
    assert pipe.native_passes == n0 + 1
    _same(pipe.collect(slot)[1], ref, "plain, submit")
    through(pipe, hb, _lone(hb, "dense"), False, masks="dense", what="dense masks")
    ev = []
    n0 = pipe.native_passes
    slot = pipe.submit(hb, "rle", stage_events=ev)
    assert pipe.native_passes == n0 and len(ev) == 5
    _same(pipe.collect(slot)[1], ref, "stage_events")
    pe = (torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True))
    # a pair of events around the projection kernel rides on the native pass (the library records it), so that a timed pass costs the host what
    # an untimed one does -- tests/test_gpu_bench_contract.py holds bench.py's timed region, whose every pass carries such a pair on a small run,
    # to within 30 % of its untimed regions; on an engine alone (`run`) the same pair takes the Python path
    through(pipe, hb, ref, True, rerun_kw=dict(project_events=pe), what="project_events, native")
    torch.cuda.synchronize()
    assert pe[0].elapsed_time(pe[1]) > 0
    assert not pipe.engines[0].native_pass_ready("rle", project_events=pe)
    mixed = X.mixed_tiny_frames(3)
    lanes = [syn.make_lane_table(mixed[0].ego_xyz[:2], 3000, seed=5)]
    hb_m = lifting.pack_frames(mixed, lanes, [0] * 3)
    assert hb_m.mask_wh is not None
    through(pipe, hb_m, _lone(hb_m), False, what="mixed mask sizes")
    through(lifting.LiftPipeline("cuda:0", depth=2, exec_streams=1, obb=True), hb, _lone(hb, obb=True), False, what="obb")
    cfg = syn.config("tiny", n_cams=5)
    frames = [syn.make_waymo_frame(cfg, i) for i in range(3)]
    centre = np.asarray(frames[0].pose).reshape(4, 4)[:2, 3]
    classes = lifting.ClassTable.waymo()
    hb_w = lifting.pack_frames(frames, [syn.make_lane_table(centre, 30000, seed=4, extent=400.0)], [0] * 3, classes)
    assert hb_w.pose_rt is not None
    through(lifting.LiftPipeline("cuda:0", depth=2, exec_streams=1, classes=classes), hb_w, _lone(hb_w, classes=classes), False, what="waymo")


def test_lane_rebuild_under_rotation():
    """rebuild_lane_grid() before every rerun (a benchmark's unamortised region), four slots on three streams."""
    from cm3d_amd import lifting
    hbs, want = _four()
    pipe = lifting.LiftPipeline("cuda:0", depth=4, exec_streams=3)
    for hb in hbs:
        pipe.submit(hb, "rle")
    for k in range(9):
        pipe.engines[k % 4].rebuild_lane_grid()
        pipe.rerun(k % 4)
    _sentinels(pipe)
    n0 = pipe.native_passes
    for k in range(9, 13):
        pipe.engines[k % 4].rebuild_lane_grid()
        pipe.rerun(k % 4)
    assert pipe.native_passes == n0                      # a pass that builds the index is not the steady-state pass
    for slot in range(4):
        _same(pipe.collect(slot)[1], want[slot], f"slot {slot}")


def test_graph_capture_pins_the_slots():
    """After capture_graph on one engine of a pipeline every later pass of slot s runs on streams[s]; replays interleaved with reruns
    give the eager results."""
    import torch
    from cm3d_amd import lifting
    hbs, want = _four()
    pipe = lifting.LiftPipeline("cuda:0", depth=3, exec_streams=2)
    for hb in hbs[:3]:
        pipe.submit(hb, "rle")
    for k in range(4):
        pipe.rerun(k % 3)
    assert [pipe.last_stream(s) for s in range(3)] == [0, 0, 1]      # passes 6, 4, 5 on two streams: rotating so far
    torch.cuda.synchronize()
    with torch.cuda.stream(pipe.streams[1]):
        g = pipe.engines[1].capture_graph(masks="rle")
    torch.cuda.synchronize()
    _sentinels(pipe)
    for k in range(9):
        slot = k % 3
        if slot == 1 and k % 2 == 0:
            with torch.cuda.stream(pipe.streams[1]):
                g.replay()
        else:
            pipe.rerun(slot)
            assert pipe.last_stream(slot) == slot
    torch.cuda.synchronize()
    for slot in range(3):
        _same(pipe.collect(slot)[1], want[slot], f"slot {slot}")
    slot = pipe.submit(hbs[3], "rle")                    # uploads stay on the slot's own stream too
    assert pipe.last_stream(slot) == slot
    _same(pipe.collect(slot)[1], want[3], "upload after the capture")
