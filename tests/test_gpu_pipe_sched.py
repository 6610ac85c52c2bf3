"""LiftPipeline on fewer executing streams than slots (cm3d_pipe_*, csrc/pipe_sched.h) and the pass submitter (cm3d_lift_pass):
whatever stream a pass lands on, every slot's download is byte for byte that of a lone LiftEngine.run, and LiftEngine.run's that of
the same pass made stage by stage."""
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


def _waymo_batch():
    from cm3d_amd import lifting
    cfg = syn.config("tiny", n_cams=5)
    frames = [syn.make_waymo_frame(cfg, i) for i in range(3)]
    centre = np.asarray(frames[0].pose).reshape(4, 4)[:2, 3]
    classes = lifting.ClassTable.waymo()
    hb = lifting.pack_frames(frames, [syn.make_lane_table(centre, 30000, seed=4, extent=400.0)], [0] * 3, classes)
    assert hb.pose_rt is not None
    return hb, classes


def _mixed_batch():
    from cm3d_amd import lifting
    from tests import mixed_size_cases as X
    mixed = X.mixed_tiny_frames(3)
    hb = lifting.pack_frames(mixed, [syn.make_lane_table(mixed[0].ego_xyz[:2], 3000, seed=5)], [0] * 3)
    assert hb.mask_wh is not None
    return hb


def _stage_by_stage(eng, masks):
    """The pass `run` makes, as the stage methods: the launches bench.py's per-stage figures time."""
    import torch
    st = torch.cuda.current_stream().cuda_stream
    fused = eng.can_fuse_sweeps()
    eng.stage_begin(st)
    if not fused:
        eng.stage_sweeps(st)
    eng.stage_masks(st, masks)
    if fused:
        eng.stage_sweep_project(st)
    else:
        eng.stage_project(st)
    eng.stage_compact(st)
    eng.stage_medoid(st)
    eng.wait_lane_grid()
    eng.stage_lanes(st)
    eng.stage_boxes(st)
    if eng.obb:
        eng.stage_obb(st)


@pytest.mark.parametrize("case", ["plain", "separate_reset", "dense", "sweeps17", "mixed_sizes", "waymo", "obb", "stage_events",
                                  "project_events"])
def test_run_equals_the_pass_stage_by_stage(case, monkeypatch):
    """LiftEngine.run (one cm3d_lift_pass) against the stage methods on one engine, sentinels written in between, for every branch of the
    pass: the reset on the mask launch or as a launch of its own (CM3D_FUSED_RESET=0), dense masks, a frame of 17 sweeps (separate sweep
    and projection launches), mixed mask sizes, Waymo poses, the OBB fit, and the two kinds of timing events."""
    import torch
    from cm3d_amd import lifting
    kw, masks, run_kw = {}, "rle", {}
    hb = _four()[0][1]                                   # three frames
    if case == "separate_reset":
        monkeypatch.setenv("CM3D_FUSED_RESET", "0")
    elif case == "dense":
        masks = "dense"
    elif case == "sweeps17":
        frames = [syn.make_frame(syn.config("tiny", n_sweeps=17, n_points=400), i) for i in range(2)]
        hb = lifting.pack_frames(frames, [syn.make_lane_table(frames[0].ego_xyz[:2], 3000, seed=1)], [0] * 2)
    elif case == "mixed_sizes":
        hb = _mixed_batch()
    elif case == "waymo":
        hb, kw["classes"] = _waymo_batch()
    elif case == "obb":
        kw["obb"] = True
    elif case == "stage_events":
        run_kw["stage_events"] = []
    elif case == "project_events":
        run_kw["project_events"] = (torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True))
    eng = lifting.LiftEngine(**kw)
    eng.fused_sweeps = True                              # (whatever CM3D_FUSED_SWEEPS says)
    eng.upload(hb)
    assert eng.can_fuse_sweeps() == (case != "sweeps17")
    if masks == "dense":
        eng.decode_masks_dense()
    _stage_by_stage(eng, masks)
    torch.cuda.synchronize()
    want = eng.download()
    assert want["hit_idx"].size > 20 and (want["flags"] == 3).any()
    eng.b.hit_idx.fill_(-7); eng.b.box.fill_(0); eng.b.lane_idx.fill_(-7); eng.b.medoid_pos.fill_(-7)
    if eng.obb:
        eng.b.obb_yaw.fill_(0); eng.b.obb_status.fill_(-7)
    torch.cuda.synchronize()
    eng.run(masks=masks, **run_kw)
    torch.cuda.synchronize()
    _same(eng.download(), want, case)
    # what the pass was told: the branch the case is about
    d = eng.b.desc
    assert bool(d.separate_reset) == (case == "separate_reset") and bool(d.dense) == (case == "dense") and bool(d.fused) == (case != "sweeps17")
    assert bool(d.mask_wh) == (case == "mixed_sizes") and bool(d.pose_rt) == bool(d.pose_inv) == (case == "waymo")
    assert bool(d.obb_yaw) == (case == "obb") and bool(d.points) == (case == "sweeps17")
    assert [bool(e) for e in d.ev_stage] == [case == "stage_events"] * 5 and [bool(e) for e in d.ev_project] == [case == "project_events"] * 2
    if case == "stage_events":
        ev = run_kw["stage_events"]
        assert len(ev) == 5 and all(a.elapsed_time(b) >= 0 for a, b in zip(ev, ev[1:]))
    if case == "project_events":
        assert run_kw["project_events"][0].elapsed_time(run_kw["project_events"][1]) > 0


def test_run_refuses_before_it_enqueues():
    from cm3d_amd import lifting
    from cm3d_amd._lib import Cm3dError
    eng = lifting.LiftEngine()
    eng.upload(_four()[0][0])
    ev = []
    with pytest.raises(Cm3dError, match="dense masks requested but not resident"):
        eng.run(masks="dense", stage_events=ev)
    with pytest.raises(ValueError):
        eng.run(masks="packed", stage_events=ev)
    assert ev == [] and not eng._lane["built"]           # nothing was started, no event handed out
    eng.upload(_mixed_batch())
    with pytest.raises(ValueError, match="different image sizes"):
        eng.run(masks="dense")


def test_native_pass_equals_python_pass():
    """cm3d_lift_pass called directly against LiftEngine.run on one engine; through a pipeline every pass counts as enqueued by cm3d_lift_pass
    -- the plain batch (with or without a pair of events around the projection kernel), dense masks, per-stage timing events, a Waymo batch
    with poses, a mixed-mask-size batch and the OBB fit -- with the results of a lone engine."""
    import torch
    from cm3d_amd import lifting
    from cm3d_amd._lib import check
    hbs, want = _four()
    hb, ref = hbs[2], want[2]
    eng = lifting.LiftEngine()
    eng.upload(hb)
    eng.run(masks="rle")
    torch.cuda.synchronize()
    _same(eng.download(), ref, "python pass")
    eng.b.hit_idx.fill_(-7); eng.b.box.fill_(0)
    check(eng.lib.cm3d_lift_pass(eng.refresh_pass_descriptor(), torch.cuda.current_stream().cuda_stream), "cm3d_lift_pass")
    torch.cuda.synchronize()
    _same(eng.download(), ref, "native pass")

    def through(pipe, hb, want, masks="rle", submit_kw=None, rerun_kw=None, what=""):
        slot = pipe.submit(hb, masks, **(submit_kw or {}))
        _same(pipe.collect(slot)[1], want, what + ": first pass")
        n0 = pipe.native_passes
        pipe.engines[slot].b.hit_idx.fill_(-7); pipe.engines[slot].b.box.fill_(0)
        torch.cuda.synchronize()
        pipe.rerun(slot, **(rerun_kw or {}))
        assert pipe.native_passes == n0 + 1, what
        _same(pipe.collect(slot)[1], want, what + ": second pass")

    pipe = lifting.LiftPipeline("cuda:0", depth=2, exec_streams=1)
    through(pipe, hb, ref, what="plain")
    n0 = pipe.native_passes
    slot = pipe.submit(hb, "rle")                    # the upload's pass too
    assert pipe.native_passes == n0 + 1
    _same(pipe.collect(slot)[1], ref, "plain, submit")
    through(pipe, hb, _lone(hb, "dense"), masks="dense", what="dense masks")
    ev = []
    n0 = pipe.native_passes
    slot = pipe.submit(hb, "rle", stage_events=ev)
    assert pipe.native_passes == n0 + 1 and len(ev) == 5
    _same(pipe.collect(slot)[1], ref, "stage_events")
    pe = (torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True))
    # a pair of events around the projection kernel rides in the descriptor (the library records it), so that a timed pass costs the host what
    # an untimed one does -- tests/test_gpu_bench_contract.py holds bench.py's timed region, whose every pass carries such a pair on a small run,
    # to within 30 % of its untimed regions
    through(pipe, hb, ref, rerun_kw=dict(project_events=pe), what="project_events")
    torch.cuda.synchronize()
    assert pe[0].elapsed_time(pe[1]) > 0
    hb_m = _mixed_batch()
    through(pipe, hb_m, _lone(hb_m), what="mixed mask sizes")
    through(lifting.LiftPipeline("cuda:0", depth=2, exec_streams=1, obb=True), hb, _lone(hb, obb=True), what="obb")
    hb_w, classes = _waymo_batch()
    through(lifting.LiftPipeline("cuda:0", depth=2, exec_streams=1, classes=classes), hb_w, _lone(hb_w, classes=classes), what="waymo")


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
    assert pipe.native_passes == n0 + 4                  # a pass that builds the index is enqueued by cm3d_lift_pass like every other
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
