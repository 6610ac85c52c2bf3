"""GPU: passes with ALL TEN opt-in stages the way the product runs them -- cluster, filters, yaw fit, placement and rotated NMS inside
the native pass call, and the vertical, ground, velocity, track and size stages as separate library calls enqueued behind it
(LiftEngine.run) -- with several DIFFERENT batches in flight in a LiftPipeline, slots reused by uploads of other shapes, passes rotating
over fewer executing streams than slots, the chain in one captured graph, and pipeline_nuscenes._lift_batches itself with every keyword.

The yardstick is always a lone LiftEngine with the same options on the same batch (upload, run, synchronise, download(full=True),
kept_box_records, kept_box_velocities, kept_box_sizes), computed once per batch and set; every in-flight comparison is byte equality
over every key of the download: the kernels are deterministic by their own statement, so there is no tolerance.  That the lone result
is RIGHT is pinned here too, for all four nuScenes batches, against the CPU composition of tests/inflight_all_cases.py with the
comparisons (and the tolerances, none new) that the size, track, velocity, vertical and ground pass tests make for the first of them;
tests/test_inflight_all_cases_host.py holds that the batches differ in every array of every stage, so that equality with the lone
engine says something about cross-slot reads."""
import functools

import numpy as np
import pytest

from cm3d_amd import boxground as bg
from cm3d_amd import boxvertical as bv
from tests import box_size_pass_cases as sp
from tests import inflight_all_cases as ac
from tests import velocity_pass_cases as pc
from tests.test_gpu_optin_in_flight import SENTINELS as FIVE_SENTINELS, _ids, _same

pytestmark = pytest.mark.gpu

# every output array of every opt-in stage, and what the walks overwrite it with before every slot's last pass: the five earlier stages'
# (test_gpu_optin_in_flight) and the five new ones'.  The one-word vel_status, track_status and size_status are not poisoned: the
# kernels only raise them; they must read 0 afterwards.
SENTINELS = dict(FIVE_SENTINELS, place_src=-3, place_pushed=-3.0, track_id=-3, track_pos=-3, track_len=-3, track_stat=-3.0, vel_smooth=-3.0,
                 **{k: (-3 if k in ("size_src", "size_obs") else -3.0) for k in sp.SIZE_KEYS},
                 **{k: (-3 if k in ("vert_src", "vert_status") else -3.0) for k in bv.RESULTS},
                 **{k: (-3 if k in ("ground_n", "ground_src", "ground_status") else -3.0) for k in bg.RESULTS})
VELOCITY_KEYS = ("next_match", "prev_match", "vel_src", "vel")
TRACK_KEYS = ("track_id", "track_pos", "track_len", "track_stat", "vel_smooth")
# the arrays an engine of each set has: the nuScenes set all of them, the Waymo layout none of the velocity, track and size stages'
N_SENTINELS = dict(ten=len(SENTINELS), waymo=len(SENTINELS) - len(VELOCITY_KEYS) - len(TRACK_KEYS) - len(sp.SIZE_KEYS))
STATUS_WORDS = ("vel_status", "track_status", "size_status")
VEL_TOL = pc.BOX_TOL * 2 / pc.DT                     # tests/test_gpu_velocity_pass.py: two centres within BOX_TOL over a span of at least DT


def _options(name):
    return {"ten": ac.ten_options, "waymo": ac.waymo_options}[name]()


def _batches(name):
    return {"ten": ac.nusc_batches, "waymo": ac.waymo_batches}[name]()


@functools.lru_cache(maxsize=None)
def _lone(name, k):
    """Batch k of a set through a lone engine: (download(full=True), kept_box_records, kept_box_velocities or None, kept_box_sizes).
    Never written to."""
    import torch
    from cm3d_amd import lifting
    hb = _batches(name)[k].hb
    eng = lifting.LiftEngine("cuda:0", **_options(name))
    eng.upload(hb)
    eng.run(masks="rle")
    torch.cuda.synchronize()
    res = eng.download(full=True)
    rec = lifting.kept_box_records(eng.b, _ids(k, hb)).cpu().numpy()
    vel = lifting.kept_box_velocities(eng.b).cpu().numpy() if eng.velocity is not None else None
    sizes = lifting.kept_box_sizes(eng.b).cpu().numpy()
    torch.cuda.synchronize()
    _statuses_zero([eng])
    assert (res["flags"] == 3).sum() >= 3 and res["hit_idx"].size > 20 and rec.shape[0] == ((res["flags"] & 3) == 3).sum() == sizes.shape[0]
    assert set(bg.RESULTS) | set(bv.RESULTS) | {"place_src", "place_pushed", "cl_off", "medoid_pos_kept", "yaw_src"} <= set(res)
    if name == "ten":
        assert set(VELOCITY_KEYS) | set(TRACK_KEYS) | set(sp.SIZE_KEYS) <= set(res) and vel.shape == (rec.shape[0], 2)
        keep = (res["flags"] & 3) == 3               # the product's rows: the sized velocities, the sized extents beside the ground stage's height
        assert vel.tobytes() == res["size_vel"][keep].tobytes() and sizes[:, 2].tobytes() == res["ground_h"][keep].tobytes()
        assert sizes[:, :2].tobytes() == np.ascontiguousarray(res["size_wlh"][keep, :2]).tobytes()
    return res, rec, vel, sizes


def _sentinels(engines):
    import torch
    torch.cuda.synchronize()
    n = 0
    for e in engines:
        for key, v in SENTINELS.items():
            if getattr(e.b, key, None) is not None:
                getattr(e.b, key).fill_(v)
                n += 1
    torch.cuda.synchronize()
    return n


def _statuses_zero(engines):
    for e in engines:
        for key in STATUS_WORDS:
            if hasattr(e.b, key):
                assert int(getattr(e.b, key).item()) == 0, key


# ------------------------------------------------------------------------------------------------ (a) the lone engine is right
def _bits(a):
    return np.ascontiguousarray(a, np.float64).view(np.uint64)


def _assert_front(got, front, fit):
    """The stages inside the pass call: the clustered lists, the medoids, the filter's verdict, the fit -- to the bit -- and column 5
    under test_gpu_yaw_fit_pass's rule (the lane's yaw to the bit, a fitted one within one float32 ulp at pi)."""
    for k in ("cl_off", "cl_status", "cl_idx", "medoid_pos", "medoid_pos_kept", "lane_idx"):
        assert got[k].dtype == np.int32 and np.array_equal(got[k], front[k]), k
    assert np.array_equal(got["cl_xyz"].view(np.uint32), np.asarray(front["cl_xyz"], np.float32).view(np.uint32))
    assert np.array_equal(got["centroid"].view(np.uint32), front["centroid"].view(np.uint32))
    for k in ("yaw_src", "fit_status", "fit_k"):
        assert got[k].dtype == np.int32 and np.array_equal(got[k], fit[k]), k
    assert np.array_equal(got["fit_rect"].view(np.uint64), fit["fit_rect"].view(np.uint64))
    lane = fit["yaw_src"] == 0
    assert np.array_equal(got["box"][lane, 5], fit["box"][lane, 5]) and np.abs(got["box"][~lane, 5] - fit["box"][~lane, 5]).max() <= 2.0 ** -22


def _assert_vertical_and_ground(got, vert, ground):
    """The two stages' results and column 2 of the masks each judged: to the bit (test_gpu_box_vertical_pass, test_gpu_box_ground_pass)."""
    for k in ("vert_status", "vert_src") + ("ground_status", "ground_src", "ground_n"):
        exp = (vert if k.startswith("vert") else ground)[k]
        assert got[k].dtype == np.int32 and np.array_equal(got[k], exp), (k, np.flatnonzero(got[k] != exp))
    for k in ("vert_z", "vert_h") + ("ground_z", "ground_h", "ground_zref"):
        exp = (vert if k.startswith("vert") else ground)[k]
        assert np.array_equal(_bits(got[k]), _bits(exp)), (k, np.flatnonzero((_bits(got[k]) != _bits(exp)).reshape(len(exp), -1).any(1)))
    assert got["vert_entry_z"].tobytes() == got["ground_zref"].tobytes()
    by_ground, by_vert = ground["ground_src"] > 0, (vert["vert_src"] > 0) & (ground["ground_src"] == 0)
    assert np.array_equal(_bits(got["box"][by_ground, 2]), _bits(ground["box"][by_ground, 2]))
    assert np.array_equal(_bits(got["box"][by_vert, 2]), _bits(vert["box"][by_vert, 2]))
    rest = ~by_ground & ~by_vert                     # left alone by both: the z the pass wrote
    assert got["box"][rest, 2].tobytes() == got["vert_entry_z"][rest].tobytes()
    left = ground["ground_src"] == 0                 # (the height of a box the ground stage left alone is the vertical stage's)
    assert got["ground_h"][left].tobytes() == got["vert_h"][left].tobytes()
    return by_ground, by_vert


@pytest.mark.parametrize("k", [0, 1, 2, 3])
def test_the_lone_engine_equals_the_cpu_composition(oracle, k):
    """Every stage of the lone ten-stage engine against inflight_all_cases.composed, with the comparisons of the pass tests: integers,
    flags, sources, matches, track arrays, sizes, ratios, the vertical and the ground stage's results and the centres of placed and sized
    boxes to the bit; every other centre within velocity_pass_cases.BOX_TOL, `vel` within 2 BOX_TOL / DT, vel_smooth and size_vel within
    the bound test_gpu_tracks_pass derives from BOX_TOL and the frame times."""
    from tests.test_gpu_tracks_pass import smooth_bound
    b = ac.nusc_batches()[k]
    c = ac.composed(oracle, b)
    before, out, hb = c["before"], c["size"], b.hb
    got = _lone("ten", k)[0]
    _assert_front(got, c["front"], before)
    # placement, rotated NMS, track stage: sources and flags exact; the scores the track stage rewrote and column 9
    assert np.array_equal(got["place_src"], before["place_src"]) and np.array_equal(got["flags"], out["flags"])
    assert np.array_equal(got["flags"], before["flags"])
    assert np.array_equal(got["box"][:, 7], before["box"][:, 7]) and np.array_equal(got["box"][:, 9], before["box"][:, 9])
    placed = before["place_src"] > 0
    assert np.abs(got["place_pushed"] - c["stages"]["place"]["place_pushed"]).max() <= pc.BOX_TOL       # (the centres the placement found)
    # velocity: the matches exact, vel within VEL_TOL (test_gpu_velocity_pass)
    for key in ("next_match", "prev_match"):
        assert np.array_equal(got[key], before[key]), key
    assert np.abs(got["vel"] - before["vel"]).max() <= VEL_TOL
    # tracks (test_gpu_tracks_pass) and size (test_gpu_box_size_pass)
    for key in ("track_id", "track_pos", "track_len"):
        assert np.array_equal(got[key], before[key]), key
    bound = smooth_bound(hb, before, ac.TR[2])
    assert (np.abs(got["vel_smooth"] - before["vel_smooth"]).max(1) <= bound).all() and (bound > 0).sum() >= 10
    for key in ("size_src", "size_obs"):
        assert np.array_equal(got[key], out[key]), key
    assert got["size_wlh"].tobytes() == out["size_wlh"].tobytes() and got["size_ratio"].tobytes() == out["size_ratio"].tobytes()
    assert got["box"][placed, :2].tobytes() == out["box"][placed, :2].tobytes()
    assert np.abs(got["box"][:, :2] - out["box"][:, :2]).max() <= pc.BOX_TOL
    assert np.abs(got["size_placed"] - before["box"][:, :2]).max() <= pc.BOX_TOL
    err = np.abs(got["size_vel"] - out["size_vel"]).max(1)
    assert (err <= bound).all()
    # vertical and ground: they judged the centres the placement left, in front of the three stages above
    by_ground, by_vert = _assert_vertical_and_ground(got, c["vert"], c["ground"])
    print(f"batch {k}: {int(placed.sum())} placed, {int((out['size_src'] > 0).sum())} sized, {int(by_ground.sum())} stood on the ground, "
          f"{int(by_vert.sum())} more by the vertical stage; max |size_vel - composed| = {err.max():.3e} (bound {bound.max():.3e})")
    for m in b.l_masks:                              # the car of two faces: its yaw is the fitted one in every frame of every batch
        assert got["yaw_src"][m] == 1 and got["fit_status"][m] == 0 and got["flags"][m] & 1


@pytest.mark.parametrize("k", [0, 1, 2])
def test_the_lone_waymo_engine_equals_the_host_statements_on_the_composed_front(oracle, k):
    """The Waymo layout: placement, vertical and ground stage against their host statements on the CPU's clustered, filtered and fitted
    pass (the sensor is the origin of the vehicle frame; the rotated NMS behind the placement leaves bit 0 of the flags)."""
    b = ac.waymo_batches()[k]
    c = ac.composed_waymo(oracle, b)
    got = _lone("waymo", k)[0]
    _assert_front(got, c["front"], c["fit"])
    pl = c["place"]
    on = pl["place_src"] > 0
    assert got["place_src"].dtype == np.int32 and np.array_equal(got["place_src"], pl["place_src"]) and on.sum() >= 2
    assert got["box"][on, :2].tobytes() == pl["box"][on, :2].tobytes() and np.array_equal(got["flags"] & 1, pl["flags"] & 1)
    assert np.abs(got["place_pushed"] - pl["place_pushed"]).max() <= pc.BOX_TOL
    by_ground, by_vert = _assert_vertical_and_ground(got, c["vert"], c["ground"])
    assert by_ground.sum() >= 3 and not {"vel", "track_id", "size_wlh"} & set(got)


# ------------------------------------------------------------------------------------------------ (b), (c), (g) rotation
def _rotation(name, ks, depth, exec_streams, n_reruns=13, **engine_kw):
    """`depth` different batches submitted, then round-robin reruns up to n_reruns passes in all -- each through LiftEngine.run on an
    acquired stream, the five calls behind the pass on that stream too --, with sentinels in every output of every stage before every
    slot's last pass.  Returns [(slot's download, the lone download)]."""
    from cm3d_amd import lifting
    bs = _batches(name)
    pipe = lifting.LiftPipeline("cuda:0", depth=depth, exec_streams=exec_streams, **engine_kw, **_options(name))
    assert pipe.exec_streams == exec_streams and len(ks) == depth
    for slot, k in enumerate(ks):
        assert pipe.submit(bs[k].hb, "rle") == slot
    assert all(e.b.plain_pass is False for e in pipe.engines)           # no engine has the plain pass: `rerun` takes its Python branch
    for j in range(n_reruns - depth):
        pipe.rerun(j % depth)
    assert _sentinels(pipe.engines) == depth * N_SENTINELS[name]        # (a renamed attribute cannot silently drop out)
    before = pipe.native_passes
    assert before == n_reruns                                           # `depth` submits and n_reruns - depth reruns so far
    for j in range(n_reruns - depth, n_reruns):                         # every slot's last pass
        pipe.rerun(j % depth)
        assert 0 <= pipe.last_stream(j % depth) < max(exec_streams, depth)
    assert pipe.native_passes == before + depth
    out = []
    for slot, k in enumerate(ks):
        got_hb, got = pipe.collect(slot)
        assert got_hb is bs[k].hb
        out.append((got, _lone(name, k)[0]))
    _statuses_zero(pipe.engines)
    return out


@pytest.mark.parametrize("exec_streams", [1, 2, 3, 4])
def test_rotation_gives_every_slot_its_lone_result(exec_streams):
    """depth 4 on 1, 2, 3 and 4 executing streams, all ten options: the four batches in the four slots, 13 passes."""
    for slot, (got, want) in enumerate(_rotation("ten", (0, 1, 2, 3), 4, exec_streams)):
        _same(got, want, f"ten: batch {slot} in slot {slot} on {exec_streams} streams")


def test_rotation_with_the_cloud_materialised():
    """keep_cloud: the ground stage reads each slot's own `points` instead of the raw rows; every key but `points` is the bytes of the
    run without the cloud."""
    for slot, (got, want) in enumerate(_rotation("ten", (0, 1, 2, 3), 4, 2, keep_cloud=True)):
        assert "points" in got and "points" not in want and got["points"].shape == (int(got["pt_off"][-1]), 4)
        _same({k: v for k, v in got.items() if k != "points"}, want, f"ten with the cloud: batch {slot} in slot {slot}")


def test_rotation_in_the_waymo_layout():
    """Cluster, lane filter, yaw fit, placement, rotated NMS, vertical and ground on the Waymo class table: depth 3 on 2 streams."""
    assert N_SENTINELS["waymo"] == 26 and N_SENTINELS["ten"] == 41
    for slot, (got, want) in enumerate(_rotation("waymo", (0, 1, 2), 3, 2)):
        _same(got, want, f"waymo: batch {slot} in slot {slot}")


# ------------------------------------------------------------------------------------------------ (d) slot reuse with uploads
def _walk(name, order, **pipe_kw):
    """The batches `order` through submit / collect as pipeline_nuscenes._lift_batches does it: the slot about to be reused is
    collected, then uploaded into.  The collects alternate between the tests' way (everything) and the product's (collect_records,
    kept_box_velocities, kept_box_sizes of the slot's engine, then everything as well); each gives the lone engine's bytes."""
    import torch
    from cm3d_amd import lifting
    bs = _batches(name)
    pipe = lifting.LiftPipeline("cuda:0", **pipe_kw, **_options(name))
    pending, held = [], {}

    def drain(keep):
        while len(pending) > keep:
            slot, k, j = pending.pop(0)
            res, rec, vel, sizes = _lone(name, k)
            what = f"{name}: upload {j} (batch {k}) in slot {slot}"
            if j % 2:
                got_rec = pipe.collect_records(slot, _ids(k, bs[k].hb)).cpu().numpy()
                got_vel = lifting.kept_box_velocities(pipe.engines[slot].b).cpu().numpy()
                got_sizes = lifting.kept_box_sizes(pipe.engines[slot].b).cpu().numpy()
                torch.cuda.synchronize()
                assert got_rec.tobytes() == rec.tobytes(), what
                assert got_vel.tobytes() == vel.tobytes() and got_sizes.tobytes() == sizes.tobytes(), what
            got_hb, got = pipe.collect(slot)
            assert got_hb is bs[k].hb
            _same(got, res, what)
            _statuses_zero([pipe.engines[slot]])
            if slot in held:
                assert held[slot] != bs[k].hb.mask_off.tolist(), what        # the slot held a batch of another shape
            held[slot] = bs[k].hb.mask_off.tolist()
    for j, k in enumerate(order):
        drain(pipe.depth - 1)
        slot = pipe.submit(bs[k].hb, "rle")
        assert slot == j % pipe.depth
        pending.append((slot, k, j))
    drain(0)
    return pipe


WALKS = {"depth2": (dict(depth=2), (0, 1, 2, 3, 1, 0, 3, 2)), "depth3_on_2_streams": (dict(depth=3, exec_streams=2), (0, 1, 2, 3, 2, 3, 1, 0))}


@pytest.mark.parametrize("walk", sorted(WALKS))
def test_slot_reuse_with_uploads(walk):
    """Eight uploads, the four batches twice in two orders: every slot receives a batch of another shape than it held -- other frame
    links and times, other workspaces for the velocity, track and size stages, other rows for the ground stage to stream."""
    pipe_kw, order = WALKS[walk]
    _walk("ten", order, **pipe_kw)


# ------------------------------------------------------------------------------------------------ (e) _lift_batches
def test_lift_batches_with_every_keyword(monkeypatch):
    """pipeline_nuscenes._lift_batches in process: six batches through its depth-2 pipeline with all twelve keywords -- 17 stage events
    per pass, the velocities and sizes beside the records, on_records once per batch with that batch's rows, velocity and size share."""
    import torch
    from cm3d_amd import lifting, pipeline_nuscenes as pn
    bs, o = _batches("ten"), _options("ten")
    order = (0, 1, 2, 3, 0, 1)
    firsts = np.concatenate([[0], np.cumsum([bs[k].hb.n_frames for k in order])])
    ids = [np.stack([np.arange(firsts[j], firsts[j + 1], dtype=np.float64), np.zeros(bs[k].hb.n_frames)], 1) for j, k in enumerate(order)]
    calls, timer, vel_out, size_out = [], {key: 0.0 for key in pn.REFERENCE_BUCKETS}, [], []
    n_events = []
    real_submit = lifting.LiftPipeline.submit

    def submit(self, hb, masks="rle", stage_events=None):
        slot = real_submit(self, hb, masks, stage_events=stage_events)
        n_events.append(len(stage_events))
        return slot
    monkeypatch.setattr(lifting.LiftPipeline, "submit", submit)
    rec = pn._lift_batches(((bs[k].hb, ids[j], 0.0) for j, k in enumerate(order)), "cuda:0", lifting.ClassTable.nuscenes(), "rle", timer,
                           on_records=lambda *a: calls.append(a), filters=o["filters"], cluster=o["cluster"], nms=o["nms"], yaw=o["yaw"],
                           velocity=o["velocity"], vel_out=vel_out, tracks=o["tracks"], place=o["place"], size=o["size"], size_out=size_out,
                           vertical=o["vertical"], ground=o["ground"])
    torch.cuda.synchronize()
    # LiftEngine.run's docstring: five events, then a pair each for filter, cluster, yaw fit, placement, vertical and ground; the velocity,
    # track and size calls have none
    assert n_events == [5 + 2 * 6] * len(order)
    want_rec, want_vel, want_sizes = [], [], []
    for j, k in enumerate(order):
        _, r, v, s = _lone("ten", k)
        r = r.copy()
        r[:, lifting.REC_FRAME_A] += firsts[j] - 1000.0 * k                      # the lone records carry _ids(k)
        want_rec.append(r); want_vel.append(v); want_sizes.append(s)
    assert rec.cpu().numpy().tobytes() == np.concatenate(want_rec, 0).tobytes()
    assert len(vel_out) == 1 and vel_out[0].cpu().numpy().tobytes() == np.concatenate(want_vel, 0).tobytes()
    assert len(size_out) == 1 and size_out[0].cpu().numpy().tobytes() == np.concatenate(want_sizes, 0).tobytes()
    assert len(calls) == len(order)
    for j, (got_rec, first, count, got_vel, got_sizes) in enumerate(calls):
        assert (first, count) == (firsts[j], firsts[j + 1] - firsts[j]), j
        assert got_rec.tobytes() == want_rec[j].tobytes() and got_vel.tobytes() == want_vel[j].tobytes(), j
        assert got_sizes.tobytes() == want_sizes[j].tobytes() and got_vel.shape == (got_rec.shape[0], 2) and got_sizes.shape == (got_rec.shape[0], 3), j
    stage_buckets = ("cluster", "yawfit", "place", "vertical", "ground")
    print({key: timer[key] for key in pn.REFERENCE_BUCKETS + stage_buckets})
    assert all(timer[key] > 0 for key in stage_buckets + ("drivable",)) and timer["medoid"] >= 0
    assert all(np.isfinite(timer[key]) and timer[key] >= 0 for key in pn.REFERENCE_BUCKETS)


# ------------------------------------------------------------------------------------------------ (f) one captured graph
def test_one_captured_graph_of_all_ten_stages():
    """The pass and the five calls behind it in one captured graph: the replay writes the eager and lone bytes; so does the same
    engine's eager run afterwards."""
    import torch
    from cm3d_amd import lifting
    want = _lone("ten", 0)[0]
    eng = lifting.LiftEngine("cuda:0", **_options("ten"))
    eng.upload(_batches("ten")[0].hb)
    eng.run(masks="rle")
    torch.cuda.synchronize()
    _same(eng.download(full=True), want, "eager")
    assert _sentinels([eng]) == N_SENTINELS["ten"]
    g = eng.capture_graph(masks="rle")
    g.replay()
    torch.cuda.synchronize()
    _same(eng.download(full=True), want, "replayed")
    assert _sentinels([eng]) == N_SENTINELS["ten"]
    eng.run(masks="rle")
    torch.cuda.synchronize()
    _same(eng.download(full=True), want, "eager again")
    _statuses_zero([eng])


def test_a_captured_graph_in_a_pipeline_pins_the_slots():
    """Depth 2 rotating over ONE stream, two different batches, engine 0 captures its ten-stage pass (the device idle before and after,
    as LiftPipeline's rule says): from then on slot s stays on streams[s], and reruns, with the graph replayed in between, still give
    each slot its lone bytes."""
    import torch
    from cm3d_amd import lifting
    bs = _batches("ten")
    pipe = lifting.LiftPipeline("cuda:0", depth=2, exec_streams=1, **_options("ten"))
    for slot, k in enumerate((1, 2)):
        assert pipe.submit(bs[k].hb, "rle") == slot
    for slot in (0, 1):
        pipe.rerun(slot)
    assert [pipe.last_stream(s) for s in (0, 1)] == [0, 0]              # one executing stream: rotating so far
    torch.cuda.synchronize()
    with torch.cuda.stream(pipe.streams[0]):
        g = pipe.engines[0].capture_graph(masks="rle")
    torch.cuda.synchronize()
    assert _sentinels(pipe.engines) == 2 * N_SENTINELS["ten"]
    for j in range(3):
        for slot in (0, 1):
            pipe.rerun(slot)
            assert pipe.last_stream(slot) == slot
        if j == 1:
            with torch.cuda.stream(pipe.streams[0]):
                g.replay()
    torch.cuda.synchronize()
    for slot, k in enumerate((1, 2)):
        _same(pipe.collect(slot)[1], _lone("ten", k)[0], f"slot {slot} behind the capture")
    _statuses_zero(pipe.engines)
