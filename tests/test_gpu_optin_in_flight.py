"""GPU: passes WITH opt-in stages the way the product runs them -- several different batches in flight in a LiftPipeline, slots reused
by uploads of other shapes, the engines sharing one cache of lane tables, lane indices and polygon indices, passes rotating over the
executing streams, the velocity call behind every pass -- and pipeline_nuscenes._lift_batches itself with every option on.

The yardstick is always a lone LiftEngine with the same options on the same batch (upload, run, synchronise, download(full=True)),
computed once per batch and option set; every comparison is byte equality over every key of the download, `vel` included: the kernels
are deterministic by their own statement, so there is no tolerance.  That the lone result is RIGHT is other modules' business
(test_gpu_velocity_pass pins batch 0's to the CPU composition); tests/test_inflight_cases_host.py holds that the batches differ where
it matters."""
import functools

import numpy as np
import pytest

from tests import inflight_cases as ic

pytestmark = pytest.mark.gpu

# every output an opt-in pass writes, and what the walks overwrite it with before every slot's last pass (the values of
# test_gpu_optin_passes._poison and its neighbours)
SENTINELS = dict(box=-3.0, flags=-3, medoid_pos=-3, centroid=-3.0, cl_off=-3, cl_idx=-3, cl_status=-3, cl_xyz=0.0, medoid_pos_kept=-3,
                 on_road=7, fit_k=-3, fit_status=-3, yaw_src=-3, next_match=-3, prev_match=-3, vel_src=-3, vel=-3.0)


def _options(name):
    return {"five": ic.five_options, "drivable": lambda: ic.five_options(True), "waymo": ic.waymo_options}[name]()


def _batches(name):
    return {"five": ic.nusc_batches, "drivable": ic.drivable_batches, "waymo": ic.waymo_batches}[name]()


def _ids(k, hb):
    return np.stack([1000.0 * k + np.arange(hb.n_frames), np.zeros(hb.n_frames)], 1)


@functools.lru_cache(maxsize=None)
def _lone(name, k):
    """Batch k of a set through a lone engine: (download(full=True), kept_box_records, kept_box_velocities or None).  Never written to."""
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
    torch.cuda.synchronize()
    assert (res["flags"] == 3).sum() >= 3 and res["hit_idx"].size > 20 and rec.shape[0] == ((res["flags"] & 3) == 3).sum()
    return res, rec, vel


def _same(got, want, what):
    assert set(got) == set(want), what
    for k in want:
        assert got[k].dtype == want[k].dtype and got[k].shape == want[k].shape, (what, k)
        assert got[k].tobytes() == want[k].tobytes(), (what, k)        # byte-equal, NaNs included


def _sentinels(engines):
    import torch
    torch.cuda.synchronize()
    n = 0
    for e in engines:
        for key, v in SENTINELS.items():
            if hasattr(e.b, key):
                getattr(e.b, key).fill_(v)
                n += 1
    torch.cuda.synchronize()
    return n


def _rotation(name, ks, depth, exec_streams, n_reruns=13):
    """`depth` different batches submitted, then n_reruns round-robin reruns -- each through LiftEngine.run on an acquired stream --
    with sentinels in every output before every slot's last pass."""
    from cm3d_amd import lifting
    bs = _batches(name)
    pipe = lifting.LiftPipeline("cuda:0", depth=depth, exec_streams=exec_streams, **_options(name))
    assert pipe.exec_streams == exec_streams and len(ks) == depth
    for slot, k in enumerate(ks):
        assert pipe.submit(bs[k].hb, "rle") == slot
    assert all(e.b.plain_pass is False for e in pipe.engines)           # `rerun` takes its Python branch: cm3d_pipe_submit knows the plain pass only
    for j in range(n_reruns - depth):
        pipe.rerun(j % depth)
    written = _sentinels(pipe.engines)
    assert written == depth * (len(SENTINELS) - (4 if name == "waymo" else 0))         # (no velocity stage in the Waymo layout)
    before = pipe.native_passes
    assert before == n_reruns                                           # `depth` submits and n_reruns - depth reruns so far
    for j in range(n_reruns - depth, n_reruns):                         # every slot's last pass
        pipe.rerun(j % depth)
        assert 0 <= pipe.last_stream(j % depth) < max(exec_streams, depth)
    assert pipe.native_passes == before + depth
    for slot, k in enumerate(ks):
        got_hb, got = pipe.collect(slot)
        assert got_hb is bs[k].hb
        _same(got, _lone(name, k)[0], f"{name}: batch {k} in slot {slot} on {exec_streams} streams")


@pytest.mark.parametrize("exec_streams", [1, 2, 3, 4])
def test_rotation_gives_every_slot_its_lone_result(exec_streams):
    """depth 4 on 1, 2, 3 and 4 executing streams, all five options: four different batches, 13 reruns."""
    _rotation("five", (0, 1, 2, 3), 4, exec_streams)


def test_rotation_in_the_waymo_layout():
    """Cluster, lane filter, yaw fit (which turns the lane's yaw by the frame's pose) and rotated NMS: depth 3 on 2 streams."""
    _rotation("waymo", (0, 1, 2), 3, 2)


def _walk(name, order, cache_log=None, **pipe_kw):
    """The batches `order` through submit / collect as pipeline_nuscenes._lift_batches does it: the slot about to be reused is
    collected, then uploaded into.  Each collect is the lone download; collect_records and kept_box_velocities are the lone engine's."""
    import torch
    from cm3d_amd import lifting
    bs = _batches(name)
    pipe = lifting.LiftPipeline("cuda:0", **pipe_kw, **_options(name))
    cache = pipe.engines[0]._lane_cache
    assert all(e._lane_cache is cache for e in pipe.engines)
    pending, held = [], {}

    def drain(keep):
        while len(pending) > keep:
            slot, k, j = pending.pop(0)
            res, rec, vel = _lone(name, k)
            what = f"{name}: upload {j} (batch {k}) in slot {slot}"
            if j % 2:                                            # the product's way (records only) and the tests' (everything) in turn
                got_rec = pipe.collect_records(slot, _ids(k, bs[k].hb)).cpu().numpy()
                got_vel = lifting.kept_box_velocities(pipe.engines[slot].b).cpu().numpy()
                torch.cuda.synchronize()
                assert got_rec.tobytes() == rec.tobytes() and got_vel.tobytes() == vel.tobytes(), what
            got_hb, got = pipe.collect(slot)
            assert got_hb is bs[k].hb
            _same(got, res, what)
            if slot in held:
                assert held[slot] != bs[k].hb.mask_off.tolist(), what        # the slot held a batch of another shape
            held[slot] = bs[k].hb.mask_off.tolist()
    for j, k in enumerate(order):
        drain(pipe.depth - 1)
        keys = list(cache)
        slot = pipe.submit(bs[k].hb, "rle")
        assert slot == j % pipe.depth
        pending.append((slot, k, j))
        if cache_log is not None:
            assert len(cache) <= 8
            cache_log.append((k, [key for key in keys if key not in cache], [key for key in cache if key not in keys]))
    drain(0)
    return pipe


@pytest.mark.parametrize("pipe_kw", [dict(depth=2), dict(depth=3, exec_streams=2)], ids=["depth2", "depth3_on_2_streams"])
def test_slot_reuse_with_uploads(pipe_kw):
    """Eight uploads, the four batches twice in two orders: every slot receives a batch of another shape than it held."""
    order = (0, 1, 2, 3, 1, 0, 3, 2) if pipe_kw["depth"] == 2 else (0, 1, 2, 3, 2, 3, 1, 0)
    _walk("five", order, **pipe_kw)


def test_slot_reuse_with_the_drivable_filter_evicts_and_rebuilds_cache_entries():
    """With the drivable-area test a batch takes two entries of the shared cache of eight, its lane tables' and its polygon tables'.
    Six table sets: the fifth evicts the first batch's entries while the pipeline still runs, and every batch that comes back after
    its entries went is uploaded and indexed again."""
    log = []
    order = (0, 1, 2, 3, 4, 5, 1, 0, 3, 2, 2)
    pipe = _walk("drivable", order, cache_log=log, depth=2)
    bs = _batches("drivable")
    keys = lambda k: {bs[k].hb.lane_tables_key(), bs[k].hb.polygon_tables_key()}
    for j, (k, gone, new) in enumerate(log):
        print(f"upload {j}: batch {k}, {len(new)} entries added, {len(gone)} evicted")
    assert all(set(new) == keys(k) and not gone for k, gone, new in log[:4])                  # eight entries, none evicted yet
    evicted_of = (0, 1, 2, 3, 4, 5)                                                              # first in, first out, two at a time
    for (k, gone, new), victim in zip(log[4:10], evicted_of):
        assert set(new) == keys(k) and set(gone) == keys(victim), (k, victim)
    assert log[10] == (2, [], [])                                                                # resident: neither uploaded nor evicted
    assert len(pipe.engines[0]._lane_cache) == 8 and sum(len(gone) for _, gone, _ in log) == 12


def test_lift_batches_with_every_option(monkeypatch):
    """pipeline_nuscenes._lift_batches in process: six batches through its depth-2 pipeline with filter, cluster, yaw fit, rotated NMS
    and velocity on -- 11 stage events per pass, the velocities beside the records, on_records once per batch with that batch's rows
    and velocity share."""
    import torch
    from cm3d_amd import lifting, pipeline_nuscenes as pn
    bs, o = _batches("drivable"), _options("drivable")
    order = (0, 1, 2, 3, 0, 1)
    firsts = np.concatenate([[0], np.cumsum([bs[k].hb.n_frames for k in order])])
    ids = [np.stack([np.arange(firsts[j], firsts[j + 1], dtype=np.float64), np.zeros(bs[k].hb.n_frames)], 1) for j, k in enumerate(order)]
    calls, timer, vel_out = [], {key: 0.0 for key in pn.REFERENCE_BUCKETS}, []
    n_events = []
    real_submit = lifting.LiftPipeline.submit

    def submit(self, hb, masks="rle", stage_events=None):
        slot = real_submit(self, hb, masks, stage_events=stage_events)
        n_events.append(len(stage_events))
        return slot
    monkeypatch.setattr(lifting.LiftPipeline, "submit", submit)
    rec = pn._lift_batches(((bs[k].hb, ids[j], 0.0) for j, k in enumerate(order)), "cuda:0", lifting.ClassTable.nuscenes(), "rle", timer,
                           on_records=lambda *a: calls.append(a), filters=o["filters"], cluster=o["cluster"], nms=o["nms"], yaw=o["yaw"],
                           velocity=o["velocity"], vel_out=vel_out)
    torch.cuda.synchronize()
    assert n_events == [5 + 2 + 2 + 2] * len(order)
    want_rec, want_vel = [], []
    for j, k in enumerate(order):
        _, r, v = _lone("drivable", k)
        r = r.copy()
        r[:, lifting.REC_FRAME_A] += firsts[j] - 1000.0 * k                      # the lone records carry _ids(k)
        want_rec.append(r); want_vel.append(v)
    assert rec.cpu().numpy().tobytes() == np.concatenate(want_rec, 0).tobytes()
    assert len(vel_out) == 1 and vel_out[0].cpu().numpy().tobytes() == np.concatenate(want_vel, 0).tobytes()
    assert len(calls) == len(order)
    for j, (got_rec, first, count, got_vel) in enumerate(calls):
        assert (first, count) == (firsts[j], firsts[j + 1] - firsts[j]), j
        assert got_rec.tobytes() == want_rec[j].tobytes() and got_vel.tobytes() == want_vel[j].tobytes(), j
        assert got_vel.shape == (got_rec.shape[0], 2)
    print({key: timer[key] for key in pn.REFERENCE_BUCKETS + ("cluster", "yawfit")})
    assert timer["cluster"] > 0 and timer["yawfit"] > 0 and timer["drivable"] > 0 and timer["medoid"] >= 0
    assert all(np.isfinite(timer[key]) and timer[key] >= 0 for key in pn.REFERENCE_BUCKETS)


def test_one_captured_graph_of_all_five_options():
    """The pass with four opt-in stages and the velocity call behind it in one captured graph: the replay writes the eager bytes."""
    import torch
    from cm3d_amd import lifting
    want = _lone("five", 0)[0]
    eng = lifting.LiftEngine("cuda:0", **_options("five"))
    eng.upload(_batches("five")[0].hb)
    eng.run(masks="rle")
    torch.cuda.synchronize()
    _same(eng.download(full=True), want, "eager")
    assert _sentinels([eng]) == len(SENTINELS)               # (on_road and medoid_pos_kept exist with the lane filter too)
    g = eng.capture_graph(masks="rle")
    g.replay()
    torch.cuda.synchronize()
    _same(eng.download(full=True), want, "replayed")
