"""CPU: the batches of tests/inflight_cases.py hold what they are for -- from the oracle and the host statements alone.  Every number
below is a condition on the recipes (what each option must decide for tests/test_gpu_optin_in_flight.py to say anything about a slot
that reads its neighbour's data), not a measurement: a recipe that misses one gets other scenes."""
import functools

import numpy as np

from tests import inflight_cases as ic
from tests import velocity_pass_cases as pc


@functools.lru_cache(maxsize=None)
def _composed(k, drivable=False):
    from oracle import oracle as orc
    b = (ic.drivable_batches() if drivable else ic.nusc_batches())[k]
    return ic.composed(orc, b, b.polygons if drivable else None)


def _counts(c):
    """What each option decides in a composed pass: lists the clustering shortens, masks with a medoid the filter drops, fitted yaws,
    flags the rotated NMS changes against the circle NMS, masks with a velocity."""
    raw, cl = np.diff(c["plain"]["hit_off"]), np.diff(c["front"]["cl_off"])
    return dict(shortened=int((cl < raw).sum()), dropped=int(((c["front"]["medoid_pos"] >= 0) & (c["front"]["medoid_pos_kept"] < 0)).sum()),
                fitted=int((c["fit"]["yaw_src"] > 0).sum()), nms=int((c["flags"] != c["fit"]["flags"]).sum()),
                moving=int((c["vel"]["vel_src"] > 0).sum()))


def test_batch_zero_is_the_velocity_stage_batch(oracle):
    """Batch 0 is velocity_pass_cases.batch() -- the same HostBatch object -- and its composition here is expected_all_four's."""
    b = ic.nusc_batches()[0]
    assert b.hb is pc.batch().hb
    box, flags, vel = pc.expected_all_four()
    c = _composed(0)
    assert c["fit"]["box"].tobytes() == box.tobytes() and np.array_equal(c["flags"], flags)
    assert all(np.asarray(c["vel"][k]).tobytes() == np.asarray(vel[k]).tobytes() for k in ("next_match", "prev_match", "vel_src", "vel"))


def test_every_option_decides_something(oracle):
    counts = [_counts(_composed(k)) for k in range(len(ic.RECIPES))]
    print(counts)
    for k, n in enumerate(counts):                     # in every batch, the two table-set extras included
        assert n["shortened"] >= 3 and n["moving"] >= 8, (k, n)
    main = counts[:ic.N_MAIN]
    assert sum(n["dropped"] for n in main) >= 1 and sum(n["fitted"] for n in main) >= 1 and sum(n["nms"] for n in main) >= 1
    assert all(_composed(k)["vel"]["status"] == 0 for k in range(len(ic.RECIPES)))


def test_no_two_batches_look_alike():
    bs = ic.nusc_batches()
    offs = [b.hb.mask_off.tolist() for b in bs]
    assert all(offs[i] != offs[j] for i in range(len(bs)) for j in range(i))
    main = bs[:ic.N_MAIN]
    assert [b.hb.n_frames for b in main] == [6, 3, 4, 4] and len({b.hb.n_masks for b in main}) == ic.N_MAIN
    assert [b.hb.frame_next.tolist() for b in main] == [[1, 2, -1, 4, 5, -1], [1, 2, -1], [1, -1, 3, -1], [1, 2, 3, -1]]
    # every batch its own lane table of ONE yaw, so its own key in the engines' cache
    yaws = [np.unique(b.lanes[0][:, 2]).tolist() for b in bs]
    assert all(len(y) == 1 for y in yaws) and len({y[0] for y in yaws}) == len(bs)
    assert len({b.hb.lane_tables_key() for b in bs}) == len(bs)


def test_a_neighbours_lane_table_shows_in_the_pushed_boxes(oracle):
    """The yaw of a pushed box is its lane table's one yaw wherever the fit did not decide: with another batch's table every such box
    differs."""
    for k in range(ic.N_MAIN):
        c, yaw = _composed(k), ic.RECIPES[k][4]
        lane = ((c["flags"] & 1) == 1) & (c["fit"]["yaw_src"] == 0)
        assert lane.sum() >= 3 and (c["fit"]["box"][lane, 5] == np.float32(yaw)).all(), k


def test_the_drivable_set_has_a_table_per_batch_and_the_road_test_decides(oracle):
    bs = ic.drivable_batches()
    assert len({b.hb.polygon_tables_key() for b in bs}) == len(bs) and all(len(b.hb.polygons) == 1 for b in bs)
    assert all(b.hb is not p.hb and p.hb.polygons is None for b, p in zip(bs, ic.nusc_batches()))
    assert ic.five_options(True)["filters"].drivable and not ic.five_options()["filters"].drivable
    assert ic.five_options(True)["filters"].lane_max_dist == ic.five_options()["filters"].lane_max_dist == 2.5
    on = off = more = 0
    for k in range(ic.N_MAIN):
        c, lane_only = _composed(k, True), _composed(k)
        has = c["front"]["medoid_pos"] >= 0
        on, off = on + int((c["front"]["on_road"][has] == 1).sum()), off + int((c["front"]["on_road"][has] == 0).sum())
        more += int(((lane_only["front"]["medoid_pos_kept"] >= 0) & (c["front"]["medoid_pos_kept"] < 0)).sum())
    assert on >= 8 and off >= 8 and more >= 2            # medoids on and off the road; masks only the road test drops


def test_waymo_batches():
    bs = ic.waymo_batches()
    assert [b.hb.n_frames for b in bs] == [n for _, n in ic.WAYMO_RECIPES] and all(b.hb.pose_rt is not None for b in bs)
    offs = [b.hb.mask_off.tolist() for b in bs]
    assert all(offs[i] != offs[j] for i in range(len(bs)) for j in range(i))
    assert len({b.hb.lane_tables_key() for b in bs}) == len(bs) and all(len(b.lanes) == b.hb.n_frames for b in bs)
    assert all(b.hb.class_id[m] == b.classes.index("car") for b in bs for m in b.l_masks)
    o = ic.waymo_options()
    assert set(o) == {"classes", "cluster", "filters", "yaw", "nms"} and o["classes"].names == bs[0].classes.names
    assert not o["filters"].drivable and o["filters"].lane_max_dist == ic.WAYMO_LANE_MAX_DIST


def test_the_defaults_of_the_shared_builders_are_unchanged():
    """scene_frames(first_scene=0) and yaw_fit_pass_cases.batch(name) are what they were: batch() packs the same bytes."""
    from cm3d_amd import lifting
    from tests import yaw_fit_pass_cases as yc
    frames = pc.scene_frames(pc.config())
    assert [f.token for f in frames] == [f.token for f in pc.batch().frames]
    hb = lifting.pack_frames(frames, [pc.lane_table()], [0] * len(frames))
    assert hb.raw.tobytes() == pc.batch().hb.raw.tobytes() and hb.sweep_xf.tobytes() == pc.batch().hb.sweep_xf.tobytes()
    third = pc.scene_frames(pc.config(), 1, 2, first_scene=2)                    # a third scene: once an IndexError
    assert len(third) == 2 and third[0].next_token == third[1].token and third[1].next_token == ""
    step = third[1].sweep_xf[0, 21:23].astype(np.float64) - third[0].sweep_xf[0, 21:23].astype(np.float64)
    assert np.array_equal(step, pc.DT * pc.VELOCITY[0])                           # even scenes move, odd ones stand
    assert yc.batch("waymo") is yc.batch("waymo", 0, 2) and yc.batch("waymo", 2, 2) is not yc.batch("waymo")
