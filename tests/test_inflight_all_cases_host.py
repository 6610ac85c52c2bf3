"""CPU: the batches of tests/inflight_all_cases.py hold what they are for -- from the oracle and the host statements alone.  Every number
below is a condition on the recipes (what each of the ten stages must decide, in EVERY batch, for tests/test_gpu_all_stages_in_flight.py
to say anything about a slot that reads its neighbour's data), not a measurement: a recipe that misses one gets other scenes."""
import functools
import itertools

import numpy as np

from tests import box_ground_cases as gc
from tests import box_size_pass_cases as sp
from tests import inflight_all_cases as ac
from tests import inflight_cases as ic
from tests import velocity_pass_cases as pc

# per batch, in the composition with all ten options: at least this many
THRESHOLDS = dict(shortened=10, kept=10, placed=8, tracked=10, sized=3, vertical=10, ground=10)


@functools.lru_cache(maxsize=None)
def _composed(k):
    from oracle import oracle as orc
    return ac.composed(orc, ac.nusc_batches()[k])


@functools.lru_cache(maxsize=None)
def _composed_waymo(k):
    from oracle import oracle as orc
    return ac.composed_waymo(orc, ac.waymo_batches()[k])


def _counts(c):
    st = c["stages"]
    raw, cl = np.diff(c["plain"]["hit_off"]), np.diff(c["front"]["cl_off"])
    return dict(shortened=int((cl < raw).sum()), kept=int(((st["nms"]["flags"] & 3) == 3).sum()), placed=int((st["place"]["place_src"] > 0).sum()),
                tracked=int((st["tracks"]["track_len"] >= 2).sum()), sized=int((st["size"]["size_src"] > 0).sum()),
                vertical=int((st["vertical"]["vert_src"] > 0).sum()), ground=int((st["ground"]["ground_src"] > 0).sum()))


def test_every_stage_decides_something_in_every_batch(oracle):
    counts = [_counts(_composed(k)) for k in range(len(ac.RECIPES))]
    for k, n in enumerate(counts):
        print(f"batch {k}: {n}")
        assert all(n[key] >= least for key, least in THRESHOLDS.items()), (k, n)
    # (box_size_pass_cases.composed asserts status 0 for the velocity and the track stage and for the size stage on its way)
    assert all(_composed(k)["size"]["status"] == 0 for k in range(len(ac.RECIPES)))
    cs = [_composed(k) for k in range(len(ac.RECIPES))]
    dropped = sum(int(((c["front"]["medoid_pos"] >= 0) & (c["front"]["medoid_pos_kept"] < 0)).sum()) for c in cs)
    assert dropped >= 1                                          # the filter drops a mask that has a medoid
    occur = lambda stage, key: set(np.concatenate([c["stages"][stage][key] for c in cs]).tolist())
    assert {1, 2, 3} <= occur("size", "size_src") and {1, 2} <= occur("vertical", "vert_src") and {1, 2} <= occur("ground", "ground_src")
    # the rotated NMS changes a flag the placement's circle NMS left
    changed = sum(int((c["rotated_flags"] != c["circle_flags"]).sum()) for c in cs)
    print(f"the filter drops {dropped} masks with a medoid; the rotated NMS changes {changed} keep bits")
    assert changed >= 1


def test_no_two_batches_look_alike():
    bs = ac.nusc_batches()
    assert [b.hb.n_frames for b in bs] == [6, 3, 4, 4] and [b.hb.n_masks for b in bs] == [54, 24, 40, 44]
    assert all(b.hb.n_frames <= 6 and b.hb.n_masks <= 54 and (b.hb.width, b.hb.height) == (512, 288) for b in bs)
    for a, b in itertools.combinations(bs, 2):
        assert a.hb.mask_off.tolist() != b.hb.mask_off.tolist() and a.hb.frame_next.tolist() != b.hb.frame_next.tolist()
        assert a.hb.lane_tables_key() != b.hb.lane_tables_key()
    assert [b.hb.frame_next.tolist() for b in bs] == [[1, 2, -1, 4, 5, -1], [1, 2, -1], [1, -1, 3, -1], [1, 2, 3, -1]]
    yaws = [np.unique(b.lanes[0][:, 2]).tolist() for b in bs]
    assert yaws == [[r[4]] for r in ac.RECIPES] and len({y[0] for y in yaws}) == len(bs)
    assert all(b.l_masks == [int(m) - 1 for m in b.hb.mask_off[1:]] for b in bs)


def test_batch_zero_is_the_size_stage_batch_and_its_composition(oracle):
    """Batch 0 is box_size_pass_cases.batch() -- the same object -- and its composition here is what box_size_pass_cases.composed
    gives without a batch argument, byte for byte: the optional argument changed nothing for the callers that do not pass it."""
    from tests import optin_pass_cases as oc
    from tests.helpers import oracle_batch
    b, o = ac.nusc_batches()[0], ac.ten_options()
    assert b is sp.batch() and ac.RECIPES[0][:3] == ic.RECIPES[0][:3]
    plain = oracle_batch(oracle, b.frames, b.lanes, b.frame_lane, b.hb)
    front = oc.expected(oracle, b.frames, b.lanes, b.frame_lane, b.hb, cluster=o["cluster"], filters=o["filters"], base=plain)
    before, out = sp.composed(oracle, front, o["nms"], tracks=(2, "mean", 2), y=o["yaw"])
    c = _composed(0)
    assert set(before) == set(c["before"]) and set(out) == set(c["size"])
    for got, want in ((c["before"], before), (c["size"], out)):
        for k, v in want.items():
            assert np.asarray(got[k]).dtype == np.asarray(v).dtype and np.asarray(got[k]).tobytes() == np.asarray(v).tobytes(), k
    # and with every default: the composition test_gpu_box_size_pass pins the engine to
    d_before, d_out = sp.composed(oracle)
    e_before, e_out = sp.composed(oracle, b=sp.batch())
    assert all(np.asarray(d_before[k]).tobytes() == np.asarray(e_before[k]).tobytes() for k in d_before)
    assert all(np.asarray(d_out[k]).tobytes() == np.asarray(e_out[k]).tobytes() for k in d_out)
    # the chain's last two stages on it are the composition test_gpu_box_ground_pass makes for this batch
    vert, ground = gc.pass_expected(b, front, before["box"], before["flags"], ac.G, ac.V)
    assert all(np.asarray(c["ground"][k]).tobytes() == np.asarray(ground[k]).tobytes() for k in ground)
    assert all(np.asarray(c["vert"][k]).tobytes() == np.asarray(vert[k]).tobytes() for k in vert)


def test_a_neighbours_data_would_show(oracle):
    """For every pair of batches and every stage, every per-mask array the stage leaves, cut to the shorter batch's mask count, differs:
    a slot that read its neighbour's arrays could not produce its own lone bytes."""
    cs = [_composed(k) for k in range(len(ac.RECIPES))]
    assert set(cs[0]["stages"]) == set(ac.STAGE_KEYS) and len(ac.STAGE_KEYS) == 10
    for i, j in itertools.combinations(range(len(cs)), 2):
        m = min(ac.nusc_batches()[i].hb.n_masks, ac.nusc_batches()[j].hb.n_masks)
        for stage, keys in ac.STAGE_KEYS.items():
            for key in keys:
                a, b = cs[i]["stages"][stage][key], cs[j]["stages"][stage][key]
                assert a.dtype == b.dtype and a.shape[1:] == b.shape[1:] and a[:m].tobytes() != b[:m].tobytes(), (i, j, stage, key)
        assert cs[i]["box"][:m].tobytes() != cs[j]["box"][:m].tobytes()


def test_the_options():
    o = ac.ten_options()
    assert set(o) == {"cluster", "filters", "yaw", "nms", "place", "velocity", "tracks", "size", "vertical", "ground"}
    assert all(o[k] == v for k, v in pc.all_four_options().items()) and o["place"] is sp.P and o["size"] is sp.S
    assert o["velocity"] == pc.settings()[0] and (o["tracks"].min_length, o["tracks"].smooth_window) == (2, 2)
    w = ac.waymo_options()
    assert set(w) == set(ic.waymo_options()) | {"place", "vertical", "ground"} and not {"velocity", "tracks", "size"} & set(w)
    assert all(w[k] == v for k, v in ic.waymo_options().items() if k != "classes") and w["classes"].names == ic.waymo_options()["classes"].names


def test_waymo_batches(oracle):
    bs = ac.waymo_batches()
    assert [b.hb.n_frames for b in bs] == [n for _, n in ic.WAYMO_RECIPES] and all(b.hb.pose_rt is not None for b in bs)
    for a, b in itertools.combinations(bs, 2):
        assert a.hb.mask_off.tolist() != b.hb.mask_off.tolist() and a.hb.lane_tables_key() != b.hb.lane_tables_key()
    assert all(b.hb.n_frames <= 6 and b.hb.n_masks <= 54 for b in bs)
    for k in range(len(bs)):
        c = _composed_waymo(k)
        n = dict(ground=int((c["ground"]["ground_src"] > 0).sum()), vertical=int((c["vert"]["vert_src"] > 0).sum()),
                 placed=int((c["place"]["place_src"] > 0).sum()))
        print(f"waymo batch {k}: {n}")
        assert n["ground"] >= 3 and n["vertical"] >= 3 and n["placed"] >= 2, (k, n)


def test_the_defaults_of_the_shared_builders_are_unchanged():
    """box_ground_cases.pass_batch(name) is what it was: the default batch under its name, the frames from 0, the same bytes as a batch
    asked for with the defaults spelled out; another first frame is another batch."""
    for name in ("nusc", "waymo"):
        b = gc.pass_batch(name)
        assert b is gc.pass_batch(name, 0, 2) and b.hb.n_frames == 2 and b.frame_lane == [0, 1]
    w = gc.pass_batch("waymo")
    other = gc.pass_batch("waymo", 2, 2)
    assert other is not w and other is gc.pass_batch("waymo", 2, 2) and other.hb.raw.tobytes() != w.hb.raw.tobytes()
    assert [f.token for f in w.frames] != [f.token for f in other.frames]
    gc._BATCHES.pop("waymo")                                       # built again from nothing: the bytes it had
    again = gc.pass_batch("waymo")
    assert again is not w and again.hb.raw.tobytes() == w.hb.raw.tobytes() and again.hb.mask_off.tolist() == w.hb.mask_off.tolist()
    assert again.hb.rle_counts.tobytes() == w.hb.rle_counts.tobytes() and again.l_heading == w.l_heading
    gc._BATCHES["waymo"] = w
