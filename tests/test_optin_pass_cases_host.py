"""CPU: the batches of tests/optin_pass_cases.py hold what they are for, and the composed expectation is what it claims -- from the oracle
and the host statements alone.  Every number below is a condition on a recipe (which length ranges, routes and limits its lists must
reach for tests/test_gpu_optin_passes.py to say anything), not a measurement: a recipe that misses one gets another seed."""
import warnings

import numpy as np
import pytest

from cm3d_amd import _lib, cluster, nms
from tests import optin_pass_cases as oc

LONG = oc.MD_BATCH_LONG


def _lens(orc, name, c="own"):
    b = oc.batch(name)
    exp = oc.expected_of(orc, name, cluster=b.cluster if c == "own" else c)
    return np.diff(oc.plain(orc, name)["hit_off"]), np.diff(exp["cl_off"]), exp


def test_mid_reaches_every_range_of_the_medoid_stage_below_the_batch_long_limit(oracle):
    raw, cl, exp = _lens(oracle, "mid")
    assert raw.max() > LONG and cl.max() <= LONG              # the raw lists would send the batch down the two-pass route, the clustered do not
    lost = cl < raw
    assert lost.sum() >= 10
    assert ((cl[lost] >= 65) & (cl[lost] <= 256)).sum() >= 3 and ((cl[lost] >= 257) & (cl[lost] <= LONG)).sum() >= 2
    assert ((cl >= 1) & (cl <= 25)).any() and ((cl >= 26) & (cl <= 64)).any()
    assert set(exp["cl_status"].tolist()) == {cluster.KEPT, cluster.KEPT_WHOLE, cluster.EMPTY}
    assert (np.diff(exp["cl_tile_off"]) > 1).sum() >= 5      # more than one medoid tile per mask
    # the other pick chooses other clusters somewhere
    other = oc.expected_of(oracle, "mid", cluster=cluster.DepthCluster(1.0, 20, "nearest"))
    assert not np.array_equal(other["cl_off"], exp["cl_off"]) and not np.array_equal(other["medoid_pos"], exp["medoid_pos"])


def test_deep_sorts_beyond_the_lds_limit_and_keeps_long_clusters(oracle):
    raw, cl, exp = _lens(oracle, "deep")
    assert ((raw > _lib.DEPTH_CLUSTER_LDS_POINTS) & (cl < raw)).any()
    assert cl.max() > LONG and (raw == 0).any() and (exp["cl_status"] == cluster.EMPTY).any()
    # what the hint word must say of each batch in an engine with eps 1.0 (tests/test_gpu_optin_passes.py)
    _, cl1, _ = _lens(oracle, "deep", cluster.DepthCluster(1.0, 20))
    _, clm, _ = _lens(oracle, "mid", cluster.DepthCluster(1.0, 20))
    assert bool(cl1.max() > LONG) is True and bool(clm.max() > LONG) is False


def test_many_takes_the_rotated_nms_to_an_lds_bound_between_its_two_tested_ones(oracle):
    b = oc.batch("many")
    planes = (int(np.diff(b.hb.mask_off).max()) + 31) // 32
    assert 64 < 32 * planes < _lib.MAX_MASKS_PER_FRAME
    r = nms.RotatedNms(class_agnostic=True)
    for exp in (oc.plain(oracle, "many"), oc.expected_of(oracle, "many", cluster=b.cluster)):
        keep = oc.rotated_keep(exp["box"], exp["flags"], b.hb, r)
        for f in range(b.hb.n_frames):
            s = slice(int(b.hb.mask_off[f]), int(b.hb.mask_off[f + 1]))
            has = (exp["flags"][s] & 1) == 1
            assert has.sum() > 64, f
            assert (has & (keep[s] == 0)).sum() >= 10, f
            assert not np.array_equal(keep[s], exp["flags"][s] >> 1), f          # not the circle NMS's kept set


@pytest.mark.parametrize("name", oc.BATCH_NAMES)
def test_the_expectation_would_catch_a_pass_that_ignores_the_clustering(oracle, name):
    """expected(cluster=c) against expected(): medoid_pos on at least 5 masks, lane_dist and the box centre on at least 3.  `deep` has
    five masks, one of them empty by its own condition above, so four medoids are all that can move there: on it every mask with a
    point must differ (4); the other two figures hold as stated."""
    b = oc.batch(name)
    p, e = oc.plain(oracle, name), oc.expected_of(oracle, name, cluster=b.cluster)
    has = p["medoid_pos"] >= 0
    assert np.array_equal(has, e["medoid_pos"] >= 0)
    assert (e["medoid_pos"] != p["medoid_pos"]).sum() >= min(5, int(has.sum()))
    assert (e["lane_dist"][has] != p["lane_dist"][has]).sum() >= 3
    assert (e["box"][:, :3] != p["box"][:, :3]).any(1).sum() >= 3


@pytest.mark.parametrize("name", oc.BATCH_NAMES)
def test_one_cluster_per_list_is_the_plain_oracle(oracle, name):
    b = oc.batch(name)
    p = oc.plain(oracle, name)
    e = oc.expected(oracle, b.frames, b.lanes, b.frame_lane, b.hb, cluster=cluster.DepthCluster(float("inf"), 1), base=p)
    for key in p:
        assert e[key].dtype == p[key].dtype and e[key].tobytes() == p[key].tobytes(), key
    assert np.array_equal(e["cl_off"], p["hit_off"]) and np.array_equal(e["cl_idx"], p["hit_idx"])
    assert e["cl_xyz"].tobytes() == oc.hit_xyz_of(b.hb, p).tobytes()
    # neither option: oracle_batch's arrays themselves
    n = oc.expected(oracle, b.frames, b.lanes, b.frame_lane, b.hb, base=p)
    assert set(n) == set(p) and all(n[k] is p[k] for k in p)


def test_expected_without_a_base_computes_the_plain_oracle(oracle):
    b = oc.batch("many")
    p = oc.plain(oracle, "many")
    n = oc.expected(oracle, b.frames, b.lanes, b.frame_lane, b.hb)
    assert set(n) == set(p) and all(n[k].dtype == p[k].dtype and n[k].tobytes() == p[k].tobytes() for k in p)


def test_filters_in_the_composition_are_the_moved_restatement_on_the_drivable_scenario(oracle):
    from cm3d_amd import lifting
    from tests.helpers import oracle_batch
    from tests.test_gpu_drivable import FILTERS, build_scenario, check_scenario

    def plain(frames, lanes, frame_lane):
        hb = lifting.pack_frames(frames, lanes, frame_lane)
        return hb, oracle_batch(oracle, frames, lanes, frame_lane, hb)

    frames, lanes, frame_lane, tables, hb, res, pairs = build_scenario(plain)
    for kw in FILTERS:
        f = lifting.Stage2Filters(**kw)
        want = oc.expected_filtered(oracle, hb, res, lanes, frame_lane, frames, tables, f)
        got = oc.expected(oracle, frames, lanes, frame_lane, hb, filters=f, tables=tables, base=res)
        assert set(want) == {"on_road", "medoid_pos_kept", "box", "flags"}
        for key in want:
            assert got[key].dtype == want[key].dtype and got[key].tobytes() == want[key].tobytes(), (kw, key)
        for key in res:
            if key not in want:
                assert got[key] is res[key], key
        if kw == FILTERS[0]:
            check_scenario(hb, res, pairs, want)


@pytest.mark.parametrize("name", ["mid", "many"])
@pytest.mark.parametrize("clustered", [False, True], ids=["plain", "clustered"])
def test_lane_thresholds_from_the_expectation_drop_and_keep(oracle, name, clustered):
    c = oc.batch(name).cluster if clustered else None
    e = oc.expected_of(oracle, name, cluster=c)
    f = oc.lane_filters(e)
    thr = float(np.median(e["lane_dist"][e["medoid_pos"] >= 0]))
    assert (f.drivable, f.lane_max_dist, f.vehicle_lane_max_dist) == (False, thr, 0.75 * thr)
    ef = oc.expected_of(oracle, name, cluster=c, filters=f)
    dropped = (e["medoid_pos"] >= 0) & (ef["medoid_pos_kept"] < 0)
    assert dropped.sum() >= 3 and (ef["medoid_pos_kept"] >= 0).sum() >= 3
    assert np.array_equal(ef["flags"] & 1, (ef["medoid_pos_kept"] >= 0).astype(np.int32)) and not ef["on_road"].any()
    for key in e:                                            # everything in front of the filter stays
        if key not in ("box", "flags"):
            assert ef[key] is e[key], key


def test_obb_lists_of_mid_are_pinned_by_the_gap_rule(oracle):
    """The OBB comparison leaves out the lists test_gpu_obb's rule leaves out (relative eigenvalue gap below EIG_GAP_MIN: thin slices
    of a few points); what is left covers every length range of `mid`."""
    from cm3d_amd import kitti as kt
    from tests.test_gpu_obb import EIG_GAP_MIN
    assert EIG_GAP_MIN == 1e-3
    _, cl, exp = _lens(oracle, "mid")
    yaw, st, pinned = oc.obb_expected(exp, EIG_GAP_MIN)
    assert np.array_equal(st == kt.OBB_SKIPPED, cl <= 3) and (st == kt.OBB_SKIPPED).any() and not (st == kt.OBB_NO_HULL).any()
    assert np.isnan(yaw[st == kt.OBB_SKIPPED]).all() and np.isfinite(yaw[st == kt.OBB_FITTED]).all()
    fitted = st == kt.OBB_FITTED
    assert pinned.sum() >= 20 and pinned.sum() >= 0.75 * fitted.sum()
    assert (pinned & (cl <= 64)).sum() >= 3 and (pinned & (cl > 64) & (cl <= 256)).sum() >= 5 and (pinned & (cl > 256)).sum() >= 3
    p = oc.plain(oracle, "mid")
    lost = pinned & (cl < np.diff(p["hit_off"]))
    assert lost.sum() >= 8                                   # ... lists that lost points among them
    # a fit that saw the raw lists would show: their yaw is another one
    raw_xyz = oc.hit_xyz_of(oc.batch("mid").hb, p)
    moved = 0
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        for m in np.flatnonzero(lost):
            ry = kt.obb_canonical(raw_xyz[p["hit_off"][m]:p["hit_off"][m + 1], :3])[0]
            moved += int(abs((ry - yaw[m] + np.pi) % (2 * np.pi) - np.pi) > 1e-3)
    assert moved >= 5
