"""CPU: the host statement of the box size stage (cm3d_amd.boxsize.box_size_host) against the separately written scalar loop of
tests/box_size_cases.py, to the bit, on every rule table and hostile case at the defaults and at q 0, 0.5 and 1; the pinned status
words and closed-form answers; the identity with lo = hi = 1; a second call on the arrays the first one left; the stage's switches
and the refusals of the command line."""
import argparse

import numpy as np
import pytest

from cm3d_amd import boxsize as bs
from cm3d_amd import tracks as T
from tests import box_size_cases as sc

CASES = sc.all_cases()
IDS = [c["name"] for c in CASES]


def _host(case, **kw):
    return bs.box_size_host(*sc.args_of(case), **dict(dict(thin=sc.THIN, max_dt=sc.MAX_DT), **kw))


@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_host_equals_the_scalar_loop_and_the_pinned_status(case):
    for run in case["runs"]:
        got, exp = _host(case, **run), sc.size_reference(case, **run)
        sc.assert_same(got, exp, (case["name"], run))
        assert got["status"] == case["status"], (case["name"], run)
        # what the stage never writes
        assert got["box"][:, 2:].tobytes() == case["box"][:, 2:].tobytes() and np.array_equal(got["flags"], case["flags"])
        assert got["size_placed"].tobytes() == case["box"][:, :2].tobytes()


def test_the_table_cases_are_what_the_track_stage_writes():
    """Track ids, positions and lengths of every well-formed table equal box_tracks_host's on the case's own links."""
    for c in sc.table_cases():
        tr = T.box_tracks_host(c["box"], c["flags"], c["mask_frame"], c["next_match"], c["prev_match"], c["frame_time"])
        assert tr["status"] == 0, c["name"]
        for k in ("track_id", "track_pos", "track_len"):
            assert np.array_equal(tr[k], c[k]), (c["name"], k)


def test_equal_ratios_the_position_decides():
    c = sc.by_name("equal_ratios_position_decides")
    for q, (rl, rw) in c["expect"]["ratio_by_q"].items():
        got = _host(c, q=q)
        assert (got["size_ratio"] == [rl, rw]).all() and (got["size_obs"] == 6).all() and (got["size_src"] == 3).all()
        assert (got["size_wlh"] == [rw * 2.0, rl * 4.0, 1.5]).all()


def test_a_ratio_on_lo_and_hi_is_an_observation_one_ulp_off_is_none():
    c = sc.by_name("ratio_on_and_one_ulp_off_lo_hi")
    got = _host(c)
    assert got["size_obs"][:, 0].tolist() == c["expect"]["obs_len"] and got["size_obs"][:, 1].tolist() == c["expect"]["obs_wid"]
    assert got["size_src"].tolist() == [3, 3, 3, 3, 2, 2, 2, 2]
    assert got["size_ratio"][:, 0].tolist() == [0.6, 0.6, 1.5, 1.5, 1.0, 1.0, 1.0, 1.0]


def test_min_obs_and_the_rank_of_the_quantile():
    c = sc.by_name("n_at_min_obs_and_q_on_an_integer")
    at = lambda ti, k=0: c["index"][ti, k]
    got = _host(c)
    assert [int(got["size_obs"][at(t), 0]) for t in range(3)] == [1, 2, 3]
    assert [int(got["size_src"][at(t)] & 1) for t in range(3)] == [0, 1, 1] and got["size_ratio"][at(0), 0] == 1.0
    got3 = _host(c, min_obs=3)
    assert [int(got3["size_src"][at(t)] & 1) for t in range(3)] == [0, 0, 1]
    got1 = _host(c, min_obs=1)
    assert [int(got1["size_src"][at(t)] & 1) for t in range(3)] == [1, 1, 1]
    five = c["expect"]["five"]
    for q, r in five["by_q"].items():
        assert _host(c, q=q)["size_ratio"][at(five["track"]), 0] == r, q


def test_members_that_kept_the_lane_yaw_get_the_prior_and_their_entry_centre():
    c = sc.by_name("place_src_0_head_inside_end")
    got = _host(c)
    z = c["place_src"] == 0
    assert z.any() and (got["size_src"][z] == 0).all() and got["box"][z].tobytes() == c["box"][z].tobytes()
    assert got["size_wlh"][z].tobytes() == c["prior_wlh"][1][None].repeat(z.sum(), 0).tobytes()
    all_zero = [c["index"][3, k] for k in range(5)]
    assert (got["size_obs"][all_zero] == 0).all() and (got["size_ratio"][all_zero] == 1.0).all()
    assert (got["size_obs"][c["index"][0, 0]] == 4).all()             # the head observes nothing, its four followers do


def test_dyadic_track_both_velocity_forms_exact():
    c = sc.by_name("dyadic_exact_velocity_and_a_span_over_max_dt")
    for W, vel in c["expect"]["vel"].items():
        for q in (0.0, 0.5, 0.75, 1.0):
            got = _host(c, smooth_window=W, q=q)
            assert np.array_equal(got["size_vel"], np.asarray(vel, np.float64)), (W, q)
            assert (got["size_wlh"][:9] == c["expect"]["wlh"]).all() and (got["size_wlh"][9] == c["prior_wlh"][0]).all()   # (one box: n < min_obs)
            assert np.array_equal(got["box"][:9, :2], c["fit_rect"][:9, :2])
    # the prior-sized entry centres are not on the grid: the test would not pass on them
    assert (c["box"][:9, :2] != c["fit_rect"][:9, :2]).any(1).all()
    # the gap of 2.0 s: with a max_dt that covers it the central difference returns; the window form never looks at max_dt
    wide = _host(c, max_dt=3.0)
    assert np.array_equal(wide["size_vel"][5:9], np.asarray([(2.0, 0.0)] * 4))


def test_extents_beyond_the_pooled_size_move_the_centre_inward():
    c = sc.by_name("centres_near_1_km_and_10_km")
    got = _host(c, q=0.0)
    m = (c["fit_rect"][:, 2] > got["size_wlh"][:, 1]) & (c["fit_rect"][:, 3] > got["size_wlh"][:, 0])
    assert m.sum() >= 5 and np.isfinite(got["box"][m, :2]).all()


@pytest.mark.parametrize("case", sc.identity_cases(), ids=lambda c: c["name"])
def test_identity_with_lo_hi_1(case):
    """Nothing is observed: the size is the prior's, the centre cm3d_box_place's own -- the input's bytes --, and the velocity the track
    stage's on the same centres."""
    for W in (0, 1, 3):
        got = _host(case, lo=1.0, hi=1.0, smooth_window=W)
        assert got["box"].tobytes() == case["box"].tobytes()
        cls = [sc._class_of(v, case["prior_wlh"].shape[0]) for v in case["box"][:, 8]]
        assert got["size_wlh"].tobytes() == case["prior_wlh"][cls].tobytes() and not got["size_src"].any() and not got["size_obs"].any()
        if W:
            tr = T.box_tracks_host(case["box"], case["flags"], case["mask_frame"], case["next_match"], case["prev_match"], case["frame_time"],
                                   smooth_window=W)
            assert got["size_vel"].tobytes() == tr["vel_smooth"].tobytes(), W
        else:
            assert got["size_vel"].tobytes() == _two_neighbour_velocity(case).tobytes()


def test_identity_through_the_chain_of_host_statements():
    """velocity -> tracks -> size on a scene in frame order: the association gives the case's links, the track stage its track arrays,
    and with lo = hi = 1 size_vel is track_velocity_host's vel (W = 0) and box_tracks_host's vel_smooth (W = 1, 3), to the bit."""
    from cm3d_amd import velocity as V
    c = sc.chain_case()
    v = V.track_velocity_host(c["box"], c["flags"], c["mask_off"], c["class_id"], c["frame_next"], c["frame_time"], c["track_group"],
                              c["max_speed"], sc.MAX_DT)
    assert np.array_equal(v["next_match"], c["next_match"]) and np.array_equal(v["prev_match"], c["prev_match"]) and v["status"] == 0
    for W in (0, 1, 3):
        tr = T.box_tracks_host(c["box"], c["flags"], c["mask_frame"], v["next_match"], v["prev_match"], c["frame_time"], smooth_window=W)
        got = bs.box_size_host(c["box"], c["flags"], c["mask_frame"], c["fit_rect"], c["place_src"], c["prior_wlh"], c["ego_xyz"],
                               v["next_match"], v["prev_match"], tr["track_id"], tr["track_pos"], tr["track_len"], c["frame_time"],
                               thin=sc.THIN, max_dt=sc.MAX_DT, smooth_window=W, lo=1.0, hi=1.0)
        assert got["status"] == 0 and got["box"].tobytes() == c["box"].tobytes()
        assert got["size_vel"].tobytes() == (tr["vel_smooth"] if W else v["vel"]).tobytes(), W
        assert np.abs(got["size_vel"]).max() > 0.5


def _two_neighbour_velocity(case):
    """velocity.track_velocity_host's last loop on the case's own links (its association is not run here: the links are given)."""
    box, t = case["box"], case["frame_time"][case["mask_frame"]]
    vel = np.zeros((len(t), 2))
    for i in np.flatnonzero((case["flags"] & 3) == 3):
        nm, pm = int(case["next_match"][i]), int(case["prev_match"][i])
        tp, tm = (t[nm] if nm >= 0 else t[i]), (t[pm] if pm >= 0 else t[i])
        if nm >= 0 and pm >= 0 and tp - tm <= sc.MAX_DT:
            vel[i] = (box[nm, :2] - box[pm, :2]) / (tp - tm)
        elif nm >= 0 and tp - t[i] <= sc.MAX_DT:
            vel[i] = (box[nm, :2] - box[i, :2]) / (tp - t[i])
        elif pm >= 0 and t[i] - tm <= sc.MAX_DT:
            vel[i] = (box[i, :2] - box[pm, :2]) / (t[i] - tm)
    return vel


@pytest.mark.parametrize("case", [c for c in CASES if len(c["flags"])][:12], ids=lambda c: c["name"])
def test_a_second_call_gives_the_same_box(case):
    first = _host(case)
    again = bs.box_size_host(first["box"], first["flags"], *sc.args_of(case)[2:], thin=sc.THIN, max_dt=sc.MAX_DT)
    assert again["box"].tobytes() == first["box"].tobytes() and again["size_wlh"].tobytes() == first["size_wlh"].tobytes()
    assert again["size_vel"].tobytes() == first["size_vel"].tobytes() and again["size_placed"].tobytes() == first["box"][:, :2].tobytes()


def test_bad_arguments():
    c = sc.by_name("equal_ratios_position_decides")
    for kw in (dict(q=-0.1), dict(q=1.5), dict(q=float("nan")), dict(min_obs=0), dict(lo=0.0), dict(lo=1.2, hi=1.1), dict(hi=float("inf")),
               dict(lo=float("nan")), dict(thin=-1.0), dict(thin=float("inf")), dict(max_dt=0.0), dict(smooth_window=-1)):
        with pytest.raises(ValueError):
            _host(c, **kw)
        if set(kw) <= {"q", "min_obs", "lo", "hi"}:
            with pytest.raises(ValueError):
                bs.BoxSize(**kw)
    d = bs.BoxSize()
    assert (d.q, d.min_obs, d.lo, d.hi) == (0.75, 2, 0.6, 1.5) and d.active


def _parser():
    from cm3d_amd import bevfit, boxplace, velocity
    ap = argparse.ArgumentParser()
    ap.add_argument("--yaw", choices=("lane", "fit"), default="lane")
    boxplace.add_arguments(ap)
    velocity.add_arguments(ap)
    bs.add_arguments(ap)
    return ap


FULL = ["--yaw", "fit", "--place", "fit", "--velocity", "track"]


def test_command_line_refusals():
    ap = _parser()
    assert bs.from_args(ap.parse_args([])) is None and bs.from_args(ap.parse_args(["--size", "prior"])) is None
    assert bs.from_args(ap.parse_args(FULL + ["--size", "track"])) == bs.BoxSize()
    got = bs.from_args(ap.parse_args(FULL + ["--size", "track", "--size-quantile", "0.5", "--size-min-obs", "3", "--size-ratio", "0.7,1.4"]))
    assert got == bs.BoxSize(0.5, 3, 0.7, 1.4)
    refused = [["--size", "track"], ["--size", "track", "--place", "fit", "--velocity", "track"], ["--size", "track", "--yaw", "fit", "--velocity", "track"],
               ["--size", "track", "--yaw", "fit", "--place", "fit"], ["--size-quantile", "0.5"], ["--size", "prior", "--size-min-obs", "2"],
               FULL + ["--size-ratio", "0.6,1.5"], FULL + ["--size", "track", "--size-ratio", "0.6"], FULL + ["--size", "track", "--size-ratio", "1.5,0.6"],
               FULL + ["--size", "track", "--size-quantile", "1.1"], FULL + ["--size", "track", "--size-min-obs", "0"]]
    for argv in refused:
        with pytest.raises(ValueError):
            bs.from_args(ap.parse_args(argv))
        with pytest.raises(SystemExit):
            bs.from_args(ap.parse_args(argv), ap)
    assert "untuned" in ap.format_help().lower()


def test_the_entry_point_refuses_before_any_work():
    from cm3d_amd import pipeline_nuscenes
    for argv in (["--size", "track"], ["--size", "track", "--yaw", "fit", "--place", "fit"], ["--size-quantile", "0.5"],
                 FULL + ["--size", "prior", "--size-ratio", "0.6,1.5"]):
        with pytest.raises(SystemExit) as e:
            pipeline_nuscenes.main(argv)
        assert e.value.code == 2, argv


# ---------------------------------------------------------------------------------------------------------------- writers
def _records_sizes():
    from tests.test_velocity_host import _records_and_velocities
    rec, vel, tokens, classes = _records_and_velocities()
    rng = np.random.default_rng(17)
    size = rng.uniform(0.3, 12.0, (len(rec), 3))
    size[:8] = [[1.9, 4.5, 1.7], [2.0, 5.0, 1.5], [0.0, -0.0, 1.0], [1e-7, 2.5e-5, 1e22], [np.inf, 1.0, 2.0], [1.0, -np.inf, np.nan],
                [1.9000000000000001, 4.499999999999999, 1.7], [5e-324, 1.7976931348623157e308, 0.1]]
    return rec, vel, size, tokens, classes


@pytest.mark.parametrize("with_vel", [True, False])
def test_writers_agree_given_sizes(with_vel):
    import json
    from cm3d_amd import lifting
    rec, vel, size, tokens, classes = _records_sizes()
    vel = vel if with_vel else None
    meta = {"use_camera": True}
    as_dicts = json.dumps({"meta": meta, "results": lifting.nuscenes_boxes_from_records(rec, tokens, classes, vel=vel, size=size)})
    text, n = lifting.nuscenes_results_json(rec, tokens, classes, meta, vel=vel, size=size)
    native = lifting.nuscenes_results_json_native(rec, tokens, classes, meta, vel=vel, size=size)
    assert n == len(rec) and text == as_dicts and native == text.encode()
    assert '"size": [2.0, 5.0, 1.5]' in text and '"size": [0.0, -0.0, 1.0]' in text and '"size": [Infinity, 1.0, 2.0]' in text
    assert '"size": [1.0, -Infinity, NaN]' in text and ('"velocity": [0, 0]' in text) == (not with_vel)
    parts = []
    for first, count in ((0, 3), (3, 2), (5, 2)):
        sel = (rec[:, 5] >= first) & (rec[:, 5] < first + count)
        parts.append(lifting.nuscenes_results_json_native(rec[sel], tokens, classes, None, part=(first, count), vel=None if vel is None else vel[sel],
                                                          size=size[sel]))
    if len(tokens) == 7:
        assert lifting.nuscenes_results_json_head(meta) + b", ".join(parts) + b"}}" == native
    for fn in (lifting.nuscenes_results_json, lifting.nuscenes_results_json_native, lifting.nuscenes_boxes_from_records):
        with pytest.raises(ValueError):
            fn(rec, tokens, classes, size=size[:-1])


def test_writers_without_sizes_write_todays_bytes():
    import json
    from cm3d_amd import lifting
    rec, vel, size, tokens, classes = _records_sizes()
    meta = {"use_camera": True}
    for v in (None, vel):
        boxes = lifting.nuscenes_boxes_from_records(rec, tokens, classes, vel=v, size=None)
        assert json.dumps(boxes) == json.dumps(lifting.nuscenes_boxes_from_records(rec, tokens, classes, vel=v))
        assert all(b["size"] == [float(x) for x in classes.prior_wlh[classes.names.index(b["detection_name"])]] for bl in boxes.values() for b in bl)
        text, _ = lifting.nuscenes_results_json(rec, tokens, classes, meta, vel=v, size=None)
        assert text == json.dumps({"meta": meta, "results": boxes}) == lifting.nuscenes_results_json(rec, tokens, classes, meta, vel=v)[0]
        assert lifting.nuscenes_results_json_native(rec, tokens, classes, meta, vel=v, size=None) == text.encode()
    # the prior rows given as sizes write the same text as no sizes
    prior_rows = classes.prior_wlh[rec[:, 8].astype(int)]
    assert lifting.nuscenes_results_json(rec, tokens, classes, meta, size=prior_rows)[0] == lifting.nuscenes_results_json(rec, tokens, classes, meta)[0]


# ---------------------------------------------------------------------------------------------------------------- (c) geometry
GEO_K, GEO_D0 = 128, 0.05


def _geometry_chain(**size_kw):
    """bev_fit_host at K = 128, box_place_host, track_velocity_host, box_tracks_host, box_size_host on tests/box_size_cases.geometry_case:
    nothing is filtered on results."""
    from cm3d_amd import bevfit, boxplace, velocity as V
    g = sc.geometry_case()
    M, F = len(g["lists"]), len(g["frame_time"])
    off = np.concatenate([[0], np.cumsum([len(x) for x in g["lists"]])])
    fit_k, rect, status = bevfit.bev_fit_lists(off, np.concatenate(g["lists"], 0), GEO_K, GEO_D0)
    assert not status.any()                                    # every list is fitted
    box = np.zeros((M, 10))
    box[:, 0:2], box[:, 3], box[:, 7], box[:, 8], box[:, 9] = rect[:, :2], 1.0, 0.9, g["class_id"], 3.0
    flags = np.full(M, 3, np.int32)
    ego = np.concatenate([np.tile(g["sensor"], (F, 1)), np.full((F, 1), 1.8)], 1)
    group, thr = np.arange(4, dtype=np.int32), np.full(4, 4.0)
    pl = boxplace.box_place_host(box, flags, g["mask_off"], rect, np.ones(M, np.int32), sc.GEO_PRIOR, group, thr, ego, sc.THIN)
    assert (pl["flags"] == 3).all() and (pl["place_src"] > 0).all()
    v = V.track_velocity_host(pl["box"], pl["flags"], g["mask_off"], g["class_id"], g["frame_next"], g["frame_time"], group, np.full(4, 40.0), sc.MAX_DT)
    tr = T.box_tracks_host(pl["box"], pl["flags"], np.repeat(np.arange(F), 4), v["next_match"], v["prev_match"], g["frame_time"])
    assert v["status"] == 0 and tr["status"] == 0 and (tr["track_len"] == F).all() and np.array_equal(tr["track_id"], g["car"])
    out = bs.box_size_host(pl["box"], pl["flags"], np.repeat(np.arange(F), 4), rect, pl["place_src"], sc.GEO_PRIOR, ego, v["next_match"],
                           v["prev_match"], tr["track_id"], tr["track_pos"], tr["track_len"], g["frame_time"], thin=sc.THIN, max_dt=sc.MAX_DT, **size_kw)
    assert out["status"] == 0
    return g, rect, pl, v, out


def test_geometry_pooled_size_centre_and_velocity_within_the_derived_bounds():
    """Four cars of L x W = 4.9 x 2.1 m (the class prior: 4.5 x 1.9) carried past the sensor over eight keyframes; the anchored corner
    changes in the middle of every track, where two frames show the long face alone (8 of 32 frames, fixed by the case; none left out).

    The bounds are derived, not measured.  eps = pi / 2K + asin(d0 / L) bounds the axis error of the fit.  A true
    L x W footprint seen at an axis error delta <= eps has, along the fitted axis, an extent of at most L cos delta + W sin delta
    <= L + W sin eps; with the long face fully shown at least L cos eps minus the point spacing L / 89 (nothing lies beyond the face's
    end points, which are list points: the spacing is slack), so every observed length lies within
        B_len = max(L (1 - cos eps) + L / 89, W sin eps) + F32
    of L, and likewise every width observed (a frame of two faces) within
        B_wid = max(W (1 - cos eps) + W / 59, L sin eps) + F32
    of W; F32 = 4 * 2^-24 * 1200 covers the float32 rows at global magnitude (two end points, x and y).  One face alone gives
    b <= L sin eps + F32 = 0.11 m < lo * 1.9 m: no width observation, by the rule.  The pooled value is an order statistic, one of the
    observed values, so the bounds hold for it at every q.
    Centre: the sensor-side corner of the rectangle lies within eps (L + W) of the car's (box_place_cases.placed_bound: the angle times
    the longest lever), and the centre hangs (len / 2, wid / 2) from it instead of (L / 2, W / 2):
        B_centre = eps (L + W) + hypot(B_len, B_wid) / 2
    (a frame of one face is centred on the face along the heading, within the lever term, and hangs wid / 2 from it across).
    Velocity: two centres, each within B_centre, over a span of at least dt: within 2 B_centre / dt of the car's true velocity."""
    L, W, K = sc.GEO_L, sc.GEO_W, GEO_K
    eps = np.pi / (2 * K) + np.arcsin(GEO_D0 / L)
    f32 = 4 * 2.0 ** -24 * 1200.0
    b_len = max(L * (1 - np.cos(eps)) + L / (sc.GEO_N_LONG - 1), W * np.sin(eps)) + f32
    b_wid = max(W * (1 - np.cos(eps)) + W / (sc.GEO_N_SHORT - 1), L * np.sin(eps)) + f32
    b_centre = eps * (L + W) + np.hypot(b_len, b_wid) / 2
    assert L * np.sin(eps) + f32 < 0.6 * 1.9
    for q in (0.75, 0.0, 1.0):
        g, rect, pl, v, out = _geometry_chain(q=q)
        assert (out["size_src"] == 3).all() and (out["size_obs"] == [8, 6]).all()        # eight lengths and six widths a track
        e_len, e_wid = np.abs(out["size_wlh"][:, 1] - L), np.abs(out["size_wlh"][:, 0] - W)
        e_c = np.hypot(*(out["box"][:, :2] - g["centre"]).T)
        e_prior = np.hypot(*(pl["box"][:, :2] - g["centre"]).T)
        e_v = np.hypot(*(out["size_vel"] - g["velocity"]).T)
        e_v_prior = np.hypot(*(v["vel"] - g["velocity"]).T)
        # the frames at which the anchored corner changes: a neighbour in the track shows another corner, or the face alone
        pu = (g["sensor"][0] - rect[:, 0]) * rect[:, 4] + (g["sensor"][1] - rect[:, 1]) * rect[:, 5]
        key = np.where(g["two_faces"], np.sign(pu), 0.0).reshape(sc.GEO_FRAMES, -1)
        change = np.zeros_like(key, bool)
        change[1:] |= key[1:] != key[:-1]
        change[:-1] |= key[:-1] != key[1:]
        change = change.reshape(-1)
        print(f"q = {q}: |len - L| <= {e_len.max():.4f} (bound {b_len:.4f}), |wid - W| <= {e_wid.max():.4f} (bound {b_wid:.4f}); centre "
              f"{e_c.max():.4f} m (bound {b_centre:.4f}; prior-sized placement {e_prior.max():.4f} m); velocity at the {int(change.sum())} "
              f"frames of a corner change {e_v[change].max():.4f} m/s, elsewhere {e_v[~change].max():.4f} (bound {2 * b_centre / sc.GEO_DT:.4f}; "
              f"on the prior-sized centres {e_v_prior[change].max():.4f})")
        assert change.sum() >= 16
        assert (e_len <= b_len).all() and (e_wid <= b_wid).all()
        assert (e_c <= b_centre).all()
        assert (e_v <= 2 * b_centre / sc.GEO_DT).all()
        # what the stage is for: with the prior's size the centre jumps where the corner changes, and the jump is in the velocity
        assert e_prior.max() > b_centre and e_v_prior[change].max() > e_v[change].max()
