"""Cases for the box size stage (cm3d_box_size, cm3d_amd.boxsize.box_size_host).  Pure numpy, seeded, no GPU.

A case is the array arguments of boxsize.box_size_host as a dict (KEYS below; ego_xyz None is the Waymo form of the sensor) plus `name`,
`status` -- the pinned status word, the same for every run --, `runs` -- the keyword arguments the case is run with -- and, where the
answer is known in closed form, `expect`.  size_reference is the rule once more as a plain scalar loop per mask (a walk and a rank
count, no sort), written apart from the host statement, which both are held against each other with.

  (a) rule tables   tracks of length 1, 2, 3, 63, 64, 65 and F, interleaved in mask order; equal ratios; a ratio exactly lo, exactly hi and
                    one ulp outside each; n == min_obs - 1 and n == min_obs; q * (n - 1) on an integer and just below one; members
                    with place_src 0 at the head, inside and at the end of a track; two classes in one track; a class of length 0;
                    NaN and infinite record values; class ids below the table, above it and NaN; the Waymo sensor; extents beyond the
                    pooled size; centres near 1 km and 10 km; no masks; a dyadic track whose velocities are exact; a span over max_dt
  (b) hostile       track_id out of range, track_pos >= track_len, a follower of another track, a 2-cycle and a self-loop in
                    next_match, track_len above F (a chain longer than F: the walk is cut), mask_frame out of range
"""
import functools

import numpy as np

BOX_STRIDE = 10
KEYS = ("box", "flags", "mask_frame", "fit_rect", "place_src", "prior_wlh", "ego_xyz", "next_match", "prev_match", "track_id", "track_pos",
        "track_len", "frame_time")
# [w, l, h] per class: dyadic rows (ratios of dyadic extents are exact), a car, a class of length 0
PRIOR = np.array([[2.0, 4.0, 1.5], [1.9, 4.5, 1.7], [2.5, 8.0, 3.0], [0.0, 0.0, 1.0], [0.7, 0.0, 1.8]], np.float64)
THIN, MAX_DT = 0.5, 1.5
Q_JUST_BELOW = float(np.nextafter(0.75, 0.0))         # 0.75 * 4 = 3 exactly; this q gives 2.99..: k = 2
DEFAULT_RUNS = tuple(dict(q=q, smooth_window=W) for q in (0.75, 0.0, 0.5, 1.0) for W in (0, 2))


def args_of(case):
    return [case[k] for k in KEYS]


def place_xy(rect, sx, sy, ln, wd, thin):
    """cm3d_box_place's centre for one rectangle, sensor and size: scalar float64, one rounding per operation."""
    cx, cy, a, b, hc, hs = (np.float64(v) for v in rect)
    sx, sy, ln, wd = np.float64(sx), np.float64(sy), np.float64(ln), np.float64(wd)
    ex, ey = sx - cx, sy - cy
    pu, pv = (ex * hc) + (ey * hs), (ey * hc) - (ex * hs)
    su, sv = (1.0 if pu >= 0.0 else -1.0), (1.0 if pv >= 0.0 else -1.0)
    du = su * ((a - ln) * 0.5) if b >= thin else np.float64(0.0)
    dv = sv * ((b - wd) * 0.5) if a >= thin else np.float64(0.0)
    return ((du * hc) - (dv * hs)) + cx, ((du * hs) + (dv * hc)) + cy


def _class_of(b8, n_classes):
    return int(b8) if (b8 >= 0.0 and b8 < float(n_classes)) else 0


def _scene(name, times, tracks, ego=None, order="frame", prior=PRIOR, runs=DEFAULT_RUNS, status=0, expect=None, waymo=False):
    """tracks: lists of member dicts in track order: frame, cls (the value of box[.][8]), rect (cx, cy, a, b, hc, hs), src (place_src,
    default 1), kept (default True: a mask that is not kept is in no track and splits nothing -- give such masks as tracks of their
    own with kept False).  order "frame": masks sorted by frame, so tracks interleave; "track": track after track.  The entry centre of a
    placed member is cm3d_box_place's with the prior size; of any other, the rectangle's centre."""
    times = np.asarray(times, np.float64)
    F = times.size
    ego = np.column_stack([np.arange(F) * 1.0 + 3.0, np.arange(F) * -0.5 - 7.0, np.zeros(F)]) if ego is None else np.asarray(ego, np.float64)
    rows = [(ti, k, m) for ti, tr in enumerate(tracks) for k, m in enumerate(tr)]
    if order == "frame":
        rows.sort(key=lambda r: (r[2]["frame"], -r[0]))            # within a frame the later track first: heads are not the lowest index
    M = len(rows)
    index = {(ti, k): i for i, (ti, k, _) in enumerate(rows)}
    box, rect = np.zeros((M, BOX_STRIDE), np.float64), np.zeros((M, 6), np.float64)
    flags, frame, src = np.zeros(M, np.int32), np.zeros(M, np.int32), np.zeros(M, np.int32)
    nm, pm = np.full(M, -1, np.int32), np.full(M, -1, np.int32)
    tid, pos, ln = np.full(M, -1, np.int32), np.full(M, -1, np.int32), np.zeros(M, np.int32)
    for i, (ti, k, m) in enumerate(rows):
        kept = m.get("kept", True)
        frame[i], src[i], rect[i] = m["frame"], m.get("src", 1), m["rect"]
        flags[i] = 3 if kept else 1
        c = _class_of(np.float64(m["cls"]), prior.shape[0])
        sx, sy = (0.0, 0.0) if waymo else ego[m["frame"], :2]
        ok = src[i] != 0 and np.isfinite(rect[i]).all() and np.isfinite(sx) and np.isfinite(sy)
        x, y = place_xy(rect[i], sx, sy, prior[c, 1], prior[c, 0], THIN) if ok else (rect[i, 0], rect[i, 1])
        box[i, :4] = x, y, 0.5, prior[c, 1]
        box[i, 7], box[i, 8], box[i, 9] = 0.5, m["cls"], flags[i]
        if kept:
            L = len(tracks[ti])
            tid[i], pos[i], ln[i] = index[ti, 0], k, L
            if k + 1 < L:
                nm[i] = index[ti, k + 1]
            if k:
                pm[i] = index[ti, k - 1]
    return dict(name=name, box=box, flags=flags, mask_frame=frame, fit_rect=rect, place_src=src, prior_wlh=prior.copy(),
                ego_xyz=None if waymo else ego, next_match=nm, prev_match=pm, track_id=tid, track_pos=pos, track_len=ln, frame_time=times,
                runs=list(runs), status=status, expect=expect or {}, index=index)


def _rect(rng, cx, cy, cls, rl=None, rw=None, prior=PRIOR):
    """A rectangle at (cx, cy) with a random heading whose extents are rl, rw times the class's prior (random in 0.3 .. 1.8 when None)."""
    c = _class_of(np.float64(cls), prior.shape[0])
    th = rng.uniform(-np.pi, np.pi)
    rl = rng.uniform(0.3, 1.8) if rl is None else rl
    rw = rng.uniform(0.3, 1.8) if rw is None else rw
    return [cx, cy, rl * prior[c, 1], rw * prior[c, 0], np.cos(th), np.sin(th)]


def _track(rng, frames, x0, y0, cls=1, src=None, **kw):
    out = []
    for k, f in enumerate(frames):
        out.append(dict(frame=int(f), cls=cls, rect=_rect(rng, x0 + 1.5 * k, y0 - 0.75 * k, cls, **kw),
                        src=int(rng.integers(0, 4)) if src is None else src))
    return out


# ---------------------------------------------------------------------------------------------------------------- (a) tables
def lengths_case(F=70, seed=1):
    rng = np.random.default_rng(seed)
    times = np.arange(F) * 0.5
    tracks = []
    for n, L in enumerate((1, 2, 3, 63, 64, 65, F, 5, 1)):
        start = int(rng.integers(0, F - L + 1))
        tracks.append(_track(rng, range(start, start + L), 1000.0 + 40.0 * n, 2000.0, cls=1 + n % 2))
    return _scene("lengths_1_2_3_63_64_65_F_interleaved", times, tracks)


def ties_case():
    """One track of six members with the ratios (1, 1.25, 1, 1.25, 1, 1.25) in both dimensions, class 0 (4 x 2 m: exact quotients):
    the order is (value, position); q = 0.5 -> k = 2, the third 1.0; q = 0.75 -> k = 3, the first 1.25; lengths 4.0 and 5.0."""
    rng = np.random.default_rng(2)
    tr = [dict(frame=k, cls=0, rect=_rect(rng, 500.0 + k, 600.0, 0, rl=r, rw=r)) for k, r in enumerate((1.0, 1.25, 1.0, 1.25, 1.0, 1.25))]
    expect = {0.75: (1.25, 1.25), 0.0: (1.0, 1.0), 0.5: (1.0, 1.0), 1.0: (1.25, 1.25)}
    return _scene("equal_ratios_position_decides", np.arange(6) * 0.5, [tr], expect=dict(ratio_by_q=expect))


def thresholds_case(lo=0.6, hi=1.5):
    """Class 0 (length 4, width 2: a = r * 4 divides back to r exactly).  Four tracks of two members each; the length ratio of both
    members is lo, hi, one ulp below lo, one ulp above hi; the width is always observed at 1.25.  n = 2, 2, 0, 0 for the length."""
    rng = np.random.default_rng(3)
    tracks = []
    vals = (lo, hi, float(np.nextafter(lo, 0.0)), float(np.nextafter(hi, 9.0)))
    for n, r in enumerate(vals):
        tr = []
        for k in range(2):
            rc = _rect(rng, 100.0 + 30.0 * n + k, 50.0, 0, rl=1.0, rw=1.25)
            rc[2] = r * 4.0
            assert np.float64(rc[2]) / np.float64(4.0) == r
            tr.append(dict(frame=k, cls=0, rect=rc))
        tracks.append(tr)
    return _scene("ratio_on_and_one_ulp_off_lo_hi", [0.0, 0.5], tracks, order="track", expect=dict(obs_len=[2, 2, 2, 2, 0, 0, 0, 0], obs_wid=[2] * 8))


def min_obs_case():
    """Tracks of three members with 1, 2 and 3 observed lengths (the others have ratio 0.3): at min_obs = 2 the first is not pooled;
    run also at min_obs = 3, where only the third is.  One track of five observations 1.0, 1.1, 1.2, 1.3, 1.4 for q * (n - 1): 0.75 * 4
    is 3 exactly (1.3), the double below 0.75 gives k = 2 (1.2)."""
    rng = np.random.default_rng(4)
    tracks = []
    for n in (1, 2, 3):
        tracks.append([dict(frame=k, cls=1, rect=_rect(rng, 10.0 * n + k, 5.0, 1, rl=1.1 + 0.05 * k if k < n else 0.3, rw=1.0 + 0.1 * k))
                       for k in range(3)])
    tracks.append([dict(frame=k, cls=0, rect=_rect(rng, 90.0 + k, 5.0, 0, rl=r, rw=r)) for k, r in enumerate((1.25, 1.0, 1.375, 1.125, 1.5))])
    runs = list(DEFAULT_RUNS) + [dict(q=0.75, min_obs=3), dict(q=Q_JUST_BELOW, smooth_window=1), dict(q=0.5, min_obs=1)]
    return _scene("n_at_min_obs_and_q_on_an_integer", np.arange(5) * 0.5, tracks, runs=runs,
                  expect=dict(five=dict(track=3, by_q={0.75: 1.375, Q_JUST_BELOW: 1.25, 0.0: 1.0, 1.0: 1.5, 0.5: 1.25})))


def place_src_zero_case():
    """Members that kept the lane's yaw (place_src 0) at the head, inside and at the end of a track of five: they observe nothing
    and receive nothing, but carry the links."""
    rng = np.random.default_rng(5)
    tracks = []
    for n, zero in enumerate(((0,), (2,), (4,), (0, 1, 2, 3, 4), (1, 3))):
        tracks.append([dict(frame=k, cls=1, rect=_rect(rng, 300.0 + 25.0 * n + k, 80.0 - k, 1, rl=1.05 + 0.05 * k, rw=0.91 + 0.05 * k),
                            src=0 if k in zero else 1 + k % 3) for k in range(5)])
    return _scene("place_src_0_head_inside_end", np.arange(5) * 0.5, tracks)


def classes_case():
    """Two classes with different priors in one track; a class whose length and width are 0, one whose length alone is; class ids
    -1, n_classes, 1e9, NaN (read as class 0) and fractional ids (truncated)."""
    rng = np.random.default_rng(6)
    tracks = [[dict(frame=k, cls=(1, 2)[k % 2], rect=_rect(rng, 40.0 + k, 9.0, (1, 2)[k % 2], rl=1.0 + 0.1 * k, rw=1.2 - 0.05 * k)) for k in range(5)],
              [dict(frame=k, cls=3, rect=[70.0 + k, 9.0, 3.0, 1.0, 1.0, 0.0]) for k in range(3)],
              [dict(frame=k, cls=4, rect=[90.0 + k, 9.0, 3.0, 0.7 * (1.0 + 0.1 * k), 0.0, 1.0]) for k in range(3)]]
    for n, cid in enumerate((-1.0, float(PRIOR.shape[0]), 1e9, float("nan"), 1.75, -0.5)):
        tracks.append([dict(frame=k, cls=cid, rect=_rect(rng, 120.0 + 20.0 * n + k, 9.0, cid, rl=1.1 + 0.1 * k, rw=1.0 + 0.1 * k)) for k in range(3)])
    return _scene("classes_mixed_zero_prior_bad_ids", np.arange(5) * 0.5, tracks)


def bad_records_case():
    """NaN and infinite values in fit_rect, one field at a time, inside tracks of three whose other members observe; a NaN and an
    infinite sensor in two frames.  Such a member is sized but its centre stays; a NaN extent is no observation."""
    rng = np.random.default_rng(7)
    tracks = []
    for n, (col, val) in enumerate([(c, v) for c in range(6) for v in (float("nan"), float("inf"), float("-inf"))]):
        tr = [dict(frame=k, cls=1, rect=_rect(rng, 1000.0 + 30.0 * n + k, 400.0, 1, rl=1.0 + 0.1 * k, rw=0.8 + 0.1 * k)) for k in range(3)]
        tr[1]["rect"][col] = val
        tracks.append(tr)
    tracks.append([dict(frame=k, cls=1, rect=_rect(rng, 10.0 + k, 400.0, 1, rl=1.2, rw=1.1)) for k in range(3, 6)])
    ego = np.column_stack([np.arange(6.0), -np.arange(6.0), np.zeros(6)])
    ego[4, 0], ego[5, 1] = float("nan"), float("inf")
    return _scene("nan_and_inf_records_and_sensor", np.arange(6) * 0.5, tracks, ego=ego)


def waymo_case():
    rng = np.random.default_rng(8)
    tracks = [_track(rng, range(s, s + L), 20.0 * n - 30.0, 15.0 - 9.0 * n, cls=1, src=1) for n, (s, L) in enumerate(((0, 6), (1, 4), (2, 2), (0, 3)))]
    return _scene("waymo_sensor_at_the_origin", np.arange(6) * 0.1, tracks, waymo=True)


def far_case():
    """Centres near 1 km and 10 km from the sensor, extents beyond the pooled size (q = 0 pools the least: a > len and b > wid for the
    other members)."""
    rng = np.random.default_rng(9)
    tracks = [_track(rng, range(6), 1000.0, -1000.0, cls=1, src=1, rl=None, rw=None), _track(rng, range(6), -10000.0, 9999.0, cls=2, src=1),
              [dict(frame=k, cls=1, rect=_rect(rng, 7000.0 + k, 7000.0, 1, rl=0.72 + 0.15 * k, rw=0.71 + 0.15 * k)) for k in range(6)]]
    return _scene("centres_near_1_km_and_10_km", np.arange(6) * 0.5, tracks, ego=np.zeros((6, 3)))


def no_masks_case():
    return _scene("no_masks", np.arange(4) * 0.5, [])


DYADIC_V = (2.0, -1.0)


def dyadic_case():
    """Five frames 0.5 s apart, axis-aligned rectangles of class 0 whose extents are 5.0 x 2.5 (ratios 1.25 exactly) in every frame:
    the pooled size is 5.0 x 2.5 at every q, (a - len) and (b - wid) are 0, the sized centre is the rectangle's, and that moves on a
    dyadic grid at (2, -1) m/s: both velocity forms are exact.  The prior-sized entry centres are half a metre off.  A second
    track has a gap of 2.0 s > max_dt in its middle: across it no velocity for W = 0 (forward / backward on the sides)."""
    tr = [dict(frame=k, cls=0, rect=[1024.0 + DYADIC_V[0] * 0.5 * k, 2048.0 + DYADIC_V[1] * 0.5 * k, 5.0, 2.5, 1.0, 0.0]) for k in range(5)]
    gap = [dict(frame=f, cls=0, rect=[64.0 + 2.0 * t, 32.0, 5.0, 2.5, 0.0, 1.0]) for f, t in ((5, 10.0), (6, 10.5), (7, 12.5), (8, 13.0))]
    once = [dict(frame=2, cls=0, rect=[0.0, 0.0, 5.0, 2.5, 1.0, 0.0])]
    times = [0.0, 0.5, 1.0, 1.5, 2.0, 10.0, 10.5, 12.5, 13.0]
    return _scene("dyadic_exact_velocity_and_a_span_over_max_dt", times, [tr, gap, once], order="track",
                  expect=dict(vel={0: [DYADIC_V] * 5 + [(2.0, 0.0)] * 4 + [(0.0, 0.0)], 2: [DYADIC_V] * 5 + [(2.0, 0.0)] * 4 + [(0.0, 0.0)]},
                              wlh=[2.5, 5.0, 1.5]))


def random_case(name, n_tracks, F, seed, drop=0.1):
    """A few thousand masks: tracks of random lengths and starts, a part of the masks not kept (in no track)."""
    rng = np.random.default_rng(seed)
    tracks = []
    for n in range(n_tracks):
        L = int(rng.integers(1, F + 1))
        s = int(rng.integers(0, F - L + 1))
        tracks.append(_track(rng, range(s, s + L), rng.normal(0.0, 500.0), rng.normal(0.0, 500.0), cls=int(rng.integers(0, 3))))
        if rng.random() < drop:
            tracks.append([dict(frame=int(rng.integers(0, F)), cls=1, rect=_rect(rng, 0.0, 0.0, 1), kept=False)])
    return _scene(name, np.arange(F) * 0.5 + rng.integers(0, 4, F) / 16.0, tracks, runs=[dict(), dict(q=0.0, smooth_window=3), dict(q=1.0, smooth_window=1)])


def chain_case(F=8, seed=31):
    """A scene in frame order for the whole chain velocity -> tracks -> size: tracks 100 m apart that move 1.5 m a keyframe (the
    gate is 20 m: the association has one candidate), starting and ending in different frames; extents never equal to the prior.
    Beside the case's arrays: mask_off, class_id, frame_next, track_group, max_speed for cm3d_box_velocity."""
    rng = np.random.default_rng(seed)
    tracks = []
    for n in range(12):
        L = int(rng.integers(1, F + 1))
        s = int(rng.integers(0, F - L + 1))
        tracks.append(_track(rng, range(s, s + L), 100.0 * n, 50.0, cls=1 + n % 2, src=None if n % 3 else 1, rl=None, rw=None))
    c = _scene("chain_in_frame_order", np.arange(F) * 0.5, tracks, runs=[dict()])
    c["mask_off"] = np.searchsorted(c["mask_frame"], np.arange(F + 1)).astype(np.int32)
    c["class_id"] = c["box"][:, 8].astype(np.int32)
    c["frame_next"] = np.array(list(range(1, F)) + [-1], np.int32)
    c["track_group"], c["max_speed"] = np.zeros(PRIOR.shape[0], np.int32), np.array([40.0])
    return c


# ---------------------------------------------------------------------------------------------------------------- (b) hostile
def _hostile_base():
    rng = np.random.default_rng(11)
    tracks = [_track(rng, range(0, 5), 0.0, 0.0, src=1), _track(rng, range(1, 5), 50.0, 0.0, src=1), _track(rng, range(0, 3), 100.0, 0.0, src=1)]
    return _scene("hostile_base", np.arange(5) * 0.5, tracks, order="track")      # masks 0..4, 5..8, 9..11


def _with(base, name, status, **arrays):
    c = dict(base, name=name, status=status, expect={})
    for k, edits in arrays.items():
        a = base[k].copy()
        for i, v in edits:
            a[i] = v
        c[k] = a
    return c


def hostile_cases():
    b = _hostile_base()
    M = len(b["flags"])
    out = [_with(b, "track_id_M", 1, track_id=[(2, M)]),                      # 2 is no member: 1's and 3's links are none, 3 and 4 are not reached
           _with(b, "track_id_negative", 1, track_id=[(6, -7)]),
           _with(b, "track_id_far_outside", 1, track_id=[(0, 1 << 30)]),        # the head itself: its track has no head
           _with(b, "track_pos_at_track_len", 1, track_pos=[(7, 4)]),
           _with(b, "track_pos_negative", 1, track_pos=[(9, -1)]),
           _with(b, "follower_of_another_track", 1, next_match=[(1, 7)]),      # 2.. are not reached from the head
           _with(b, "predecessor_of_another_track", 1, prev_match=[(6, 0)]),   # the followers stand: only the velocity's backward link goes
           _with(b, "two_cycle_in_next_match", 1, next_match=[(1, 2), (2, 1)]),
           _with(b, "self_loop_in_next_match", 1, next_match=[(3, 3)]),
           _with(b, "next_match_outside", 1, next_match=[(4, M), (8, -2)]),
           _with(b, "mask_frame_F", 1, mask_frame=[(10, 5)]),
           _with(b, "mask_frame_negative", 1, mask_frame=[(5, -1)]),
           _with(b, "track_len_0_in_a_chain", 1, track_len=[(3, 0)])]
    # track_len above F: a chain of F + 3 members, two per frame and more; the walk is cut at F steps, the last three are not reached
    rng = np.random.default_rng(12)
    F = 6
    chain = [dict(frame=k % F, cls=1, rect=_rect(rng, 10.0 + k, 3.0, 1, rl=1.0 + 0.05 * k, rw=1.0)) for k in range(F + 3)]
    out.append(_scene("track_len_above_F_walk_cut", np.arange(F) * 0.5, [chain, _track(rng, range(3), 80.0, 0.0, src=1)], order="track", status=3))
    # every mask claims a track_len far above F while the chains are short: no walk is cut; the window of W = 2 never exceeds F
    big = dict(b, name="track_len_huge_chains_short", status=0, expect={})
    big["track_len"] = np.where(b["track_len"] > 0, (1 << 31) - 1, 0).astype(np.int32)
    out.append(big)
    return out


# ---------------------------------------------------------------------------------------------------------------- the scalar loop
def size_reference(case, thin=THIN, max_dt=MAX_DT, smooth_window=0, q=0.75, min_obs=2, lo=0.6, hi=1.5):
    """The rule of include/cm3d_hip.h as one plain loop per mask, float64 scalars, a walk and a rank count per member."""
    f8 = np.float64
    box = np.array(case["box"], np.float64)
    M, F = box.shape[0], len(case["frame_time"])
    prior, rect, ego = case["prior_wlh"], case["fit_rect"], case["ego_xyz"]
    C = prior.shape[0]
    frm, src, nmv, pmv = case["mask_frame"], case["place_src"], case["next_match"], case["prev_match"]
    tid, pos, ln = case["track_id"], case["track_pos"], case["track_len"]
    q, lo, hi, thin, max_dt = f8(q), f8(lo), f8(hi), f8(thin), f8(max_dt)
    status = 0

    def member(i):
        return bool(ln[i] > 0 and 0 <= tid[i] < M and 0 <= pos[i] < ln[i] and 0 <= frm[i] < F)

    def link(i, j, step):
        nonlocal status
        j = int(j)
        if 0 <= j < M and member(j) and tid[j] == tid[i] and int(pos[j]) == int(pos[i]) + step:
            return j
        if j != -1:
            status |= 1
        return -1
    is_mem = [member(i) for i in range(M)]
    vnext = [link(i, nmv[i], 1) if is_mem[i] else -1 for i in range(M)]
    vprev = [link(i, pmv[i], -1) if is_mem[i] else -1 for i in range(M)]
    time = [f8(case["frame_time"][frm[i]]) if is_mem[i] else f8(0.0) for i in range(M)]
    cls = [_class_of(box[i, 8], C) for i in range(M)]
    obs = [[None, None] for _ in range(M)]
    with np.errstate(all="ignore"):
        for i in range(M):
            if is_mem[i] and src[i] != 0:
                for d, (ext, p0) in enumerate(((rect[i, 2], prior[cls[i], 1]), (rect[i, 3], prior[cls[i], 0]))):
                    if p0 > 0.0:
                        r = f8(ext) / f8(p0)
                        if lo <= r and r <= hi:
                            obs[i][d] = r
        size_wlh = np.array([prior[cls[i]] for i in range(M)], np.float64).reshape(M, 3)
        size_src, size_ratio, size_obs = np.zeros(M, np.int32), np.zeros((M, 2)), np.zeros((M, 2), np.int32)
        size_placed, size_vel = box[:, :2].copy(), np.zeros((M, 2))
        track_ratio = {}                                       # head -> [r_len, r_wid]
        on_track = [False] * M
        for i in range(M):
            if not is_mem[i]:
                continue
            h = int(tid[i])
            if not (is_mem[h] and tid[h] == h and pos[h] == 0):
                status |= 1
                continue
            n, rank, met, m, steps = [0, 0], [0, 0], False, h, 0
            while m >= 0 and steps < F:
                if m == i:
                    met = True
                else:
                    for d in (0, 1):
                        v = obs[m][d]
                        if v is not None:
                            n[d] += 1
                            if obs[i][d] is not None and (v < obs[i][d] if met else v <= obs[i][d]):
                                rank[d] += 1
                m, steps = vnext[m], steps + 1
            if m >= 0:
                status |= 2
            if not met:
                status |= 1
                continue
            on_track[i] = True
            for d in (0, 1):
                if obs[i][d] is not None:
                    n[d] += 1
                    if n[d] >= min_obs and rank[d] == int(q * f8(n[d] - 1)):
                        track_ratio.setdefault(h, [f8(1.0), f8(1.0)])[d] = obs[i][d]
            size_obs[i] = n
        for i in range(M):
            if not is_mem[i]:
                continue
            r = track_ratio.get(int(tid[i]), [f8(1.0), f8(1.0)]) if on_track[i] else [f8(1.0), f8(1.0)]
            size_ratio[i] = r
            if src[i] == 0:
                continue
            length, width = r[0] * prior[cls[i], 1], r[1] * prior[cls[i], 0]
            size_wlh[i, 0], size_wlh[i, 1] = width, length
            size_src[i] = (1 if size_obs[i, 0] >= min_obs else 0) | (2 if size_obs[i, 1] >= min_obs else 0)
            sx, sy = (f8(0.0), f8(0.0)) if ego is None else ego[frm[i], :2]
            if np.isfinite(rect[i]).all() and np.isfinite(sx) and np.isfinite(sy):
                box[i, 0], box[i, 1] = place_xy(rect[i], sx, sy, length, width, thin)
        W = int(smooth_window)
        for i in range(M):
            if not is_mem[i]:
                continue
            t = time[i]
            if W == 0:
                a, b = vnext[i], vprev[i]
                if a >= 0 and b >= 0 and time[a] - time[b] <= max_dt:
                    size_vel[i] = (box[a, 0] - box[b, 0]) / (time[a] - time[b]), (box[a, 1] - box[b, 1]) / (time[a] - time[b])
                elif a >= 0 and time[a] - t <= max_dt:
                    size_vel[i] = (box[a, 0] - box[i, 0]) / (time[a] - t), (box[a, 1] - box[i, 1]) / (time[a] - t)
                elif b >= 0 and t - time[b] <= max_dt:
                    size_vel[i] = (box[i, 0] - box[b, 0]) / (t - time[b]), (box[i, 1] - box[b, 1]) / (t - time[b])
                continue
            Wc = min(W, F)
            back, ahead = min(int(pos[i]), Wc), min(int(ln[i]) - 1 - int(pos[i]), Wc)
            want = back + 1 + ahead
            if want > F:
                want, status = F, status | 2
            m = i
            for _ in range(back):
                if vprev[m] < 0:
                    break
                m = vprev[m]
            n = 0
            St = Stt = Sx = Sy = Stx = Sty = f8(0.0)
            while n < want and m >= 0:
                tj, xj, yj = time[m] - t, box[m, 0] - box[i, 0], box[m, 1] - box[i, 1]
                St, Stt, Sx, Sy, Stx, Sty = St + tj, Stt + (tj * tj), Sx + xj, Sy + yj, Stx + (tj * xj), Sty + (tj * yj)
                n, m = n + 1, vnext[m]
            if n >= 2:
                dn = f8(n)
                den = (dn * Stt) - (St * St)
                if den > 0.0:
                    size_vel[i] = ((dn * Stx) - (St * Sx)) / den, ((dn * Sty) - (St * Sy)) / den
    return dict(box=box, flags=np.array(case["flags"], np.int32), size_wlh=size_wlh, size_src=size_src, size_ratio=size_ratio, size_obs=size_obs,
                size_placed=size_placed, size_vel=size_vel, status=status)


INT_OUT, F64_OUT = ("size_src", "size_obs", "flags"), ("size_wlh", "size_ratio", "size_placed", "size_vel", "box")


def _bits(a):
    """The array's bit patterns with every NaN made the same one: IEEE 754 leaves the sign and payload of a NaN that an operation
    forms (inf - inf through an infinite centre) to the implementation, and the host's and the device's differ."""
    a = np.ascontiguousarray(a, np.float64).copy()
    a[np.isnan(a)] = np.nan
    return a.view(np.uint64)


def assert_same(got, exp, what):
    """Every output to the bit; a NaN stands where the other side has a NaN."""
    for k in INT_OUT:
        assert np.array_equal(np.asarray(got[k]).reshape(-1), np.asarray(exp[k]).reshape(-1)), (what, k)
    for k in F64_OUT:
        g, e = _bits(got[k]), _bits(exp[k])
        assert g.shape == e.shape and np.array_equal(g, e), (what, k, np.flatnonzero(g.reshape(-1) != e.reshape(-1))[:8])
    assert got["status"] == exp["status"], (what, got["status"], exp["status"])


@functools.lru_cache(maxsize=None)
def table_cases():
    cases = [lengths_case(), ties_case(), thresholds_case(), min_obs_case(), place_src_zero_case(), classes_case(), bad_records_case(),
             waymo_case(), far_case(), no_masks_case(), dyadic_case(), random_case("three_thousand_masks", 180, 32, 21)]
    return cases


@functools.lru_cache(maxsize=None)
def all_cases():
    cases = table_cases() + hostile_cases()
    assert len({c["name"] for c in cases}) == len(cases)
    return cases


def by_name(name):
    return next(c for c in all_cases() if c["name"] == name)


def identity_cases():
    """Tables whose extents never equal the prior exactly (random ratios), all well-formed: with lo = hi = 1 nothing is observed."""
    out = [c for c in table_cases() if c["name"] in ("lengths_1_2_3_63_64_65_F_interleaved", "place_src_0_head_inside_end", "waymo_sensor_at_the_origin",
                                                     "centres_near_1_km_and_10_km", "three_thousand_masks")]
    for c in out:
        c0 = c["prior_wlh"][[_class_of(v, c["prior_wlh"].shape[0]) for v in c["box"][:, 8]]]
        assert not (c["fit_rect"][:, 2] == c0[:, 1]).any() and not (c["fit_rect"][:, 3] == c0[:, 0]).any()
    return out


# ---------------------------------------------------------------------------------------------------------------- (c) geometry
# Cars carried past a fixed sensor: box_place_cases' visible-face construction (the long face that looks at the sensor, and the short
# one with it while the sensor stands at least GEO_MARGIN outside its slab; 90 and 60 points; float32 rows in a shuffled order), for a
# car of GEO_L x GEO_W -- not the class prior's 4.5 x 1.9 -- whose centre moves along its heading from keyframe to keyframe.
GEO_L, GEO_W = 4.9, 2.1
GEO_PRIOR = np.array([[1.9, 4.5, 1.6]] * 4, np.float64)          # four classes of one prior: a class, and an association group, per car
GEO_SENSOR = np.array([600.0, 1200.0])
GEO_MARGIN = 0.5                                                  # box_place_cases.MARGIN
GEO_FRAMES, GEO_DT = 8, 0.5
GEO_N_LONG, GEO_N_SHORT = 90, 60
# (heading, lateral offset of the path from the sensor, speed along the heading, where along the heading the car is at the middle frame)
GEO_CARS = ((0.3, 6.0, 6.0, 0.4), (2.0, -9.0, 8.0, -0.7), (-1.2, 7.5, 5.0, 0.2), (-2.7, -12.0, 7.0, 1.1))
GEO_EXCLUDED = 0                                                  # no frame is left out: inside the margin of the short face the long one is shown alone
GEO_ONE_FACE = 8                                                  # frames (of 32) that show the long face alone: fixed by the geometry above


def geometry_case():
    """dict: lists (per mask, (n, 4) float32), mask_off, class_id, centre (M, 2) true centres, velocity (M, 2), sensor, frame_time,
    frame_next, two_faces (M,) bool, car (M,) -- masks in frame order, car j the j-th mask of every frame."""
    lists, centre, vel, two, car = [], [], [], [], []
    t_mid = 0.5 * (GEO_FRAMES - 1) * GEO_DT
    for f in range(GEO_FRAMES):
        for j, (yaw, lateral, speed, along) in enumerate(GEO_CARS):
            c, s = np.cos(yaw), np.sin(yaw)
            ctr = GEO_SENSOR + lateral * np.array([-s, c]) + (along + speed * (f * GEO_DT - t_mid)) * np.array([c, s])
            e = GEO_SENSOR - ctr
            pu, pv = e[0] * c + e[1] * s, e[1] * c - e[0] * s
            assert abs(pv) >= GEO_W / 2 + GEO_MARGIN                 # the long face always looks at the sensor from outside its slab
            both = abs(pu) >= GEO_L / 2 + GEO_MARGIN
            u = np.linspace(-GEO_L / 2, GEO_L / 2, GEO_N_LONG)
            v = np.full(GEO_N_LONG, np.sign(pv) * GEO_W / 2)
            if both:
                u = np.concatenate([u, np.full(GEO_N_SHORT, np.sign(pu) * GEO_L / 2)])
                v = np.concatenate([v, np.linspace(-GEO_W / 2, GEO_W / 2, GEO_N_SHORT)])
            xy = np.stack([ctr[0] + u * c - v * s, ctr[1] + u * s + v * c], 1)
            xy = xy[np.random.default_rng(1000 * f + j).permutation(len(xy))]
            xyz = np.zeros((len(xy), 4), np.float32)
            xyz[:, :2], xyz[:, 2] = xy, 1.5
            lists.append(xyz); centre.append(ctr); vel.append(speed * np.array([c, s])); two.append(both); car.append(j)
    n = len(GEO_CARS)
    two = np.array(two)
    assert int((~two).sum()) == GEO_ONE_FACE
    return dict(lists=lists, mask_off=np.arange(0, n * GEO_FRAMES + 1, n, dtype=np.int32), class_id=np.array(car, np.int32), centre=np.array(centre),
                velocity=np.array(vel), sensor=GEO_SENSOR, frame_time=np.arange(GEO_FRAMES) * GEO_DT,
                frame_next=np.array(list(range(1, GEO_FRAMES)) + [-1], np.int32), two_faces=two, car=np.array(car))
