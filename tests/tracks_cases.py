"""Cases for the box track stage (cm3d_box_tracks, cm3d_amd.tracks.box_tracks_host).  Pure numpy, seeded, no GPU.

A case is the array arguments of tracks.box_tracks_host / ops.box_tracks as a dict (box, flags, mask_frame, next_match, prev_match,
frame_time) plus `name`, `settings` -- the (min_length, score, smooth_window) triples the case is run with -- and, where the answer is
known in closed form, `expect`: settings triple -> dict of the outputs that are pinned.  A status case also carries `status` and
`fixed`: the same case with the offending entries replaced by what the rule reads them as, whose outputs it must share.

  shapes    tracks of length 1, 2, 3 and F; two tracks interleaved in mask order; frames that are not in time order, with a follower at a
            lower batch index; a frame without masks; no mask at all; 257 and 513 masks (grid tails); dropped boxes inside what would
            be a chain
  status    each invalid link alone -- not mutual, to a dropped box, backward in time, equal times, index -2, index M --, a
            mask_frame of F and one of -1
  settings  min_length 1, L and L + 1; the three score modes on scores whose float64 sum depends on the order; W = 1, 2 and F at the
            head, the middle and the tail of a track
  dyadic    five frames 0.5 s apart, boxes on a dyadic grid that move at (2, -1) m/s, one box that shows once: ids, positions, lengths,
            mean scores and the filter are known, and the least-squares slope is (2.0, -1.0) exactly for W = 1, 2, 3
"""
import functools

import numpy as np

BOX_STRIDE = 10
DEFAULT = (1, "own", 0)


def _case(name, times, masks, links, settings=None, expect=None):
    """masks: (frame, x, y, score, flags) per mask, in mask order; links: (i, j) pairs, next_match[i] = j and prev_match[j] = i."""
    M, F = len(masks), len(times)
    box = np.zeros((M, BOX_STRIDE), np.float64)
    flags, frame = np.zeros(M, np.int32), np.zeros(M, np.int32)
    for i, (f, x, y, s, fl) in enumerate(masks):
        box[i, 0], box[i, 1], box[i, 2], box[i, 3], box[i, 7], box[i, 8], box[i, 9] = x, y, 0.5, 1.0, s, 0.0, fl
        flags[i], frame[i] = fl, f
    nm, pm = np.full(M, -1, np.int32), np.full(M, -1, np.int32)
    for i, j in links:
        nm[i], pm[j] = j, i
    if settings is None:
        settings = [DEFAULT, (2, "mean", 1), (3, "max", 2), (1, "mean", F), (F + 1, "own", 0)]
    return dict(name=name, box=box, flags=flags, mask_frame=frame, next_match=nm, prev_match=pm,
                frame_time=np.asarray(times, np.float64), settings=list(settings), expect=expect or {}, status=0, fixed=None)


def args_of(case):
    """The array arguments of box_tracks_host / ops.box_tracks."""
    return [case[k] for k in ("box", "flags", "mask_frame", "next_match", "prev_match", "frame_time")]


def _with(case, name, status, **arrays):
    """`case` with some arrays replaced: a status case whose outputs are those of `case`."""
    return dict(case, name=name, status=status, fixed=case, expect={}, **{k: np.asarray(v, case[k].dtype) for k, v in arrays.items()})


TIMES5 = [0.0, 0.5, 1.0, 1.5, 2.0]


# ---------------------------------------------------------------------------------------------------------------- shapes
def lengths_case():
    """F = 5, masks in frame order.  Track A through every frame (masks 0, 4, 7, 9, 10), B of three (1, 5, 8), C of two (2, 6), D alone
    (3).  Scores differ per member, so mean and max are told apart."""
    masks = [(0, 0.0, 0.0, 0.5, 3), (0, 64.0, 0.0, 0.25, 3), (0, 128.0, 0.0, 0.75, 3), (0, 192.0, 0.0, 0.125, 3),
             (1, 1.0, -0.5, 0.25, 3), (1, 64.0, 1.0, 0.5, 3), (1, 128.0, 2.0, 0.25, 3),
             (2, 2.0, -1.0, 0.75, 3), (2, 64.0, 2.0, 0.75, 3),
             (3, 3.0, -1.5, 0.5, 3),
             (4, 4.0, -2.0, 1.0, 3)]
    links = [(0, 4), (4, 7), (7, 9), (9, 10), (1, 5), (5, 8), (2, 6)]
    tid = [0, 1, 2, 3, 0, 1, 2, 0, 1, 0, 0]
    pos = [0, 0, 0, 0, 1, 1, 1, 2, 2, 3, 4]
    ln = [5, 3, 2, 1, 5, 3, 2, 5, 3, 5, 5]
    mean = [0.6, 0.5, 0.5, 0.125, 0.6, 0.5, 0.5, 0.6, 0.5, 0.6, 0.6]
    common = dict(track_id=tid, track_pos=pos, track_len=ln)
    settings = [DEFAULT, (2, "mean", 1), (3, "max", 2), (4, "own", 5), (5, "mean", 0), (6, "max", 0)]
    fl = lambda n: [3 if L >= n else 1 for L in ln]
    expect = {DEFAULT: dict(common, flags=[3] * 11),
              (2, "mean", 1): dict(common, flags=fl(2), score=mean),
              (3, "max", 2): dict(common, flags=fl(3), score=[1.0, 0.75, 0.75, 0.125, 1.0, 0.75, 0.75, 1.0, 0.75, 1.0, 1.0]),
              (4, "own", 5): dict(common, flags=fl(4)),
              (5, "mean", 0): dict(common, flags=fl(5)),                 # min_length = L of the longest track: it stays
              (6, "max", 0): dict(common, flags=[1] * 11)}               # L + 1: nothing is left
    # track A: centre (k, -k/2) at t = k/2 -- (2, -1) m/s; its statistics in closed form
    expect[DEFAULT]["track_stat_of"] = {0: [3.0, 1.0, 2.0, float(np.sqrt(20.0))], 3: [0.125, 0.125, 0.0, 0.0]}
    return _case("lengths_1_2_3_F", TIMES5, masks, links, settings, expect)


def interleaved_case():
    """Two tracks whose members alternate in mask order: one mask of each per frame."""
    masks, links = [], []
    for k in range(5):
        masks += [(k, 8.0 + k, 16.0, 0.5 + k / 16.0, 3), (k, 200.0, 100.0 - 2.0 * k, 0.25, 3)]
        if k:
            links += [(2 * k - 2, 2 * k), (2 * k - 1, 2 * k + 1)]
    exp = dict(track_id=[0, 1] * 5, track_pos=[k for k in range(5) for _ in (0, 1)], track_len=[5] * 10)
    return _case("two_tracks_interleaved", TIMES5, masks, links, expect={DEFAULT: exp})


ORDER_SCORES = [1.0, 1e16, -1e16, 1.0]          # in track order: ((1 + 1e16) - 1e16) + 1 = 1; in mask order below: 2


def out_of_time_order_case():
    """Frames 0..3 at times 1.5, 0.0, 1.0, 0.5: the track runs frame 1 -> 3 -> 2 -> 0, masks 1 -> 3 -> 2 -> 0, so the head is not the
    lowest index and two followers lie below their predecessors.  The scores' float64 sum depends on the order: 1.0 in track order,
    2.0 in mask order; the mean is 0.25.  A second track (4 -> 5) runs frame 1 -> 2."""
    times = [1.5, 0.0, 1.0, 0.5]
    s = ORDER_SCORES
    masks = [(0, 3.0, -1.5, s[3], 3), (1, 0.0, 0.0, s[0], 3), (2, 2.0, -1.0, s[2], 3), (3, 1.0, -0.5, s[1], 3),
             (1, 50.0, 50.0, 0.5, 3), (2, 51.0, 50.0, 0.25, 3)]
    assert sum(m[3] for m in masks[:4]) == 2.0 and (((0.0 + s[0]) + s[1]) + s[2]) + s[3] == 1.0
    links = [(1, 3), (3, 2), (2, 0), (4, 5)]
    common = dict(track_id=[1, 1, 1, 1, 4, 4], track_pos=[3, 0, 2, 1, 0, 1], track_len=[4, 4, 4, 4, 2, 2])
    expect = {DEFAULT: dict(common, track_stat_of={1: [1.0, 1e16, 1.5, float(np.sqrt(11.25))], 4: [0.75, 0.5, 1.0, 1.0]}),
              (1, "mean", 0): dict(common, score=[0.25] * 4 + [0.375] * 2),
              (1, "max", 0): dict(common, score=[1e16] * 4 + [0.5] * 2),
              (3, "own", 2): dict(common, flags=[3, 3, 3, 3, 1, 1], vel_smooth=[[2.0, -1.0]] * 4 + [[1.0, 0.0]] * 2)}
    return _case("frames_out_of_time_order", times, masks, links, list(expect) + [(2, "mean", 1), (5, "max", 4)], expect)


def empty_frame_case():
    """Frame 2 holds no mask: the tracks of frames 0-1 and 3-4 end and begin there, one link spans it."""
    masks = [(0, 0.0, 0.0, 0.5, 3), (0, 40.0, 0.0, 0.5, 3), (1, 1.0, 0.0, 0.5, 3), (1, 41.0, 0.0, 0.5, 3),
             (3, 3.0, 0.0, 0.5, 3), (3, 90.0, 0.0, 0.5, 3), (4, 4.0, 0.0, 0.5, 3), (4, 91.0, 0.0, 0.5, 3)]
    links = [(0, 2), (1, 3), (2, 4), (4, 6), (5, 7)]
    exp = dict(track_id=[0, 1, 0, 1, 0, 5, 0, 5], track_pos=[0, 0, 1, 1, 2, 0, 3, 1], track_len=[4, 2, 4, 2, 4, 2, 4, 2])
    return _case("frame_without_masks", TIMES5, masks, links, expect={DEFAULT: exp})


def no_masks_case():
    return _case("no_masks", TIMES5, [], [])


def random_case(name, M, F, seed, drop=0.15):
    """M masks over F frames in frame order, frame times shuffled; between consecutive frames in TIME a random part of the kept masks
    is linked one to one, so tracks start and end everywhere.  Centres and scores are arbitrary doubles."""
    rng = np.random.default_rng(seed)
    frame = np.sort(rng.integers(0, F, M))
    times = rng.permutation(F) * 0.5 + rng.integers(0, 4, F) / 16.0
    flags = np.where(rng.random(M) < drop, rng.choice([0, 1, 2], M), 3)
    masks = [(int(frame[i]), float(rng.normal(1000.0, 60.0)), float(rng.normal(2000.0, 60.0)), float(rng.random()), int(flags[i])) for i in range(M)]
    by_time = np.argsort(times)
    links = []
    for a, b in zip(by_time[:-1], by_time[1:]):
        ia, ib = np.flatnonzero((frame == a) & (flags == 3)), np.flatnonzero((frame == b) & (flags == 3))
        k = int(min(len(ia), len(ib)) * 0.8)
        links += list(zip(rng.permutation(ia)[:k].tolist(), rng.permutation(ib)[:k].tolist()))
    return _case(name, times, masks, links)


def dropped_in_chain_case():
    """What would be the chain 0 -> 1 -> 2 -> 3 -> 4 with masks 1 and 3 dropped by the NMS (flags 1): the velocity stage links no dropped
    box, so three tracks of one remain; a second chain beside it is whole."""
    masks = [(k, float(k), 0.0, 0.5, 1 if k in (1, 3) else 3) for k in range(5)] + [(k, 100.0 + k, 7.0, 0.25, 3) for k in range(5)]
    links = [(5 + k, 6 + k) for k in range(4)]
    exp = dict(track_id=[0, -1, 2, -1, 4, 5, 5, 5, 5, 5], track_pos=[0, -1, 0, -1, 0, 0, 1, 2, 3, 4], track_len=[1, 0, 1, 0, 1, 5, 5, 5, 5, 5])
    return _case("dropped_inside_a_chain", TIMES5, masks, links,
                 expect={DEFAULT: exp, (2, "mean", 1): dict(exp, flags=[1, 1, 1, 1, 1, 3, 3, 3, 3, 3])})


# ---------------------------------------------------------------------------------------------------------------- status
def status_cases():
    """Each offence alone, on a scene of two whole tracks (0 -> 2 -> 4 and 1 -> 3 -> 5 through frames 0, 1, 2; frame 3 is empty or
    holds mask 6) plus masks 6 and 7, which the offence links.  `fixed` is the scene as the rule reads it."""
    tracks = [(0, 0.0, 0.0, 0.5, 3), (0, 50.0, 0.0, 0.25, 3), (1, 1.0, 0.0, 0.5, 3), (1, 51.0, 0.0, 0.25, 3), (2, 2.0, 0.0, 0.5, 3),
              (2, 52.0, 0.0, 0.25, 3)]
    whole = [(0, 2), (2, 4), (1, 3), (3, 5)]
    t4 = [0.0, 0.5, 1.0, 1.5]

    def scene(name, f6=0, f7=1, fl6=3, fl7=3, times=t4):
        return _case(name, times, tracks + [(f6, 90.0, 9.0, 0.75, fl6), (f7, 91.0, 9.0, 0.75, fl7)], whole)

    def linked(c, nm=(), pm=()):
        n, p = c["next_match"].copy(), c["prev_match"].copy()
        for i, j in nm:
            n[i] = j
        for i, j in pm:
            p[i] = j
        return dict(next_match=n, prev_match=p)
    base = scene("status_base")
    out = [_with(base, "link_not_mutual", 4, **linked(base, nm=[(6, 7)])),                       # 7 does not point back
           _with(base, "prev_link_not_mutual", 4, **linked(base, pm=[(7, 2)])),                  # 7 claims 2, whose next is 4
           _with(scene("dropped_base", fl7=1), "link_to_a_dropped_box", 4, **linked(base, nm=[(6, 7)], pm=[(7, 6)])),
           # 6 -> 7 mutual, but 6 lies in frame 3 and 7 in frame 0: backward, and with frame 3 at time 0.0 between equal times
           _with(scene("backward_base", f6=3, f7=0), "link_backward_in_time", 4, **linked(base, nm=[(6, 7)], pm=[(7, 6)])),
           _with(scene("equal_base", f6=3, f7=0, times=[0.0, 0.5, 1.0, 0.0]), "link_between_equal_times", 4,
                 **linked(base, nm=[(6, 7)], pm=[(7, 6)])),
           _with(base, "next_match_minus_2", 2, **linked(base, nm=[(6, -2)])),
           _with(base, "next_match_M", 2, **linked(base, nm=[(6, 8)])),
           _with(base, "prev_match_far_outside", 2, **linked(base, pm=[(7, 1 << 30)]))]
    # a marked mask whose frame is F / -1: not kept, status bit 0; `fixed` has it dropped
    for name, bad in (("mask_frame_F", 4), ("mask_frame_minus_1", -1)):
        fixed = scene(name + "_base", fl6=1)
        fr, fl, bx = fixed["mask_frame"].copy(), fixed["flags"].copy(), fixed["box"].copy()
        fr[6], fl[6], bx[6, 9] = bad, 3, 3.0
        out.append(_with(fixed, name, 1, mask_frame=fr, flags=fl, box=bx))
    return out


# ---------------------------------------------------------------------------------------------------------------- dyadic
DYADIC_V = (2.0, -1.0)
DYADIC_K = 6


def dyadic_case():
    """Five frames 0.5 s apart; DYADIC_K boxes per frame on a grid of 64 m, moving at (2, -1) m/s, box j's score (j + 1) / 8 in frame 0
    and half of that afterwards; box 5 is dropped in frame 2, which cuts its track into 2 + 2; one more box shows in frame 3 only."""
    masks, index = [], {}
    for k, t in enumerate(TIMES5):
        for j in range(DYADIC_K):
            index[k, j] = len(masks)
            s = (j + 1) / 8.0 if k == 0 else (j + 1) / 16.0
            masks.append((k, 1024.0 + 64.0 * j + DYADIC_V[0] * t, 2048.0 - 32.0 * j + DYADIC_V[1] * t, s, 1 if (k, j) == (2, 5) else 3))
        if k == 3:
            once = len(masks)
            masks.append((k, 900.0, 1900.0, 0.875, 3))
    links = [(index[k, j], index[k + 1, j]) for k in range(4) for j in range(DYADIC_K) if not (j == 5 and k in (1, 2))]
    M = len(masks)
    tid, pos, ln, mean = np.full(M, -1), np.full(M, -1), np.zeros(M, int), np.zeros(M)
    for j in range(DYADIC_K - 1):
        for k in range(5):
            i = index[k, j]
            tid[i], pos[i], ln[i], mean[i] = index[0, j], k, 5, (j + 1) * (1 / 8.0 + 4 / 16.0) / 5.0
    for k0 in (0, 3):
        for k in (k0, k0 + 1):
            i = index[k, 5]
            tid[i], pos[i], ln[i], mean[i] = index[k0, 5], k - k0, 2, (6 / 8.0 + 6 / 16.0) / 2.0 if k0 == 0 else 6 / 16.0
    tid[once], pos[once], ln[once], mean[once] = once, 0, 1, 0.875
    kept = tid >= 0
    common = dict(track_id=tid, track_pos=pos, track_len=ln, once=once)
    vel = np.where((ln >= 2)[:, None], np.array(DYADIC_V)[None, :], 0.0)
    flags_at = lambda n: np.where(kept, np.where(ln >= n, 3, 1), 1)
    expect = {DEFAULT: dict(common, flags=flags_at(1)),
              (2, "mean", 1): dict(common, flags=flags_at(2), vel_smooth=vel, score=np.where(kept, mean, 0.0)),
              (3, "own", 2): dict(common, flags=flags_at(3), vel_smooth=vel),
              (1, "own", 3): dict(common, flags=flags_at(1), vel_smooth=vel)}
    return _case("dyadic_constant_velocity", TIMES5, masks, links, list(expect) + [(6, "max", 5)], expect)


def window_case():
    """One track of seven boxes that does NOT move uniformly, frames at uneven times: the window sums at the head, in the middle and at
    the tail differ for W = 1, 2 and F, and none is exact -- the order of the six sums decides the last bits."""
    times = [0.0, 0.45, 1.05, 1.5, 2.1, 2.45, 3.05]
    xs = [1013.1, 1014.3, 1014.9, 1016.6, 1017.2, 1019.1, 1019.4]
    ys = [2391.7, 2391.2, 2390.1, 2390.3, 2389.0, 2388.8, 2387.1]
    masks = [(k, xs[k], ys[k], 0.1 * (k + 1), 3) for k in range(7)]
    links = [(k, k + 1) for k in range(6)]
    return _case("uneven_track_windows", times, masks, links, [(1, "own", 1), (1, "own", 2), (1, "own", 7), (7, "mean", 3), (8, "max", 40)])


def check_pinned(case, st, got):
    """The closed-form answers of a case for one settings triple (also used on the device's outputs)."""
    e = case["expect"].get(st)
    if e is None:
        return 0
    for k in ("track_id", "track_pos", "track_len", "flags"):
        if k in e:
            assert np.array_equal(got[k], np.asarray(e[k])), (case["name"], st, k)
    if "score" in e:
        keep = got["track_id"] >= 0
        assert np.array_equal(got["box"][keep, 7], np.asarray(e["score"], np.float64)[keep]), (case["name"], st)
    if "vel_smooth" in e:
        assert np.array_equal(got["vel_smooth"], np.asarray(e["vel_smooth"], np.float64)), (case["name"], st)
    for head, stat in e.get("track_stat_of", {}).items():
        members = got["track_id"] == head
        assert members.any() and (got["track_stat"][members] == np.asarray(stat)).all(), (case["name"], st, head)
    return 1


@functools.lru_cache(maxsize=None)
def all_cases():
    cases = [lengths_case(), interleaved_case(), out_of_time_order_case(), empty_frame_case(), no_masks_case(),
             random_case("grid_tail_257", 257, 8, 5), random_case("grid_tail_513", 513, 16, 6), random_case("three_hundred_masks", 300, 40, 7),
             dropped_in_chain_case(), dyadic_case(), window_case()] + status_cases()
    assert len({c["name"] for c in cases}) == len(cases)
    return cases


def by_name(name):
    return next(c for c in all_cases() if c["name"] == name)
