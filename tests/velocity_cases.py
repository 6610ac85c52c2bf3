"""Cases for the box velocity stage (cm3d_box_velocity, cm3d_amd.velocity.track_velocity_host).  Pure numpy, seeded, no GPU.

A case is the argument set of velocity.track_velocity_host / ops.box_velocity as a dict (box, flags, mask_off, class_id, frame_next,
frame_time, track_group, max_speed, max_dt) plus `name` and, where the answer is known in closed form, `expect` (a dict of the outputs
that are pinned).  Five families, and the clamp pairs (clamp_cases) beside them:

  links     the last frame of a scene; two scenes in one batch; dt exactly max_dt and one ulp above; dt <= 0; a middle frame without a
            kept box; a frame_next out of range; a chain of three links
  capacity  a frame of 1025 masks on either side of a link
  weights   group mismatch; a box that is not kept on either side; d2 == gate^2 exactly and one ulp outside; identical centres;
            global-magnitude coordinates
  assign    a pair of mutual nearest neighbours the optimum separates; a "domino" chain (tests/assign_cases.py); an all-equal matrix;
            the mask counts at the solver's instance borders, (1024, 300), the LDS / L2 seam at 8192 pairs
  velocity  a three-frame scene of constant-velocity boxes on a dyadic grid with dt = 0.5: central, forward and backward differences
            are exact in float64; the same scene with max_dt below the central span
"""
import functools

import numpy as np

BOX_STRIDE = 10
TRACK_GROUP = np.array([0, 1, 1, 2], np.int32)            # four classes, classes 1 and 2 share a group
MAX_SPEED = np.array([40.0, 5.0, 1.0], np.float64)         # per group
COUNTS = [(0, 5), (5, 0), (1, 1), (63, 64), (64, 64), (65, 64), (64, 65), (129, 100), (100, 129), (257, 200)]
SEAM_COUNTS = [(64, 128), (64, 129)]                       # 8192 pairs: the last link in LDS, 8256: the first from L2


def _case(name, frames, frame_next, frame_time, max_dt=1.5, track_group=TRACK_GROUP, max_speed=MAX_SPEED, expect=None):
    """frames: one (xy (k, 2), class_id (k,), flags (k,)) triple per frame (scalars broadcast)."""
    xs, cs, fs, off = [], [], [], [0]
    for xy, cls, flg in frames:
        xy = np.asarray(xy, np.float64).reshape(-1, 2)
        k = xy.shape[0]
        xs.append(xy)
        cs.append(np.broadcast_to(np.asarray(cls, np.int32), (k,)))
        fs.append(np.broadcast_to(np.asarray(flg, np.int32), (k,)))
        off.append(off[-1] + k)
    M = off[-1]
    box = np.zeros((M, BOX_STRIDE), np.float64)
    box[:, :2] = np.concatenate(xs) if M else np.zeros((0, 2))
    box[:, 3] = 1.0
    cls = np.concatenate(cs).astype(np.int32) if M else np.zeros(0, np.int32)
    flags = np.concatenate(fs).astype(np.int32) if M else np.zeros(0, np.int32)
    box[:, 8], box[:, 9], box[:, 7] = cls, flags, 0.5
    return dict(name=name, box=box, flags=flags, mask_off=np.array(off, np.int32), class_id=cls,
                frame_next=np.asarray(frame_next, np.int32), frame_time=np.asarray(frame_time, np.float64),
                track_group=np.asarray(track_group, np.int32), max_speed=np.asarray(max_speed, np.float64), max_dt=float(max_dt),
                expect=expect or {})


def args_of(case):
    """The positional arguments of track_velocity_host / ops.box_velocity."""
    return [case[k] for k in ("box", "flags", "mask_off", "class_id", "frame_next", "frame_time", "track_group", "max_speed", "max_dt")]


def _pairs_of_scenes(n):
    """frame_next of n two-frame scenes back to back: 0 -> 1, 2 -> 3, ..."""
    nxt = np.full(2 * n, -1, np.int32)
    nxt[0::2] = np.arange(1, 2 * n, 2)
    return nxt


# ---------------------------------------------------------------------------------------------------------------- links
def link_cases():
    out = []
    p = np.array([[8.0, 16.0], [40.0, -24.0]])
    step = np.array([[1.0, 0.5], [-0.5, 0.25]])
    out.append(_case("last_frame", [(p, 0, 3), (p + step, 0, 3), (p + 2 * step, 0, 3)], [1, 2, -1], [0.0, 0.5, 1.0],
                     expect=dict(next_match=[2, 3, 4, 5, -1, -1], prev_match=[-1, -1, 0, 1, 2, 3], vel_src=[1, 1, 3, 3, 2, 2])))
    # the seam of two scenes: frames 1 and 2 hold the same boxes and are no link
    out.append(_case("two_scenes", [(p, 0, 3), (p + step, 0, 3), (p + step, 0, 3), (p + 2 * step, 0, 3)], [1, -1, 3, -1],
                     [0.0, 0.5, 20.0, 20.5],
                     expect=dict(next_match=[2, 3, -1, -1, 6, 7, -1, -1], prev_match=[-1, -1, 0, 1, -1, -1, 4, 5],
                                 vel_src=[1, 1, 2, 2, 1, 1, 2, 2])))
    out.append(_case("dt_exactly_max_dt", [(p, 0, 3), (p + step, 0, 3)], [1, -1], [0.0, 1.5],
                     expect=dict(next_match=[2, 3, -1, -1], vel_src=[1, 1, 2, 2])))
    out.append(_case("dt_one_ulp_above_max_dt", [(p, 0, 3), (p + step, 0, 3)], [1, -1], [0.0, np.nextafter(1.5, 2.0)],
                     expect=dict(next_match=[-1] * 4, prev_match=[-1] * 4, vel_src=[0] * 4, vel=np.zeros((4, 2)))))
    out.append(_case("dt_zero_and_negative", [(p, 0, 3), (p, 0, 3), (p, 0, 3), (p, 0, 3)], [1, -1, 3, -1], [1.0, 1.0, 1.0, 0.5],
                     expect=dict(next_match=[-1] * 8, prev_match=[-1] * 8, vel_src=[0] * 8)))
    # 0 -> 1 -> 2 -> 3, frame 1 without a kept box: frame 0 gets nothing, frames 2 and 3 one-sided velocities
    out.append(_case("middle_frame_not_kept", [(p, 0, 3), (p + step, 0, 1), (p + 2 * step, 0, 3), (p + 3 * step, 0, 3)], [1, 2, 3, -1],
                     [0.0, 0.5, 1.0, 1.5],
                     expect=dict(next_match=[-1, -1, -1, -1, 6, 7, -1, -1], vel_src=[0, 0, 0, 0, 1, 1, 2, 2])))
    out.append(_case("middle_frame_empty", [(p, 0, 3), (np.zeros((0, 2)), 0, 3), (p + 2 * step, 0, 3)], [1, 2, -1], [0.0, 0.5, 1.0],
                     expect=dict(next_match=[-1] * 4, prev_match=[-1] * 4, vel_src=[0] * 4)))
    for bad in (7, 4, -2):                     # F = 4: 4 is the first index outside
        out.append(_case(f"frame_next_out_of_range_{bad}", [(p, 0, 3), (p + step, 0, 3), (p, 0, 3), (p + step, 0, 3)], [bad, -1, 3, -1],
                         [0.0, 0.5, 9.0, 9.5],
                         expect=dict(status=1, next_match=[-1, -1, -1, -1, 6, 7, -1, -1], prev_match=[-1] * 6 + [4, 5],
                                     vel_src=[0, 0, 0, 0, 1, 1, 2, 2])))
    out.append(chain_case())
    return out


CHAIN_COUNTS = (5, 6, 4, 7)


def chain_case():
    """0 -> 1 -> 2 -> 3: three links in the slots 0, 1, 2 (pair_off 0, 30, 54, 82, 82), boxes 64 m apart (gate: 20 m) that move by
    (1, 0.5) a frame; frame k shows the first CHAIN_COUNTS[k] of them, one of frame 1 is not kept.  The batch of the tests that hand
    cm3d_box_velocity a pair_off that disagrees with it."""
    p = np.array([[64.0 * i, 8.0 * (i % 3)] for i in range(max(CHAIN_COUNTS))]) + [900.0, 1800.0]
    frames = [(p[:n] + k * np.array([1.0, 0.5]), 0, 3) for k, n in enumerate(CHAIN_COUNTS)]
    frames[1] = (frames[1][0], 0, [3, 3, 1, 3, 3, 3])
    return _case("three_link_chain", frames, [1, 2, 3, -1], [0.0, 0.5, 1.0, 1.5],
                 expect=dict(pair_off=[0, 30, 54, 82, 82], next_match=[5, 6, -1, 8, 9] + [11, 12, -1, 14, -1, -1] + [15, 16, 17, 18] + [-1] * 7,
                             vel_src=[1, 1, 0, 1, 1] + [3, 3, 0, 3, 2, 0] + [3, 3, 1, 3] + [2, 2, 2, 2, 0, 0, 0]))


# ------------------------------------------------------------------------------------------------------------- capacity
OVER_CAPACITY_COUNTS = [(1025, 3), (3, 1025), (5, 4)]


def capacity_cases():
    """Three two-frame scenes; the first two hold a frame of 1025 masks, one more than CM3D_MAX_MASKS_PER_FRAME, on either side of
    their link: status bit 1, no pair in their slots, no match; the third scene's link is untouched."""
    rng = np.random.default_rng(11)
    frames = [fr for P, G in OVER_CAPACITY_COUNTS for fr in _scatter_link(rng, P, G)]
    n = len(OVER_CAPACITY_COUNTS)
    times = np.repeat(np.arange(n) * 30.0, 2) + np.tile([0.0, 0.5], n)
    return [_case("over_capacity", frames, _pairs_of_scenes(n), times, max_speed=[8.0, 6.0, 4.0],
                  expect=dict(status=2, pair_off=[0, 0, 0, 0, 0, 20, 20]))]


# ---------------------------------------------------------------------------------------------------------------- clamp
def clamp_cases():
    """(case, the same case with mask_off as the rule reads it) pairs: a mask_off whose last entry lies beyond the masks, one whose
    first entry is negative.  Every frame's range is clamped into [0, M] (velocity._frame_masks, track_frame_masks), so each is the
    batch `two_scenes` -- whose first and last frame are both part of a link -- with mask_off = 0, 2, 4, 6, 8.  Not members of
    all_cases(): the plain loop of test_velocity_host takes mask_off as it stands."""
    base = by_name("two_scenes")
    M = len(base["flags"])
    hi, lo = base["mask_off"].copy(), base["mask_off"].copy()
    hi[-1], lo[0] = M + 1000, -5
    return [(dict(base, name="mask_off_last_beyond", mask_off=hi, expect={}), base),
            (dict(base, name="mask_off_first_negative", mask_off=lo, expect={}), base)]


# -------------------------------------------------------------------------------------------------------------- weights
def weight_cases():
    out = []
    o = np.array([[8.0, 16.0]])
    # classes 0 (group 0) against 1 (group 1): no match; classes 1 and 2 share group 1: a match
    out.append(_case("group_mismatch", [(np.repeat(o, 2, 0) + [[0, 0], [64, 0]], [0, 1], 3), (np.repeat(o, 2, 0) + [[0, 0], [64, 0]], [1, 2], 3)],
                     [1, -1], [0.0, 0.5], expect=dict(next_match=[-1, 3, -1, -1], prev_match=[-1, -1, -1, 1], weights={0: [[0, 0], [0, 1000000]]})))
    xy = o + np.array([[0.0, 0.0], [64.0, 0.0], [128.0, 0.0], [192.0, 0.0]])
    out.append(_case("not_kept_either_side", [(xy, 0, [3, 1, 3, 2]), (xy, 0, [3, 3, 0, 3])], [1, -1], [0.0, 0.5],
                     expect=dict(next_match=[4, -1, -1, -1, -1, -1, -1, -1], prev_match=[-1, -1, -1, -1, 0, -1, -1, -1])))
    # group 1: 5 m/s, dt = 0.5: gate = 2.5, gate^2 = 6.25 = 1.5^2 + 2^2 exactly
    # (from the origin: the ulp of 2.0 survives the subtraction)
    z = np.zeros((1, 2))
    on, off_ = np.array([[1.5, 2.0]]), np.array([[1.5, np.nextafter(2.0, 3.0)]])
    assert (1.5 * 1.5) + (2.0 * 2.0) == 6.25 and (1.5 * 1.5) + (off_[0, 1] - 0.0) ** 2 > 6.25
    out.append(_case("on_the_gate", [(z, 1, 3), (on, 1, 3)], [1, -1], [0.0, 0.5],
                     expect=dict(next_match=[1, -1], prev_match=[-1, 0], weights={0: [[1]]}, vel=[[3.0, 4.0], [3.0, 4.0]])))
    out.append(_case("one_ulp_outside_the_gate", [(z, 1, 3), (off_, 1, 3)], [1, -1], [0.0, 0.5],
                     expect=dict(next_match=[-1, -1], prev_match=[-1, -1], weights={0: [[0]]})))
    out.append(_case("identical_centres", [(o, 0, 3), (o, 0, 3)], [1, -1], [0.0, 0.5],
                     expect=dict(next_match=[1, -1], weights={0: [[1000000]]}, vel=np.zeros((2, 2)), vel_src=[1, 2])))
    rng = np.random.default_rng(41)
    g = np.array([1013.25, 2391.5]) + rng.uniform(-60, 60, (24, 2))               # global-frame magnitudes
    mv = rng.uniform(-4, 4, (24, 2))
    out.append(_case("global_magnitude", [(g, 0, 3), (g + mv * 0.5, 0, 3), (g + mv, 0, 3)], [1, 2, -1], [0.0, 0.5, 1.0]))
    return out


# ---------------------------------------------------------------------------------------------------------------- assign
def greedy_total(W):
    """Total weight of the greedy pairing: the heaviest remaining pair first (the nearest neighbours first)."""
    W = np.array(W, np.int64)
    total = 0
    while W.size and W.max() > 0:
        i, j = np.unravel_index(np.argmax(W), W.shape)
        total += int(W[i, j])
        W[i, :], W[:, j] = 0, 0
    return total


def _scatter_link(rng, P, G, side=None):
    """A link of P against G boxes: G's boxes are P's moved by up to a few metres (as far as there are), the rest fresh; a tenth not
    kept, three classes.  The area grows with the count so that a box sees a handful of candidates."""
    side = side or 6.0 * np.sqrt(max(P, G, 1))
    a = rng.uniform(0, side, (P, 2))
    k = min(P, G)
    b = np.concatenate([a[rng.permutation(P)[:k]] + rng.uniform(-2.0, 2.0, (k, 2)), rng.uniform(0, side, (G - k, 2))])[rng.permutation(G)]
    def extras(n):
        return rng.choice([0, 0, 0, 1, 2], n).astype(np.int32), np.where(rng.random(n) < 0.1, rng.choice([0, 1, 2], n), 3).astype(np.int32)
    return (a,) + extras(P), (b,) + extras(G)


def assign_cases():
    out = []
    # b and c are each other's nearest neighbour; the optimum pairs a-c and b-d (gate 2.5: a-d lies outside)
    f = np.array([[0.0, 0.0], [2.0, 0.0]])             # a, b
    n = np.array([[1.2, 0.0], [3.0, 0.0]])             # c, d
    out.append(_case("mutual_nearest_neighbours", [(f, 1, 3), (n, 1, 3)], [1, -1], [0.0, 0.5], expect=dict(next_match=[2, 3, -1, -1])))
    # domino: row i between columns i and i + 1, a shade nearer to i; the last row on column 0 shifts every earlier row by one
    K = 40
    cols = np.stack([np.arange(K) * 1.0, np.zeros(K)], 1)
    rows = np.concatenate([np.stack([np.arange(K - 1) + 0.5 - 1.0 / 64, np.zeros(K - 1)], 1), [[0.0, 0.0]]])
    out.append(_case("domino_chain", [(rows, 1, 3), (cols, 1, 3)], [1, -1], [0.0, 0.5],
                     expect=dict(next_match=list(K + 1 + np.arange(K - 1)) + [K] + [-1] * K)))
    same = np.full((7, 2), 3.5)
    # only the tie rule decides: an unassigned column first, then the lowest -- row i takes column i
    out.append(_case("all_equal_5x7", [(same[:5], 0, 3), (same, 0, 3)], [1, -1], [0.0, 0.5],
                     expect=dict(next_match=[5, 6, 7, 8, 9] + [-1] * 7)))
    out.append(_case("all_equal_7x5", [(same, 0, 3), (same[:5], 0, 3)], [1, -1], [0.0, 0.5],
                     expect=dict(next_match=[7, 8, 9, 10, 11, -1, -1] + [-1] * 5)))
    rng = np.random.default_rng(7)
    for name, counts in (("instance_borders", COUNTS), ("lds_l2_seam", SEAM_COUNTS), ("widest_instance", [(1024, 300)])):
        frames = [fr for P, G in counts for fr in _scatter_link(rng, P, G)]
        times = np.repeat(np.arange(len(counts)) * 30.0, 2) + np.tile([0.0, 0.5], len(counts))
        out.append(_case(name, frames, _pairs_of_scenes(len(counts)), times, max_speed=[8.0, 6.0, 4.0]))
    return out


# -------------------------------------------------------------------------------------------------------------- velocity
def velocity_cases():
    rng = np.random.default_rng(3)
    k = 12
    p0 = rng.integers(-64, 64, (k, 2)) * 8.0 + np.array([1024.0, 2048.0])      # 8 m apart at least: no ambiguity
    v = rng.integers(-16, 17, (k, 2)) * 0.25                                   # up to 4 m/s, dyadic
    frames = [(p0 + v * t, 0, 3) for t in (0.0, 0.5, 1.0)]
    idx = np.arange(k)
    common = dict(next_match=list(k + idx) + list(2 * k + idx) + [-1] * k, prev_match=[-1] * k + list(idx) + list(k + idx),
                  vel=np.tile(v, (3, 1)))
    return [_case("constant_velocity", frames, [1, 2, -1], [0.0, 0.5, 1.0], expect=dict(common, vel_src=[1] * k + [3] * k + [2] * k)),
            # the central span is 1.0 > max_dt: the middle frame falls back to the forward difference
            _case("central_span_above_max_dt", frames, [1, 2, -1], [0.0, 0.5, 1.0], max_dt=0.75,
                  expect=dict(common, vel_src=[1] * k + [1] * k + [2] * k))]


@functools.lru_cache(maxsize=None)
def all_cases():
    cases = link_cases() + weight_cases() + assign_cases() + velocity_cases() + capacity_cases()
    assert len({c["name"] for c in cases}) == len(cases)
    return cases


def by_name(name):
    return next(c for c in all_cases() if c["name"] == name)
