"""Inputs of the ground stage's tests (cm3d_box_ground; numpy and, for the clouds, the CPU oracle's sweep preparation): (a) small
clouds built to sit on the rule's edges, (b) the apply table, (c) frames of 130 and 70 masks that cross a workgroup's chunk of masks (64
at the most, fewer where the launch wants more workgroups) twice and once at least, with two sweeps of different transforms, (d) the two-frame nuScenes and Waymo batches of the pass tests with a tilted
ground sheet of rings in every frame -- and a scalar loop written apart from the host statement (one mask and one point at a time,
Python floats) that both the host statement and the device are held against.

A case holds the raw rows (five floats each, sensor frame) of its sweeps with their transforms; cloud() is the oracle's sweep
preparation of them, the cloud every expectation starts from.  Every frame's rows are padded with NaN rows to a multiple of four, as
the loader pads the quad layout, so that one set of offsets serves all three layouts (raw_layouts)."""
import math
from types import SimpleNamespace

import numpy as np

BOX_STRIDE = 10
BINS, CHUNK = 128, 64                               # include/cm3d_hip.h: CM3D_GROUND_BINS, CM3D_GROUND_CHUNK (the largest chunk)
DEFAULTS = dict(radius=3.0, quantile=0.1, min_points=20, down=5.0, up=0.5, lo=0.7, hi=1.3)
DZ = (5.0 + 0.5) / 128.0                            # 11 / 256: exact
IDENTITY = np.array([1, 0, 0, 0, 1, 0, 0, 0, 1, 0, 0, 0] * 2, np.float32)
PRIOR = np.array([[2.1, 4.9, 1.7], [0.7, 0.8, 1.75], [2.9, 11.0, 3.5]], np.float64)
f32 = np.float32


def _up(v):
    return float(np.nextafter(f32(v), f32(np.inf)))


def _dn(v):
    return float(np.nextafter(f32(v), f32(-np.inf)))


def _xf(rng, centre):
    """A sweep transform in the sweep preparation's record: two rotations and translations, float32."""
    def rot(yaw, tilt):
        c, s = np.cos(yaw), np.sin(yaw)
        Rz = np.array([[c, -s, 0], [s, c, 0], [0, 0, 1.0]])
        ct, st = np.cos(tilt), np.sin(tilt)
        return Rz @ np.array([[1, 0, 0], [0, ct, -st], [0, st, ct]])
    return np.concatenate([rot(rng.uniform(-3, 3), rng.normal() * 0.01).reshape(-1), [0.9, 0.0, 1.84],
                           rot(rng.uniform(-3, 3), rng.normal() * 0.01).reshape(-1), centre]).astype(np.float32)


class _Builder:
    """Frames of sweeps and masks -> a case."""

    def __init__(self, name, halfw, prior=PRIOR):
        self.name, self.halfw, self.prior = name, float(f32(halfw)), np.asarray(prior, np.float64)
        self.sweeps, self.fso, self.mask_off = [], [0], [0]
        self.rows, self.names = [], []              # per mask: (cx, cy, zref, class column, flags, vert_status, vert top, vert_h)

    def frame(self, sweeps, masks):
        """sweeps: [(points (n, 3), xf (24,))]; the frame's last sweep gets its NaN padding.  masks: [(name, cx, cy, zref, class column,
        flags, vert_status, vert top, vert_h)]."""
        n = sum(len(p) for p, _ in sweeps)
        pad = (-n) % 4
        for i, (p, xf) in enumerate(sweeps):
            rows = np.zeros((len(p), 5), np.float32)
            rows[:, :3] = np.asarray(p, np.float32).reshape(-1, 3)
            rows[:, 3], rows[:, 4] = 7.0, np.arange(len(p)) % 32
            if i == len(sweeps) - 1 and pad:
                tail = np.full((pad, 5), np.nan, np.float32)
                rows = np.concatenate([rows, tail], 0)
            self.sweeps.append((rows, np.asarray(xf, np.float32)))
        assert not (pad and not sweeps)
        self.fso.append(len(self.sweeps))
        for m in masks:
            self.names.append(m[0]), self.rows.append(m[1:])
        self.mask_off.append(len(self.rows))

    def case(self, rng, runs, with_vert=True, zref_given=True, **more):
        M = len(self.rows)
        r = np.array(self.rows, np.float64).reshape(M, 8)
        box = rng.normal(0.0, 20.0, (M, BOX_STRIDE))
        box[:, 0], box[:, 1], box[:, 8], box[:, 9] = r[:, 0], r[:, 1], r[:, 3], r[:, 4]
        # with zref handed in, column 2 holds what a vertical stage may have left there: something else
        box[:, 2] = r[:, 2] + 0.125 if zref_given else r[:, 2]
        vert = None
        if with_vert:
            vz = rng.normal(0.0, 1.0, (M, 2))
            vz[:, 1] = r[:, 6]
            vert = dict(vert_status=r[:, 5].astype(np.int32), vert_z=vz, vert_h=r[:, 7].copy())
        row_off = np.concatenate([[0], np.cumsum([len(s[0]) for s in self.sweeps])]).astype(np.int32)
        return dict(name=self.name, names=self.names, sweeps=self.sweeps, sweep_row_off=row_off, frame_sweep_off=np.array(self.fso, np.int32),
                    halfw=self.halfw, mask_off=np.array(self.mask_off, np.int32), box=box, flags=r[:, 4].astype(np.int32),
                    prior_wlh=self.prior, zref=r[:, 2].copy() if zref_given else None, vert=vert, runs=runs, **more)


def _stack(x, y, zs):
    """Points at (x, y) with the heights zs."""
    zs = np.asarray(zs, np.float64).reshape(-1)
    return np.stack([np.full(zs.size, x), np.full(zs.size, y), zs], 1)


def _bin_z(zref, b, frac=0.5):
    """A height inside bin b of the default window around zref."""
    return zref - 5.0 + (b + frac) * DZ


# ------------------------------------------------------------------------------------------------ (a) the rule's edges
def edges_case(with_vert=True):
    """Frame 0 (identity transform, so the cloud is the rows to the bit; ego box 1.5 m): one mask per edge, 20 m apart.  Frame 1: a mask
    at the x, y of frame 0's first with other points.  Frame 2: rows, no mask.  Frame 3: masks, no sweep.  Frame 4: masks, a sweep
    without rows."""
    rng = np.random.default_rng(2901)
    b = _Builder("edges" if with_vert else "edges_no_vertical", 1.5)
    pts, masks = [], []
    ok = (0.0, 3, 0, 1.2, 1.7)                      # class 0, flags 3, vert_status 0, a top of 1.2, vert_h

    def add(name, cx, cy, zref, p, cls=ok[0], flags=ok[1], vs=ok[2], top=ok[3], vh=ok[4]):
        masks.append((name, cx, cy, zref, cls, flags, vs, top, vh))
        pts.append(np.asarray(p, np.float64).reshape(-1, 3))
    gz = lambda zref, n, b0=90: _bin_z(zref, b0 + np.arange(n) % 3)        # n ground heights over three bins below zref
    # the circle: 20 points on it at (cx + 3, cy) and (cx, cy - 3), 5 on the next float32 outside -- n is 20, not 25
    add("on_circle", 100.0, 40.0, 1.0, np.concatenate([_stack(103.0, 40.0, gz(1.0, 10)), _stack(100.0, 37.0, gz(1.0, 10)),
                                                       _stack(_up(103.0), 40.0, gz(1.0, 3)), _stack(100.0, _dn(37.0), gz(1.0, 2))]))
    # the window: z0 itself (bin 0), one float32 below it (out), a bin edge (bin 10, not 9), the window's end (out), one below it (bin 127)
    z0 = 1.0 - 5.0
    add("window", 120.0, 40.0, 1.0, _stack(121.0, 40.5, [z0] * 6 + [_dn(z0)] * 4 + [z0 + 10 * DZ] * 7 + [1.5] * 5 + [_dn(1.5)] * 8))
    add("few_19", 140.0, 40.0, 1.0, _stack(141.0, 41.0, gz(1.0, 19)))
    add("enough_20", 160.0, 40.0, 1.0, _stack(161.0, 41.0, gz(1.0, 20)))
    # k = (int)(0.1 * 20) = 2: the third point in ascending order -- the last of bin 80's three, or the first of bin 85 behind bin 80's two
    add("k_last_of_bin", 180.0, 40.0, 1.0, _stack(181.0, 41.0, [_bin_z(1.0, 80)] * 3 + [_bin_z(1.0, 85)] * 18))
    add("k_first_of_next", 200.0, 40.0, 1.0, _stack(201.0, 41.0, [_bin_z(1.0, 80)] * 2 + [_bin_z(1.0, 85)] * 19))
    add("one_bin", 220.0, 40.0, 1.0, _stack(221.0, 41.0, _bin_z(1.0, 92, rng.uniform(0.05, 0.95, 30))))
    add("last_bins", 240.0, 40.0, 1.0, _stack(241.0, 41.0, _bin_z(1.0, 126 + np.arange(24) % 2)))       # the scan's last lane
    add("nan_cx", np.nan, 40.0, 1.0, np.zeros((0, 3)))
    add("inf_cy", 260.0, np.inf, 1.0, _stack(260.0, 41.0, gz(1.0, 20)))
    add("nan_zref", 280.0, 40.0, np.nan, _stack(281.0, 41.0, gz(1.0, 20)))
    add("inf_zref", 300.0, 40.0, -np.inf, _stack(301.0, 41.0, gz(1.0, 20)))
    add("flags_0", 320.0, 40.0, 1.0, _stack(321.0, 41.0, gz(1.0, 25)), flags=0)
    add("flags_2", 340.0, 40.0, 1.0, _stack(341.0, 41.0, gz(1.0, 25)), flags=2)
    add("class_below", 360.0, 40.0, 1.0, _stack(361.0, 41.0, gz(1.0, 25)), cls=-1.0)
    add("class_above", 380.0, 40.0, 1.0, _stack(381.0, 41.0, gz(1.0, 25)), cls=float(len(PRIOR)))
    add("class_nan", 400.0, 40.0, 1.0, _stack(401.0, 41.0, gz(1.0, 25)), cls=np.nan)
    add("class_fraction", 420.0, 40.0, 1.0, _stack(421.0, 41.0, gz(1.0, 25)), cls=1.75)
    # -0.0 coordinates, and the ego box: the rows at |x|, |y| < 1.5 are dropped (12 of them), those at y = 2 with x = -0.0 stay (22)
    add("ego_box", -0.0, 2.5, 1.0, np.concatenate([_stack(-0.0, 2.0, gz(1.0, 22)), _stack(0.5, -0.0, gz(1.0, 6)), _stack(-1.25, 1.25, gz(1.0, 6))]))
    add("non_finite_points", 440.0, 40.0, 1.0, np.concatenate([_stack(441.0, 41.0, gz(1.0, 21)), [[np.nan, 41.0, -1.0], [441.0, np.inf, -1.0],
                                                                                                  [441.0, 41.0, np.nan], [441.0, 41.0, -np.inf]]]))
    add("empty_circle", 460.0, 40.0, 1.0, _stack(464.0, 40.0, gz(1.0, 20)))
    add("own_points_count", 480.0, 40.0, 1.0, np.concatenate([_stack(481.0, 41.0, gz(1.0, 12)), _stack(480.0, 40.0, _bin_z(1.0, 100 + np.arange(16)))]))
    order = rng.permutation(sum(len(p) for p in pts))                          # the order of arrival is not the masks' order
    b.frame([(np.concatenate(pts, 0)[order], IDENTITY)], masks)
    b.frame([(_stack(101.0, 41.0, _bin_z(1.0, 60 + np.arange(26) % 2)), IDENTITY)], [("other_frame_same_xy", 100.0, 40.0, 1.0) + ok])
    b.frame([(_stack(100.5, 40.5, gz(1.0, 40)), IDENTITY)], [])
    b.frame([], [("frame_without_sweeps", 100.0, 40.0, 1.0) + ok, ("frame_without_sweeps_nan", np.nan, 40.0, 1.0) + ok])
    b.frame([(np.zeros((0, 3)), IDENTITY)], [("sweep_without_rows", 100.0, 40.0, 1.0) + ok])
    expect = dict(on_circle=(0, 20), window=(0, 21), few_19=(1, 19), enough_20=(0, 20), k_last_of_bin=(0, 21), k_first_of_next=(0, 21),
                  one_bin=(0, 30), last_bins=(0, 24), nan_cx=(4, 0), inf_cy=(4, 0), nan_zref=(4, 0), inf_zref=(4, 0), ego_box=(0, 22),
                  non_finite_points=(0, 21), empty_circle=(2, 0), own_points_count=(0, 28), other_frame_same_xy=(0, 26),
                  frame_without_sweeps=(2, 0), frame_without_sweeps_nan=(4, 0), sweep_without_rows=(2, 0))
    bins = dict(window=0, k_last_of_bin=80, k_first_of_next=85, one_bin=92, last_bins=126, other_frame_same_xy=60)
    runs = [{}, dict(min_points=1), dict(quantile=0.0), dict(quantile=1.0), dict(min_points=21), dict(radius=_dn(3.0)), dict(radius=1.0e-3)]
    return b.case(rng, runs, with_vert=with_vert, zref_given=with_vert, expect=expect, bins=bins)


# ------------------------------------------------------------------------------------------------ (b) the apply table
def apply_case(with_vert=True):
    """Every mask has 24 members in bin 92 of the default window around zref = 1: g = -4 + 92.5 * 11 / 256 = -0.025390625, exact, and
    zref - g = 1.025390625.  The runs move lo and hi one ulp around the ratio of mask 0 ((1.5 - g) / 1.7)."""
    rng = np.random.default_rng(2902)
    g = -4.0 + 92.5 * DZ
    assert g == -0.025390625
    edge = 1.0 - g - 0.5                            # the prior height at which zref - g == h0 + UP, exact
    prior = np.array([[2.0, 4.5, 1.7], [1.0, 1.0, 0.0], [1.0, 1.0, -1.6], [1.0, 1.0, np.nan], [1.0, 1.0, np.inf], [0.6, 0.7, edge],
                      [0.6, 0.7, edge - 2.0 ** -40], [0.5, 0.5, 0.3]], np.float64)
    b = _Builder("apply" if with_vert else "apply_no_vertical", 0.0, prior)
    rows = [("ratio", 0.0, 3, 0, 1.5), ("ground_and_top", 0.0, 1, 0, 1.6), ("top_below_ground", 0.0, 3, 0, -1.0), ("top_too_low", 0.0, 3, 0, 0.5),
            ("top_too_high", 0.0, 3, 0, 4.0), ("top_too_high_short_class", 7.0, 3, 0, 4.0), ("vertical_few", 0.0, 3, 1, 1.6),
            ("vertical_empty", 0.0, 3, 2, 1.6), ("vertical_not_finite", 0.0, 3, 4, 1.6), ("top_nan", 0.0, 3, 0, np.nan), ("top_inf", 0.0, 3, 0, np.inf),
            ("h0_zero", 1.0, 3, 0, 1.6), ("h0_negative", 2.0, 3, 0, 1.6), ("h0_nan", 3.0, 3, 0, 1.6), ("h0_inf", 4.0, 3, 0, 1.6),
            ("medoid_on_the_edge", 5.0, 3, 1, 1.6), ("medoid_above_the_edge", 6.0, 3, 1, 1.6), ("medoid_far_above", 7.0, 3, 1, 1.6),
            ("flags_0", 0.0, 0, 0, 1.6), ("flags_2", 0.0, 2, 0, 1.6)]
    pts, masks = [], []
    for i, (name, cls, flags, vs, top) in enumerate(rows):
        cx = 50.0 + 10.0 * i
        masks.append((name, cx, -30.0, 1.0, cls, flags, vs, top, 1.5 + 0.01 * i))
        pts.append(_stack(cx + 1.0, -29.0, _bin_z(1.0, 92, rng.uniform(0.05, 0.95, 24))))
    masks.append(("few_members", 400.0, -30.0, 1.0, 0.0, 3, 0, 1.6, 1.9))
    pts.append(_stack(401.0, -29.0, _bin_z(1.0, 92, rng.uniform(0.05, 0.95, 19))))
    b.frame([(np.concatenate(pts, 0), IDENTITY)], masks)
    r0 = (1.5 - g) / 1.7
    up, dn = float(np.nextafter(r0, np.inf)), float(np.nextafter(r0, -np.inf))
    runs = [{}, dict(lo=up, hi=2.0), dict(lo=r0, hi=2.0), dict(lo=dn, hi=2.0), dict(lo=0.1, hi=up), dict(lo=0.1, hi=r0), dict(lo=0.1, hi=dn),
            dict(lo=r0, hi=r0), dict(up=0.25), dict(down=4.0)]
    # mask 0 in each run with the vertical inputs: the ratio one ulp below lo or above hi falls to source 2 (zref - g <= 1.7 + UP)
    src = dict(ratio=1, ground_and_top=1, top_below_ground=2, top_too_low=2, top_too_high=2, top_too_high_short_class=0, vertical_few=2,
               vertical_empty=2, vertical_not_finite=2, top_nan=2, top_inf=2, h0_zero=0, h0_negative=0, h0_nan=0, h0_inf=0, medoid_on_the_edge=2,
               medoid_above_the_edge=0, medoid_far_above=0, flags_0=0, flags_2=0, few_members=0)
    if not with_vert:
        src = {k: (2 if v == 1 else v) for k, v in src.items()}
    return b.case(rng, runs, with_vert=with_vert, zref_given=False, src=src, mask0_src=[1, 2, 1, 1, 1, 1, 2, 1] if with_vert else [2] * 8, g=g)


# ------------------------------------------------------------------------------------------------ (c) many masks, two sweeps
def many_case():
    """130, 70 and 3 masks in three frames of 2048, 1500 and 600 rows; frame 0 has two sweeps with transforms of their own.  A cloud of a
    ground sheet with bumps, an ego box of sqrt(2.3) m around each sensor, centres drawn among the points."""
    rng = np.random.default_rng(2903)
    b = _Builder("many", math.sqrt(2.3))
    for n_masks, n_sweeps, n_rows in ((130, 2, 2046), (70, 1, 1499), (3, 1, 600)):
        centre = np.array([600.0, 1600.0, 1.0]) + rng.normal(0, 50, 3) * [1, 1, 0.01]
        sweeps, cloud = [], []
        for s in range(n_sweeps):
            n = n_rows // n_sweeps
            p = np.stack([rng.uniform(-14, 14, n), rng.uniform(-14, 14, n), -1.84 + rng.normal(0, 0.05, n)], 1)
            tall = rng.random(n) < 0.25
            p[tall, 2] += rng.uniform(0.0, 3.0, int(tall.sum()))
            xf = _xf(rng, centre + [0.4 * s, 0.0, 0.0])
            sweeps.append((p, xf))
            x64 = xf.astype(np.float64)
            cloud.append((p @ x64[0:9].reshape(3, 3).T + x64[9:12]) @ x64[12:21].reshape(3, 3).T + x64[21:24])
        cloud = np.concatenate(cloud, 0)
        masks = []
        for i in range(n_masks):
            c = cloud[rng.integers(0, len(cloud))] + rng.normal(0, 0.5, 3)
            cls = float(rng.integers(0, len(PRIOR)))
            zref = c[2] + rng.uniform(0.0, 2.5)
            vs = int(rng.choice([0, 0, 0, 1, 2, 4]))
            masks.append((f"m{i}", c[0], c[1], zref, cls, int(rng.choice([3, 3, 1, 0])), vs, zref + rng.uniform(0.0, 1.5), rng.uniform(0.5, 3.0)))
        masks[n_masks // 2] = ("nan", np.nan) + masks[n_masks // 2][2:]
        b.frame(sweeps, masks)
    return b.case(rng, [{}, dict(radius=1.5, quantile=0.5, min_points=5, down=2.0, up=1.0)])


def padded(case, name, in_front, behind):
    """The case with frames that have neither sweeps nor masks in front of and behind its own: the same masks and rows, more frames.
    The launch sizes a workgroup's chunk of masks from the batch's shape (cm3d_box_ground_chunk): few frames give the smallest
    chunk, 8, many give the largest, 64."""
    fso, mo = case["frame_sweep_off"], case["mask_off"]
    pad = lambda off: np.concatenate([np.full(in_front, off[0]), off, np.full(behind, off[-1])]).astype(np.int32)
    return dict(case, name=name, frame_sweep_off=pad(fso), mask_off=pad(mo))


# (name, frames in front, frames behind, the chunk the launch takes): 130 masks cross a chunk of 8, of 33 and of 64 twice and more;
# with 33 and 64 every wave of the workgroup scans, and a wave scans more than one mask
MANY_SHAPES = (("many", 0, 0, 8), ("many_chunk33", 20, 41, 33), ("many_chunk64", 60, 65, 64))


def all_cases():
    many = many_case()
    return [edges_case(True), edges_case(False), apply_case(True), apply_case(False), many, dict(many, name="many_own_zref", zref=None)] + \
        [padded(many, name, a, b) for name, a, b, _ in MANY_SHAPES[1:]]


# ------------------------------------------------------------------------------------------------ the clouds and the layouts
def cloud(orc, case):
    """The oracle's sweep preparation of the case's rows: (points (n_rows, 4) float32 at the raw row index, the rows it drops as NaN --
    what cm3d_sweep_prep's `points` holds --, pt_off (F + 1,))."""
    out = []
    for rows, xf in case["sweeps"]:
        pts = np.full((len(rows), 4), np.nan, np.float32)
        with np.errstate(invalid="ignore"):
            drop = (np.abs(rows[:, 0]) < f32(case["halfw"])) & (np.abs(rows[:, 1]) < f32(case["halfw"]))
        if len(rows):
            kept = orc.sweep_prep(rows, xf[0:9], xf[9:12], xf[12:21], xf[21:24], case["halfw"])
            assert len(kept) == int((~drop).sum())
            pts[~drop] = kept
        pts[drop, 3] = rows[drop, 3]
        out.append(pts)
    pts = np.concatenate(out, 0) if out else np.zeros((0, 4), np.float32)
    return pts, case["sweep_row_off"][case["frame_sweep_off"]].astype(np.int32)


def raw_layouts(case):
    """{name: (raw flat float32, raw_stride)}: the rows with five floats, with four, and the quad layout (every frame starts on a
    multiple of four rows by the builder's padding)."""
    rows = np.concatenate([s[0] for s in case["sweeps"]], 0) if case["sweeps"] else np.zeros((0, 5), np.float32)
    assert all(int(v) % 4 == 0 for v in case["sweep_row_off"][case["frame_sweep_off"]])
    n = len(rows)
    padded = np.full(((n + 3) // 4 * 4, 3), np.nan, np.float32)
    padded[:n] = rows[:, :3]
    quads = np.ascontiguousarray(padded.reshape(-1, 4, 3).transpose(0, 2, 1))       # x0 x1 x2 x3 y0 .. y3 z0 .. z3 per four rows
    return {"stride5": (rows.reshape(-1).copy(), 5), "stride4": (np.ascontiguousarray(rows[:, :4]).reshape(-1), 4), "quads": (quads.reshape(-1), 3)}


def sweep_xf(case):
    return np.stack([s[1] for s in case["sweeps"]]) if case["sweeps"] else np.zeros((0, 24), np.float32)


def params(run):
    return dict(DEFAULTS, **run)


# ------------------------------------------------------------------------------------------------ the scalar loop
def loop_ground(case, points, pt_off, radius=3.0, quantile=0.1, min_points=20, down=5.0, up=0.5, lo=0.7, hi=1.3):
    """The rule of include/cm3d_hip.h, one mask and one point at a time, in Python floats (IEEE doubles, every operation rounded)."""
    pts = np.asarray(points, np.float32)[:, :3].astype(np.float64).tolist()
    box = case["box"].copy()
    M, prior, vert = box.shape[0], case["prior_wlh"], case["vert"]
    out = dict(box=box, ground_z=np.zeros(M), ground_n=np.zeros(M, np.int32), ground_h=np.zeros(M), ground_src=np.zeros(M, np.int32),
               ground_status=np.zeros(M, np.int32), ground_zref=np.zeros(M))
    fin = lambda v: not (math.isnan(v) or math.isinf(v))
    dz = (down + up) / 128.0
    for f in range(len(pt_off) - 1):
        frame_pts = [p for p in pts[int(pt_off[f]):int(pt_off[f + 1])] if fin(p[0]) and fin(p[1]) and fin(p[2])]
        for m in range(int(case["mask_off"][f]), int(case["mask_off"][f + 1])):
            cx, cy = float(box[m, 0]), float(box[m, 1])
            zref = float(box[m, 2]) if case["zref"] is None else float(case["zref"][m])
            status, n, g = 0, 0, 0.0
            if not (fin(cx) and fin(cy) and fin(zref)):
                status = 4
            else:
                z0 = zref - down
                count = [0] * 128
                for px, py, pz in frame_pts:
                    dx, dy = px - cx, py - cy
                    if dx * dx + dy * dy <= radius * radius:
                        t = (pz - z0) / dz
                        if 0.0 <= t < 128.0:
                            count[int(t)] += 1
                            n += 1
                if n == 0:
                    status = 2
                elif n < min_points:
                    status = 1
                else:
                    k, cum = int(quantile * float(n - 1)), 0
                    for b in range(128):
                        cum += count[b]
                        if cum > k:
                            g = z0 + (float(b) + 0.5) * dz
                            break
            c8 = float(box[m, 8])
            cls = int(c8) if 0.0 <= c8 < float(prior.shape[0]) else 0
            h0 = float(prior[cls, 2])
            h = prior[cls, 2] if vert is None else vert["vert_h"][m]
            src = 0
            if (int(case["flags"][m]) & 1) and status == 0 and fin(h0) and h0 > 0.0:
                if vert is not None and int(vert["vert_status"][m]) == 0:
                    ext = float(vert["vert_z"][m, 1]) - g
                    if lo <= ext / h0 <= hi:
                        src, h, box[m, 2] = 1, ext, g + ext * 0.5
                if src == 0 and zref - g <= h0 + up:
                    src, h, box[m, 2] = 2, h0, g + h0 * 0.5
            out["ground_status"][m], out["ground_n"][m], out["ground_z"][m] = status, n, g
            out["ground_h"][m], out["ground_src"][m], out["ground_zref"][m] = h, src, zref
    return out


def _bits(a):
    return np.ascontiguousarray(a, np.float64).view(np.uint64)


def assert_same(got, exp, what=""):
    """Every output and box to the bit (NaN payloads included: they are only ever copied)."""
    for k in ("ground_status", "ground_src", "ground_n"):
        g, e = np.asarray(got[k]), np.asarray(exp[k])
        assert g.dtype == np.int32 and np.array_equal(g, e), (what, k, np.flatnonzero(g != e)[:8])
    for k in ("ground_z", "ground_h", "ground_zref", "box"):
        g, e = _bits(got[k]).reshape(-1), _bits(exp[k]).reshape(-1)
        assert g.shape == e.shape and np.array_equal(g, e), (what, k, np.flatnonzero(g != e)[:8])


# ------------------------------------------------------------------------------------------------ (d) the batches of the pass tests
SHEET_SLOPE = (0.02, -0.01)                         # the tilt of the added ground sheet, metres per metre along x and y
SHEET_RADII = np.arange(4.0, 26.5, 0.75)            # its rings: none inside 4 m (no member around a box at the origin), none beyond 26 m
SHEET_POINTS = 300


def add_ground_sheet(fr, centre_xy, z):
    """Adds to sweep 0 of the frame (in place, in the sweep's own coordinates) rings of points around centre_xy on the plane
    z + slope . (p - centre): a second, tilted ground 0.15 m under the synthetic one."""
    a = np.linspace(-np.pi, np.pi, SHEET_POINTS, endpoint=False)
    x = np.concatenate([r * np.cos(a + 0.01 * i) for i, r in enumerate(SHEET_RADII)])
    y = np.concatenate([r * np.sin(a + 0.01 * i) for i, r in enumerate(SHEET_RADII)])
    raw = np.asarray(fr.sweeps_raw[0])
    rows = np.zeros((x.size, raw.shape[1]), np.float32)
    rows[:, 0], rows[:, 1], rows[:, 2] = centre_xy[0] + x, centre_xy[1] + y, z + SHEET_SLOPE[0] * x + SHEET_SLOPE[1] * y
    rows[:, 3] = 3.0
    fr.sweeps_raw[0] = np.ascontiguousarray(np.concatenate([raw, rows], 0))


_BATCHES, _PLAIN = {}, {}


def pass_batch(name, first=0, n_frames=2):
    """`nusc` or `waymo`: tests/yaw_fit_pass_cases.py's batch -- parallel lanes, an L vehicle as every frame's last mask -- with the
    ground sheet in every frame (added before the L vehicle, whose mask is kept clear of other rows).  Synthetic frames first ..
    first + n_frames - 1: two frames from 0 unless told otherwise, as yaw_fit_pass_cases.batch takes them."""
    key = name if (first, n_frames) == (0, 2) else (name, first, n_frames)         # pass_plain knows the default batch by its name
    if key in _BATCHES:
        return _BATCHES[key]
    from cm3d_amd import lifting
    from cm3d_amd import synthetic as syn
    from tests import yaw_fit_pass_cases as yc
    ids = range(first, first + n_frames)
    if name == "nusc":
        cfg = syn.config("tiny", n_points=9000, n_masks=20, width=512, height=288, ratio=0.32, max_area=12000.0)
        frames = [syn.make_frame(cfg, i) for i in ids]
        classes = lifting.ClassTable.nuscenes()
        for f in frames:
            add_ground_sheet(f, (0.0, 0.0), -1.84 - 0.15)
        lanes = [yc.parallel_lanes(f.ego_xyz[:2], yc.LANE_YAW[name]) for f in frames]
        heading = [yc.add_l_vehicle(f, yc.LANE_YAW[name]) for f in frames]
    else:
        cfg = syn.config("tiny", n_cams=5, n_points=9000, n_masks=17, width=512, height=288, ratio=0.32, max_area=12000.0)
        frames = [syn.make_waymo_frame(cfg, i) for i in ids]
        classes = lifting.ClassTable.waymo()
        for f in frames:                            # the rows are in the vehicle frame: the sensor stands at x = 0.94, the ground at z = 0
            # (no ego box here: the rows on the vehicle itself go, so that a mask without a box -- centre 0, 0 -- has no member)
            f.sweeps_raw = [np.ascontiguousarray(r[np.hypot(r[:, 0], r[:, 1]) > 3.05]) for r in f.sweeps_raw]
            add_ground_sheet(f, (0.943713, 0.0), -0.15)
        poses = [np.asarray(f.pose, np.float64).reshape(4, 4) for f in frames]
        lanes = [yc.parallel_lanes(P[:2, 3], yc.LANE_YAW[name]) for P in poses]
        heading = [yc.add_l_vehicle(f, yc.LANE_YAW[name], P) for f, P in zip(frames, poses)]
    frame_lane = list(range(n_frames))
    hb = lifting.pack_frames(frames, lanes, frame_lane, classes)
    _BATCHES[key] = SimpleNamespace(name=name, frames=frames, lanes=lanes, frame_lane=frame_lane, hb=hb, classes=classes,
                                    l_masks=[int(m) - 1 for m in hb.mask_off[1:]], l_heading=heading)
    return _BATCHES[key]


def pass_plain(orc, name):
    """The oracle's plain pass over pass_batch(name), once per process (read-only arrays)."""
    if name not in _PLAIN:
        from tests import optin_pass_cases as oc
        b = pass_batch(name)
        _PLAIN[name] = oc._frozen(oc.oracle_batch(orc, b.frames, b.lanes, b.frame_lane, b.hb))
    return _PLAIN[name]


def pass_expected(b, front, box, flags, ground, vertical=None):
    """The host statements on the oracle's cloud (front: an expectation that holds `points`, `pt_off` and the lists) and on a composed
    CPU pass's box and flags: with `vertical` its host statement first, then the ground stage's on what it leaves.  Returns
    (the vertical stage's dict or None, the ground stage's dict)."""
    from cm3d_amd import boxground as bg
    from cm3d_amd import boxvertical as bv
    from tests import optin_pass_cases as oc
    vert, zref = None, None
    if vertical is not None:
        if "cl_off" in front:
            off, xyz = front["cl_off"], front["cl_xyz"]
        else:
            off, xyz = front["hit_off"], oc.hit_xyz_of(b.hb, front)
        xyz = np.asarray(xyz, np.float32)
        xyz4 = np.zeros((len(xyz), 4), np.float32)
        xyz4[:, :xyz.shape[1]] = xyz
        v = vertical
        vert = bv.box_vertical_host(xyz4, off, len(xyz4), box, flags, b.classes.prior_wlh, v.q_bot, v.q_top, v.min_points, v.lo, v.hi)
        box, zref = vert["box"], vert["vert_entry_z"]
    return vert, bg.box_ground_host(front["points"], front["pt_off"], b.hb.mask_off, box, flags, b.classes.prior_wlh, zref=zref, vert=vert,
                                    **ground.params())
