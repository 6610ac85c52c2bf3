"""Inputs of the ground strip's tests (cm3d_ground_grid, cm3d_ground_strip; numpy and, for the clouds, the CPU oracle's sweep
preparation): (a) small frames built to sit on the rule's edges -- cell edges, the z window, counts and ranks, the seams of the kernel's
16 x 16-cell tiles, origins, rows and frames, and lists on the threshold, on the MIN_KEEP rule and across the compaction's 64-position
chunks --, (b) three frames of a bumpy ground with two sweeps of their own transforms and lists drawn from the cloud -- and a scalar
loop written apart from the host statement (one point at a time, Python floats) that both the host statement and the device are held
against.

A case holds the raw rows (five floats each, sensor frame) of its sweeps with their transforms, as tests/box_ground_cases.py does:
cloud(), raw_layouts() and sweep_xf() there serve these cases too.  Every frame's rows are padded with NaN rows to a multiple of four."""
import math

import numpy as np

from tests.box_ground_cases import IDENTITY, _dn, _up, _xf, cloud, raw_layouts, sweep_xf  # noqa: F401  (re-exported)

CELLS, BINS, HALF = 64, 64, 32                      # include/cm3d_hip.h: CM3D_GROUND_GRID_CELLS, CM3D_GROUND_GRID_BINS
N_CELLS = CELLS * CELLS
DEFAULTS = dict(cell=2.0, down=4.0, up=4.0, quantile=0.1, min_points=8, margin=0.3, min_keep=5)
DZ = 0.125                                          # (4 + 4) / 64: exact
f32 = np.float32


def cell_index(iu, iv):
    return (iv + HALF) * CELLS + (iu + HALF)


def grid_params(run):
    p = dict(DEFAULTS, **run)
    return {k: p[k] for k in ("cell", "down", "up", "quantile", "min_points")}


def strip_params(run):
    p = dict(DEFAULTS, **run)
    return {k: p[k] for k in ("cell", "margin", "min_keep")}


class _Builder:
    """Frames of sweeps, origins and lists -> a case."""

    def __init__(self, name, halfw):
        self.name, self.halfw = name, float(f32(halfw))
        self.sweeps, self.fso, self.origin = [], [0], []
        self.lists, self.names, self.mask_frame = [], [], []

    def frame(self, sweeps, origin, lists=()):
        """sweeps: [(points (n, 3), xf (24,))]; the frame's last sweep gets its NaN padding.  lists: [(name, points (n, 3))]."""
        n = sum(len(p) for p, _ in sweeps)
        pad = (-n) % 4
        for i, (p, xf) in enumerate(sweeps):
            rows = np.zeros((len(p), 5), np.float32)
            rows[:, :3] = np.asarray(p, np.float32).reshape(-1, 3)
            rows[:, 3], rows[:, 4] = 7.0, np.arange(len(p)) % 32
            if i == len(sweeps) - 1 and pad:
                rows = np.concatenate([rows, np.full((pad, 5), np.nan, np.float32)], 0)
            self.sweeps.append((rows, np.asarray(xf, np.float32)))
        assert not (pad and not sweeps)
        f = len(self.origin)
        self.fso.append(len(self.sweeps))
        self.origin.append(np.asarray(origin, np.float64))
        for name, p in lists:
            self.add_list(name, p, f)

    def add_list(self, name, p, frame):
        self.names.append(name), self.lists.append(np.asarray(p, np.float32).reshape(-1, 3)), self.mask_frame.append(frame)

    def case(self, rng, runs, **more):
        row_off = np.concatenate([[0], np.cumsum([len(s[0]) for s in self.sweeps])]).astype(np.int32)
        n = [len(p) for p in self.lists]
        xyz = np.zeros((sum(n), 4), np.float32)
        if sum(n):
            xyz[:, :3] = np.concatenate(self.lists, 0)
        xyz[:, 3] = rng.uniform(0, 255, sum(n)).astype(np.float32)             # (the intensity travels with the point)
        return dict(name=self.name, names=self.names, sweeps=self.sweeps, sweep_row_off=row_off, frame_sweep_off=np.array(self.fso, np.int32),
                    halfw=self.halfw, origin=np.array(self.origin, np.float64).reshape(-1, 3), hit_xyz=xyz,
                    hit_idx=rng.integers(0, 1 << 20, sum(n)).astype(np.int32), hit_off=np.concatenate([[0], np.cumsum(n)]).astype(np.int32),
                    mask_frame=np.array(self.mask_frame, np.int32), runs=runs, **more)


def _stack(x, y, zs):
    zs = np.asarray(zs, np.float64).reshape(-1)
    return np.stack([np.full(zs.size, x), np.full(zs.size, y), zs], 1)


# ------------------------------------------------------------------------------------------------ (a) the rule's edges
O0 = np.array([10.0, -6.0, 1.0])                    # frame 0's origin: z0 = -3, the window ends at 5
G_CELL, G_BIN = (5, 5), 8                           # the cell the lists stand in: ten members in bin 8
G = -3.0 + (G_BIN + 0.5) * DZ                       # its estimate, -1.9375: exact
T25 = G + 0.25                                      # g + MARGIN of the run with margin 0.25: -1.6875, a float32


def edges_case():
    """Frame 0 (identity transform, so the cloud is the rows to the bit; ego box 1.5 m): one cell per edge.  Frame 1: origin 0, 0 and
    -0.0 coordinates.  Frame 2: a non-finite origin.  Frame 3: frame 0's origin, other points, no list.  Frame 4: lists, no sweep.
    Frame 5: lists, a sweep without rows."""
    rng = np.random.default_rng(3001)
    b = _Builder("edges", 1.5)
    pts, cells = [], {}
    at = lambda iu, iv, fx=0.5, fy=0.5, o=O0: (o[0] + (iu + fx) * 2.0, o[1] + (iv + fy) * 2.0)
    zb = lambda bins, frac=0.5, o=O0: (o[2] - 4.0) + (np.asarray(bins, np.float64) + frac) * DZ

    def add(name, iu, iv, p, n, b_star=None):
        cells[name] = (cell_index(iu, iv), n, b_star)
        pts.append(np.asarray(p, np.float64).reshape(-1, 3))
    eight = lambda b0: zb(b0 + np.arange(8) % 2)
    # a point on a cell edge belongs to the cell that starts there, the next float32 below it to the cell before
    add("edge_x_on", 3, 0, _stack(16.0, at(0, 0)[1], eight(20)), 8, 20)
    add("edge_x_below", 2, 0, _stack(_dn(16.0), at(0, 0)[1], eight(22)), 8, 22)
    add("edge_y_on", 0, -3, _stack(at(0, 0)[0], -12.0, eight(24)), 8, 24)
    add("edge_y_below", 0, -4, _stack(at(0, 0)[0], _dn(-12.0), eight(26)), 8, 26)
    # the grid's ends: iu, iv = -33 and 32 are outside, -32 and 31 the first and last cells
    for i, (iu, inside) in enumerate(((-33, False), (-32, True), (31, True), (32, False))):
        p = _stack(at(iu, 7)[0], at(iu, 7)[1], eight(28 + 2 * i))
        add(f"iu_{iu}", iu, 7, p, 8, 28 + 2 * i) if inside else pts.append(p)
        p = _stack(at(8, iu)[0], at(8, iu)[1], eight(36 + 2 * i))
        add(f"iv_{iu}", 8, iu, p, 8, 36 + 2 * i) if inside else pts.append(p)
    # u = -0.25: floor gives -1 where truncation would give 0
    add("negative_fraction", -1, -1, _stack(O0[0] - 0.5, O0[1] - 0.5, eight(12)), 8, 12)
    # the window: z0 itself (bin 0), one float32 below (out), a bin edge (bin 10, not 9), the window's end (out), one below it (bin 63)
    add("window", -6, -6, _stack(*at(-6, -6), [-3.0] * 3 + [_dn(-3.0)] * 4 + [-3.0 + 10 * DZ] * 2 + [5.0] * 5 + [_dn(5.0)] * 3), 8, 0)
    add("few_7", -8, -6, _stack(*at(-8, -6), zb(np.arange(7) % 2 + 5)), 7)
    add("enough_8", -10, -6, _stack(*at(-10, -6), eight(5)), 8, 5)
    # k = (int)(0.1 * 20) = 2: the third point in ascending order -- the last of bin 20's three, or the first of bin 25 behind bin 20's two
    add("k_last_of_bin", -12, -6, _stack(*at(-12, -6), zb([20] * 3 + [25] * 18)), 21, 20)
    add("k_first_of_next", -14, -6, _stack(*at(-14, -6), zb([20] * 2 + [25] * 19)), 21, 25)
    add("all_bin_0", -16, -6, _stack(*at(-16, -6), zb([0] * 12, rng.uniform(0.05, 0.95, 12))), 12, 0)
    add("all_bin_63", -18, -6, _stack(*at(-18, -6), zb([63] * 12, rng.uniform(0.05, 0.95, 12))), 12, 63)
    # both sides of every seam of the kernel's 16 x 16-cell tiles: cells 15/16, 31/32, 47/48 of 0 .. 63, in x and in y
    for j, i in enumerate((15, 16, 31, 32, 47, 48)):
        add(f"seam_x_{i}", i - HALF, 12, _stack(*at(i - HALF, 12), eight(40 + 2 * j)), 8, 40 + 2 * j)
        add(f"seam_y_{i}", 13, i - HALF, _stack(*at(13, i - HALF), eight(50 + 2 * j)), 8, 50 + 2 * j)
    # the ego box: rows at |x|, |y| < 1.5 are dropped (5 of them), those at x = 1.6 in the same cell stay
    add("ego_box", -5, 3, np.concatenate([_stack(1.6, 0.5, eight(7)), _stack(0.5, 0.5, zb([7] * 5))]), 8, 7)
    add("non_finite_rows", 9, -9, np.concatenate([_stack(*at(9, -9), eight(9)), [[np.nan, at(9, -9)[1], 0.0], [at(9, -9)[0], np.inf, 0.0],
                                                                               [*at(9, -9), np.nan], [*at(9, -9), -np.inf]]]), 8, 9)
    add("G", *G_CELL, _stack(*at(*G_CELL), zb([G_BIN] * 10, rng.uniform(0.05, 0.95, 10))), 10, G_BIN)
    gx, gy = at(*G_CELL)
    low = lambda n: rng.uniform(-2.9, -2.0, n)       # below G + any margin of the runs
    high = lambda n: rng.uniform(0.0, 3.0, n)
    in_g = lambda zs: np.stack([gx + rng.uniform(-0.9, 0.9, len(zs)), gy + rng.uniform(-0.9, 0.9, len(zs)), zs], 1)
    t30 = float(f32(G + 0.3))
    lists = [("threshold_025", in_g(np.array([_dn(T25), T25, _up(T25)] + list(high(5))))),
             ("threshold_03", in_g(np.array([_dn(t30), t30, _up(t30)] + list(high(5))))),
             ("outside_and_no_estimate", np.concatenate([_stack(O0[0] + 70.0, O0[1], low(3)), _stack(*at(-8, -6), low(3)),
                                                         _stack(O0[0], O0[1] - 64.5, low(2))])),
             ("kept_4", in_g(np.concatenate([high(4), low(3)]))), ("kept_5", in_g(np.concatenate([low(3), high(5)]))),
             ("all_ground", in_g(low(9))), ("empty", np.zeros((0, 3))), ("nothing_to_drop", in_g(high(7))),
             ("non_finite", np.concatenate([in_g(high(5)), [[np.nan, gy, -2.5], [gx, np.inf, -2.5], [gx, gy, np.nan], [gx, gy, -np.inf],
                                                            [gx, gy, np.inf]], in_g(low(2))]))]
    for n in (1, 63, 64, 65, 257, 300):
        z = np.where(rng.random(n) < 0.4, low(n), high(n))
        lists.append((f"len_{n}", in_g(z)))
    order = rng.permutation(sum(len(p) for p in pts))                          # the order of arrival is not the cells' order
    b.frame([(np.concatenate(pts, 0)[order], IDENTITY)], O0, lists)
    b.add_list("frame_99", in_g(np.concatenate([low(4), high(6)])), 99)
    b.add_list("frame_minus_1", in_g(np.concatenate([low(4), high(6)])), -1)
    # frame 1: the origin 0, 0 and -0.0 coordinates (u = -0.0: cell 0, not -1)
    O1 = np.array([0.0, 0.0, 0.5])
    b.frame([(np.concatenate([_stack(-0.0, 2.5, zb(np.arange(9) % 2 + 10, o=O1)), _stack(2.5, -0.0, zb(np.arange(8) % 2 + 14, o=O1))]), IDENTITY)], O1,
            [("minus_zero", np.concatenate([_stack(-0.0, 2.5, [-3.4, -3.3, 1.0, 1.5]), _stack(2.5, -0.0, [-3.4, 1.0, 1.2, 1.4])]))])
    frame1 = {"minus_zero_x": (cell_index(0, 1), 9, 10), "minus_zero_y": (cell_index(1, 0), 8, 14)}
    # frame 2: a non-finite origin -- no estimate anywhere, every count 0, nothing is ground
    b.frame([(_stack(3.0, 3.0, zb(np.arange(20) % 4)), IDENTITY)], [np.nan, 0.0, 1.0], [("nan_origin", _stack(3.0, 3.0, np.linspace(-2.9, 2.0, 8)))])
    # frame 3: frame 0's origin and enough_8's cell with other bins; no list
    b.frame([(_stack(*at(-10, -6), eight(33)), IDENTITY)], O0)
    b.frame([], O0, [("frame_without_sweeps", in_g(np.concatenate([low(4), high(6)])))])
    b.frame([(np.zeros((0, 3)), IDENTITY)], O0, [("sweep_without_rows", in_g(np.concatenate([low(4), high(6)])))])
    b.frame([(_stack(3.0, 3.0, zb(np.arange(20) % 4)), IDENTITY)], [0.0, 0.0, np.inf], [("inf_origin_z", _stack(3.0, 3.0, np.linspace(-2.9, 2.0, 8)))])
    # (status, dropped) per list at the defaults, and with margin 0.25 where that differs
    lists_expect = dict(threshold_03=None, threshold_025=None, outside_and_no_estimate=(0, 0), kept_4=(1, 0), kept_5=(0, 3), all_ground=(1, 0),
                        empty=(2, 0), nothing_to_drop=(0, 0), non_finite=(0, 2), len_1=(1, 0), frame_99=(0, 0), frame_minus_1=(0, 0),
                        minus_zero=(0, 3), nan_origin=(0, 0), frame_without_sweeps=(0, 0), sweep_without_rows=(0, 0), inf_origin_z=(0, 0))
    runs = [{}, dict(margin=0.25), dict(min_points=1), dict(min_points=11), dict(quantile=0.0), dict(quantile=1.0), dict(min_keep=1),
            dict(min_keep=6), dict(margin=-0.5), dict(cell=_dn(2.0)), dict(down=3.0, up=1.0)]
    return b.case(rng, runs, cells=cells, frame1_cells=frame1, lists_expect=lists_expect, same_xy_frame=(3, cell_index(-10, -6), 8, 33))


# ------------------------------------------------------------------------------------------------ (b) bumpy ground, two sweeps, drawn lists
def many_case():
    """Three frames of 3000, 1500 and 600 rows; frame 0 has two sweeps with transforms of their own.  A ground sheet with bumps and tall
    points, an ego box of sqrt(2.3) m; every list holds the rows within a radius of a drawn row (list_rows: indices into the batch's
    rows, the coordinates come from the cloud), so every list point is a point of its frame's cloud."""
    rng = np.random.default_rng(3002)
    b = _Builder("many", math.sqrt(2.3))
    list_rows, first = [], 0
    for f, (n_lists, n_sweeps, n_rows) in enumerate(((24, 2, 3000), (12, 1, 1499), (3, 1, 600))):
        centre = np.array([600.0, 1600.0, 1.0]) + rng.normal(0, 50, 3) * [1, 1, 0.01]
        sweeps, approx = [], []
        for s in range(n_sweeps):
            n = n_rows // n_sweeps
            p = np.stack([rng.uniform(-12, 12, n), rng.uniform(-12, 12, n), -1.84 + rng.normal(0, 0.04, n)], 1)
            tall = rng.random(n) < 0.3
            p[tall, 2] += rng.uniform(0.0, 3.0, int(tall.sum()))
            xf = _xf(rng, centre + [0.4 * s, 0.0, 0.0])
            sweeps.append((p, xf))
            x64 = xf.astype(np.float64)
            approx.append((p @ x64[0:9].reshape(3, 3).T + x64[9:12]) @ x64[12:21].reshape(3, 3).T + x64[21:24])
        approx = np.concatenate(approx, 0)
        b.frame(sweeps, centre)
        for i in range(n_lists):
            c = approx[rng.integers(0, len(approx))]
            near = np.flatnonzero(np.hypot(approx[:, 0] - c[0], approx[:, 1] - c[1]) < rng.uniform(1.0, 5.0))
            list_rows.append(first + near), b.names.append(f"f{f}_m{i}"), b.mask_frame.append(f), b.lists.append(np.zeros((len(near), 3)))
        first += n_rows + (-n_rows) % 4
    return b.case(rng, [{}, dict(cell=1.0, quantile=0.5, min_points=3, margin=0.1, min_keep=2), dict(min_points=1000)], list_rows=list_rows)


def all_cases():
    return [edges_case(), many_case()]


def lists(case, points):
    """(hit_xyz (n, 4) float32, hit_idx, hit_off, mask_frame) of the case; `points`: its cloud (drawn lists take their rows from it --
    rows the preparation dropped are NaN there and stay in the list: a non-finite point is never ground)."""
    xyz = case["hit_xyz"].copy()
    if "list_rows" in case:
        xyz[:, :] = np.asarray(points, np.float32)[np.concatenate(case["list_rows"])]
    return xyz, case["hit_idx"], case["hit_off"], case["mask_frame"]


# ------------------------------------------------------------------------------------------------ the scalar loop
def _fin(v):
    return not (math.isnan(v) or math.isinf(v))


def _cell(px, py, ox, oy, C):
    """The rule's cell of a point, or None outside the grid."""
    if not (_fin(px) and _fin(py) and _fin(ox) and _fin(oy)):
        return None
    iu, iv = math.floor((px - ox) / C), math.floor((py - oy) / C)
    if -32 <= iu < 32 and -32 <= iv < 32:
        return (iv + 32) * 64 + (iu + 32)
    return None


def loop_grid(points, pt_off, origin, cell=2.0, down=4.0, up=4.0, quantile=0.1, min_points=8):
    """The grid of include/cm3d_hip.h, one point at a time, in Python floats (IEEE doubles, every operation rounded)."""
    pts = np.asarray(points, np.float32)[:, :3].astype(np.float64).tolist()
    F = len(pt_off) - 1
    grid_z, grid_n = np.full((F, N_CELLS), np.nan), np.zeros((F, N_CELLS), np.int32)
    dz = (down + up) / 64.0
    for f in range(F):
        ox, oy, oz = (float(v) for v in origin[f])
        if not (_fin(ox) and _fin(oy) and _fin(oz)):
            continue
        count = {}
        for px, py, pz in pts[int(pt_off[f]):int(pt_off[f + 1])]:
            if not _fin(pz):
                continue
            c = _cell(px, py, ox, oy, cell)
            if c is None:
                continue
            t = (pz - (oz - down)) / dz
            if 0.0 <= t < 64.0:
                count.setdefault(c, [0] * 64)[int(t)] += 1
        for c, bins in count.items():
            n = sum(bins)
            grid_n[f, c] = n
            if n >= min_points:
                k, cum = int(quantile * float(n - 1)), 0
                for b in range(64):
                    cum += bins[b]
                    if cum > k:
                        grid_z[f, c] = (oz - down) + (float(b) + 0.5) * dz
                        break
    return grid_z, grid_n


def loop_strip(hit_xyz, hit_off, mask_frame, origin, grid_z, cell=2.0, margin=0.3, min_keep=5):
    """The strip of include/cm3d_hip.h, one list point at a time: (keep over all positions, gs_status, gs_dropped)."""
    xyz = np.asarray(hit_xyz, np.float32)[:, :3].astype(np.float64).tolist()
    M, F = len(hit_off) - 1, len(origin)
    keep, status, dropped = np.ones(int(hit_off[-1]), bool), np.zeros(M, np.int32), np.zeros(M, np.int32)
    for m in range(M):
        o, e, f = int(hit_off[m]), int(hit_off[m + 1]), int(mask_frame[m])
        if e == o:
            status[m] = 2
            continue
        ground = []
        for px, py, pz in xyz[o:e]:
            is_ground = False
            if 0 <= f < F and _fin(pz):
                c = _cell(px, py, float(origin[f][0]), float(origin[f][1]), cell)
                if c is not None:
                    g = float(grid_z[f][c])
                    is_ground = (not math.isnan(g)) and pz < g + margin
            ground.append(is_ground)
        kept = len(ground) - sum(ground)
        if kept < min_keep:
            status[m] = 1
        else:
            keep[o:e] = [not g for g in ground]
            dropped[m] = sum(ground)
    return keep, status, dropped


def expected(case, points, pt_off, run):
    """The host statements on a case's cloud: a dict of grid_z, grid_n and the gs_* arrays the device is held against."""
    from cm3d_amd import groundstrip as gs
    grid_z, grid_n = gs.ground_grid_host(points, pt_off, case["origin"], **grid_params(run))
    xyz, idx, off, mf = lists(case, points)
    gs_off, gs_tile_off, keep, status, dropped = gs.strip_lists(off, xyz, mf, case["origin"], grid_z, **strip_params(run))
    return dict(grid_z=grid_z, grid_n=grid_n, gs_off=gs_off, gs_tile_off=gs_tile_off, gs_status=status, gs_dropped=dropped, gs_xyz=xyz[keep],
                gs_idx=idx[keep], keep=keep)


def bits(a):
    return np.ascontiguousarray(a, np.float64).view(np.uint64)
