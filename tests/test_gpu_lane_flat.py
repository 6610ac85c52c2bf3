"""GPU: k_lane_nn_grid's flat scan (csrc/boxes.hip, csrc/lane_flat.h) at its seams.  A ring batch's row segments are scanned as one list,
64 positions per round and four rounds per block, so the tables here are built cell by cell: first-batch segments of 0 .. 65 points, block
totals of 63 .. 600 with the nearest point at flat position 0, at T - 1 and at every multiple of 64; exact ties across segments, rounds
and unroll slots; centroids at and beyond the grid's edges; nearest points in rings 3 .. 16+ behind dense full-width rows; waves without a
medoid, with a NaN centroid and live ones in one workgroup; one table (the short header) and three tables, one of them empty.  Tables
of at most about 3 000 points, at most 600 centroids per call; every expectation is oracle.lane_nn, index equal and distance equal bit
for bit."""
import numpy as np
import pytest

from tests import lane_maps as lm
from tests.test_gpu_stage2 import _lane_lookup

pytestmark = pytest.mark.gpu

H = 4.0                  # LG_CELL0: the cell edge of tables this small
# the 16 cells of ring 2 in the order the first batch's flat list meets them: row segments qj - 2 .. qj + 2, columns ascending
RING2 = ([(d, -2) for d in range(-2, 3)] + [(-2, -1), (2, -1), (-2, 0), (2, 0), (-2, 1), (2, 1)] + [(d, 2) for d in range(-2, 3)])
CORNERS = (0, 4, 11, 15)


def _pinned(points, gw, gh):
    """float64 (L, 3) table of the (x, y) rows, shuffled, with two pins that fix the grid to gw x gh cells of 4 m from (0, 0).  Returns the
    table and the new row of every input row."""
    pins = np.array([[0.0, 0.0], [H * gw - 2.0, H * gh - 2.0]])
    xy = np.concatenate([np.asarray(points, np.float64).reshape(-1, 2), pins], 0)
    perm = np.random.default_rng(xy.shape[0]).permutation(xy.shape[0])
    at = np.empty(perm.size, np.int64)
    at[perm] = np.arange(perm.size)
    table = np.concatenate([xy[perm], np.linspace(-3.0, 3.0, xy.shape[0])[:, None]], 1)
    assert lm.grid_geometry(table)[:2] == (0.0, 0.0) and lm.grid_geometry(table)[2] == H and lm.grid_geometry(table)[4:] == (gw | 1, gh)
    return table, at


def _plan(T, specials):
    """Entries for the 16 ring-2 cells (a filler count or "S", a cell with one point) such that the flat list has T points and a
    one-point cell exactly at each position of `specials`.  Corner cells take fillers only: their nearest point is 4 sqrt 2 m from
    the centre cell, further than a neighbour's."""
    entries, pos, todo = [], 0, sorted(specials)
    for idx in range(16):
        if todo and pos == todo[0] and idx not in CORNERS:
            entries.append("S"); pos += 1; todo.pop(0)
        else:
            n = (todo[0] if todo else T) - pos
            entries.append(n); pos += n
    assert not todo and pos == T, (T, specials, entries)
    return entries


def _ring2_block(ci, cj, entries, rng):
    """Points of a block whose centre cell is (ci, cj): cell RING2[i] gets entries[i] filler points in its quarter furthest from the centre
    cell (at least 7 m from every point of it), or for "S" one point where the cell comes nearest (4.2 m).  The 3 x 3 cells inside stay
    empty.  Returns (points, the specials' rows among them, one centroid per special: the point of the centre cell nearest to it)."""
    x0, y0 = H * ci, H * cj
    pts, spec, cent = [], [], []
    for (di, dj), e in zip(RING2, entries):
        cx0, cy0 = x0 + H * di, y0 + H * dj
        if e == "S":
            assert abs(di) != abs(dj)
            sx, sy = min(max(x0 + 2.0, cx0 + 0.1), cx0 + 3.9), min(max(y0 + 2.0, cy0 + 0.1), cy0 + 3.9)
            # (the insets differ along and across: the centroid of cell (-1, -2)'s point must not be as near to cell (-2, -1)'s)
            ix, iy = (0.3, 0.1) if abs(dj) == 2 else (0.1, 0.3)
            spec.append(len(pts)); pts.append((sx, sy))
            cent.append((min(max(sx, x0 + ix), x0 + H - ix), min(max(sy, y0 + iy), y0 + H - iy)))
            continue
        u, far = rng.uniform(0.1, 3.9, e), rng.uniform(0.1, 0.9, e)
        if abs(dj) == 2:
            pts += list(zip(cx0 + u, cy0 + (far if dj < 0 else H - far)))
        else:
            pts += list(zip(cx0 + (far if di < 0 else H - far), cy0 + u))
    return pts, spec, cent


def _z(xy):
    xy = np.asarray(xy, np.float64).reshape(-1, 2)
    return np.concatenate([xy, np.zeros((xy.shape[0], 1))], 1).astype(np.float32)


_OTHER = np.concatenate([np.random.default_rng(77).uniform([10.0, 20.0], [90.0, 70.0], (300, 2)), np.zeros((300, 1))], 1)


def _check(oracle, table, cent, medoid_pos=None):
    """The centroids on `table` alone (n_tables = 1: the short header), then once on each of three tables -- another one, an empty one and
    `table` -- with five frames mapped across them.  Masks without a medoid get (-1, inf), NaN centroids and the empty table (0, inf),
    every other answer is the oracle's.  Returns the oracle's (index, distance) on `table`."""
    K = cent.shape[0]
    assert K * 3 <= 600 and table.shape[0] <= 3100
    mp = np.zeros(K, np.int32) if medoid_pos is None else np.asarray(medoid_pos, np.int32)
    nan = np.isnan(cent[:, :2]).any(1)
    live = (mp >= 0) & ~nan

    def expect(t):
        j, d = np.zeros(K, np.int32), np.full(K, np.inf)
        if t.shape[0]:
            j[live], d[live] = oracle.lane_nn(cent[live], t)
        j[mp < 0] = -1
        return j, d

    def same(idx, dist, j, d, what):
        bad = np.flatnonzero((idx != j) | (dist.view(np.uint64) != d.view(np.uint64)))
        assert bad.size == 0, (what, bad[:8].tolist(), cent[bad[:8]].tolist(), idx[bad[:8]].tolist(), j[bad[:8]].tolist())

    j1, d1 = expect(table)
    idx, dist = _lane_lookup([table], cent, np.zeros(K, np.int32), np.zeros(1, np.int32), mp)
    same(idx, dist, j1, d1, "one table")
    tables = [_OTHER, np.zeros((0, 3)), table]
    frame_lane = np.array([2, 0, 1, 0, 2], np.int32)
    frames = (np.array([1, 3]), np.array([2, 2]), np.array([0, 4]))                  # the frames of each table
    mask_frame = np.concatenate([frames[t][np.arange(K) % 2] for t in range(3)]).astype(np.int32)
    idx, dist = _lane_lookup(tables, np.concatenate([cent] * 3), mask_frame, frame_lane, np.concatenate([mp] * 3))
    for t in range(3):
        j, d = expect(tables[t])
        same(idx[t * K:(t + 1) * K], dist[t * K:(t + 1) * K], j, d, f"table {t} of three")
    return j1, d1


# ------------------------------------------------------------------------------------------------ segment and total seams
def _seam_blocks():
    """(entries, what) of every block: totals T with one-point cells at positions 0, every multiple of 64 and T - 1 (T about 600: over
    two blocks), and two blocks whose five row segments have 0, 1, 12, 13, 63 and 64, 65, 0, 1, 0 points."""
    blocks = []
    for T in (63, 64, 65, 128, 129, 255, 256, 257):
        blocks.append((_plan(T, sorted(set(range(0, T, 64)) | {T - 1})), T))
    blocks.append((_plan(600, range(0, 385, 64)), 600))
    blocks.append((_plan(600, [448, 512, 576, 599]), 600))
    blocks.append(([0, 0, 0, 0, 0, "S", 0, 12, 0, 13, 0, 63, 0, 0, 0, 0], 89))
    blocks.append(([20, 20, 24, 0, 0, 65, 0, 0, 0, 0, "S", 0, 0, 0, 0, 0], 130))
    return blocks


def test_first_batch_segment_and_total_seams(oracle):
    """Twelve blocks of 5 x 5 cells, eight cells apart.  For every one-point cell a centroid whose nearest point it is, at flat position
    0, 64, 128, ... or T - 1 of a list of T = 63 .. 600 points; five more centroids per block up to two cells off its centre."""
    rng = np.random.default_rng(21)
    pts, cent, want = [], [], []
    seg_lens, totals = set(), set()
    for b, (entries, T) in enumerate(_seam_blocks()):
        ci, cj = 4 + 8 * (b % 4), 4 + 8 * (b // 4)
        p, spec, c = _ring2_block(ci, cj, entries, rng)
        assert len(p) == T
        n = [1 if e == "S" else e for e in entries]
        seg_lens |= {sum(n[0:5]), sum(n[5:7]), sum(n[7:9]), sum(n[9:11]), sum(n[11:16])}
        totals.add(T)
        want += [len(pts) + s for s in spec] + [-1] * 5
        cent += c + list(np.array([H * ci + 2.0, H * cj + 2.0]) + rng.uniform(-9.0, 9.0, (5, 2)))
        pts += p
    assert {0, 1, 12, 13, 63, 64, 65} <= seg_lens and {63, 64, 65, 128, 129, 255, 256, 257, 600} <= totals
    table, at = _pinned(pts, 32, 24)
    j, d = _check(oracle, table, _z(cent))
    want = np.array(want)
    sel = want >= 0
    assert sel.sum() == 40 and np.array_equal(j[sel], at[want[sel]]), "the one-point cells are the nearest points of their centroids"
    assert (d[sel] < 2 * H - 1.0).all()                     # ... and settle the search in the first batch


# ------------------------------------------------------------------------------------------------ ties
def test_ties_across_segments_rounds_and_slots(oracle):
    """Exact ties (coordinates on a 0.25 m lattice): two points in different row segments; two points of one segment 64, 65 and 192
    flat positions apart (the centre cell's points lie between them, further away), the smaller index at the later position; points
    with identical coordinates.  np.argmin's first minimum every time."""
    rng = np.random.default_rng(22)
    pts, cent, pair = [], [], []

    def corners(ci, cj, n):
        u, v = rng.uniform(0.05, 0.2, n), rng.uniform(0.05, 0.2, n)
        return list(zip(H * ci + np.where(rng.random(n) < 0.5, u, H - u), H * cj + np.where(rng.random(n) < 0.5, v, H - v)))

    for b, n in enumerate((63, 64, 191)):                   # same segment: cells (ci - 1, cj), (ci, cj) x n, (ci + 1, cj)
        ci, cj = 4 + 8 * b, 4
        first, later = (H * ci - 0.25, H * cj + 2.0), (H * ci + 4.25, H * cj + 2.0)
        pair.append((len(pts) + 1, len(pts)))               # (first-visited row, later-visited row): the later one comes first here
        pts += [later, first] + corners(ci, cj, n)
        cent.append((H * ci + 2.0, H * cj + 2.0))
    ci, cj = 4, 12                                          # different segments: rows cj - 1 and cj + 1
    pair.append((len(pts) + 1, len(pts)))
    pts += [(H * ci + 2.0, H * cj + 4.25), (H * ci + 2.0, H * cj - 0.25)] + corners(ci, cj, 5)
    cent.append((H * ci + 2.0, H * cj + 2.0))
    ci, cj = 12, 12                                         # duplicates: three rows with the same coordinates, two more one cell on
    dup0 = len(pts)
    pts += [(H * ci + 1.0, H * cj + 1.5)] * 3 + [(H * ci + 5.0, H * cj + 1.5)] * 2 + corners(ci, cj + 1, 7)
    cent += [(H * ci + 2.0, H * cj + 2.0), (H * ci + 1.0, H * cj + 1.5), (H * ci + 3.0, H * cj + 1.5), (H * ci + 3.75, H * cj + 0.5)]
    # keep the rows in this order (the index decides the ties): pins last, no shuffle
    xy = np.concatenate([np.array(pts), [[0.0, 0.0], [H * 25 - 2.0, H * 17 - 2.0]]], 0)
    table = np.concatenate([xy, np.linspace(-3.0, 3.0, xy.shape[0])[:, None]], 1)
    assert lm.grid_geometry(table)[4:] == (25, 17)
    cz = _z(cent)
    j, d = _check(oracle, table, cz)
    for k, (first_visited, later_visited) in enumerate(pair):
        assert later_visited < first_visited and j[k] == later_visited and d[k] == 2.25, (k, j[k], d[k])
        t32 = table.astype(np.float32).astype(np.float64)
        assert np.hypot(*(t32[first_visited, :2] - cz[k, :2])) == np.hypot(*(t32[later_visited, :2] - cz[k, :2]))
    assert j[4] == dup0 and j[5] == dup0 and d[5] == 0.0 and j[6] == dup0 and d[6] == 2.0 and j[7] == dup0 + 3


# ------------------------------------------------------------------------------------------------ clipping and degenerate waves
def _scatter_table():
    """1 500 points over 100 m x 100 m (a 25 x 26-cell grid), a crowded cell in one corner and one on an edge."""
    rng = np.random.default_rng(23)
    xy = np.concatenate([rng.uniform(0.0, 100.0, (1500, 2)), rng.uniform([0.2, 0.2], [3.8, 3.8], (70, 2)),
                         rng.uniform([48.2, 96.2], [51.8, 99.8], (30, 2)), [[0.0, 0.0], [100.0, 100.0]]], 0)
    return np.concatenate([xy, rng.uniform(-3.0, 3.0, (xy.shape[0], 1))], 1)


def _edge_centroids(table):
    """Centroids in the four corner cells, in cells along each edge, 1, 2 and 3 cells outside the grid on each side (and diagonally off
    each corner), and further out than LG_MAX_RINGS cells on each side: the exact scan of the whole table."""
    x0, y0, h, _, gw, gh = (float(v) for v in lm.grid_geometry(table))
    rng = np.random.default_rng(24)
    cells = [(0, 0), (gw - 1, 0), (0, gh - 1), (gw - 1, gh - 1)]
    cells += [(i, 0) for i in (3, 12, 20)] + [(i, gh - 1) for i in (3, 12, 20)] + [(0, j) for j in (3, 12, 20)] + [(gw - 1, j) for j in (3, 12, 20)]
    for k in (1, 2, 3):
        cells += [(-k, 7), (gw - 1 + k, 15), (9, -k), (17, gh - 1 + k), (-k, -k), (gw - 1 + k, gh - 1 + k), (-k, gh - 1 + k), (gw - 1 + k, -k)]
    far = lm.LG_MAX_RINGS + 3
    cells += [(-far, 5), (gw + far, 11), (6, -far), (13, gh + far), (-far - 40, -far - 9)]
    c = np.array([(x0 + (i + u) * h, y0 + (j + v) * h) for i, j in cells for u, v in rng.uniform(0.05, 0.95, (3, 2))])
    return _z(c), len(cells) - 5


def test_centroids_at_and_beyond_the_grid_edges(oracle):
    """The first batch is not the 5 x 5 cells here: clipped at corners and edges, and starting at ring 1, 2 or 3 for a centroid outside
    the grid; beyond LG_MAX_RINGS cells the whole table is scanned."""
    table = _scatter_table()
    cent, n_ring = _edge_centroids(table)
    j, d = _check(oracle, table, cent)
    assert (d[3 * n_ring:] > lm.LG_MAX_RINGS * H).all() and (d[:3 * n_ring] < 30.0).all()


def test_degenerate_and_live_waves_share_workgroups(oracle):
    """A workgroup is four waves, a wave one mask: masks without a medoid, NaN centroids and live ones interleaved in every group of four,
    in rotating places."""
    table = _scatter_table()
    rng = np.random.default_rng(25)
    K = 96
    cent = _z(rng.uniform(-10.0, 110.0, (K, 2)))
    kind = np.array([(0, 1, 2, 2), (2, 0, 2, 1), (1, 2, 0, 2), (2, 2, 1, 0), (0, 0, 1, 2), (2, 1, 1, 0)] * 4).reshape(-1)      # 0: no medoid, 1: NaN
    cent[kind == 1, rng.integers(0, 2, int((kind == 1).sum()))] = np.nan
    mp = np.where(kind == 0, -1, 5).astype(np.int32)
    j, d = _check(oracle, table, cent, mp)
    assert (j[kind == 0] == -1).all() and (j[kind == 1] == 0).all() and np.isinf(d[kind != 2]).all() and np.isfinite(d[kind == 2]).all()


# ------------------------------------------------------------------------------------------------ later batches
def test_nearest_point_in_far_rings_behind_dense_rows(oracle):
    """A 51 x 50-cell table that is empty but for four full-width rows of ten points per cell (rows 45 .. 48) and a few points in column
    9.  Centroids 3, 5, 6 and 9 rows below the wall: the first batch is an empty list (T = 0), the batch of rings 3 .. 5 a step of 330
    points (more than four rounds), the nearest point in the batch's full-width rows.  Centroids 16 and more cells from every point: the
    batch of rings 16 .. 24 has 80 segments, two steps, the first of more than 1 000 points; for those in row 24 the nearest point is in
    column 9, in a side piece of the second step."""
    rng = np.random.default_rng(26)
    cells = [(i, j) for j in range(45, 49) for i in range(51)]
    pts = [(H * i + u, H * j + v) for i, j in cells for u, v in rng.uniform(0.1, 3.9, (10, 2))]
    side0 = len(pts)
    pts += [(H * 9 + u, H * j + v) for j in range(32, 36) for u, v in rng.uniform(0.1, 3.9, (2, 2))]
    table, at = _pinned(pts, 51, 50)
    rows = np.array([42] * 3 + [40] * 3 + [39] * 3 + [36] * 3 + [29] * 3 + [24] * 4)
    cols = np.array([25] * 12 + [40] * 3 + [25] * 4)
    cent = np.array([(H * c + u, H * r + v) for c, r, (u, v) in zip(cols, rows, rng.uniform(0.1, 3.9, (len(rows), 2)))])
    j, d = _check(oracle, table, _z(cent))
    t32 = table.astype(np.float32)
    ring = np.maximum(np.abs(np.floor(t32[j, 0] / H) - cols), np.abs(np.floor(t32[j, 1] / H) - rows)).astype(int)
    assert {3, 5, 6, 9} <= set(ring.tolist()) and (ring[12:] >= 16).all() and (ring[12:] <= 24).all(), ring.tolist()
    in_side = np.isin(j, at[side0:side0 + 8])
    assert in_side[15:].all() and not in_side[:15].any(), (j.tolist(), in_side.tolist())
    # the side points lie 8 rows and more above their centroids: segments 64 .. 79 of the batch (rows qj + 8 .. qj + 15 of its side pieces)
    assert ((np.floor(t32[j[in_side], 1] / H) - rows[in_side]) >= 8).all()


# ------------------------------------------------------------------------------------------------ a map regime at this size
def test_small_city_map_regime(oracle):
    """tests/lane_maps.py's street map at 100 m x 80 m (lanes on a 0.5 m lattice, junction connectors, shuffled rows) with its crafted
    centroids: near and on lane points, exact ties, junctions, cell boundaries to the ulp, the park, the far rings, the exact scan."""
    m = lm.city_map(origin=(30.0, 45.0), extent=(100.0, 80.0), block=(50.0, 80.0), lanes_per_dir=1, park=(52.0, 2.0, 98.0, 78.0), seed=3)
    assert 1500 < m.lane.shape[0] <= 3100, m.lane.shape
    sets = lm.crafted_centroids(m, seed=1, n=(50, 25, 25, 6, 10, 10, 20))
    cent = np.concatenate([v[:30] for v in sets.values()], 0)
    assert cent.shape[0] <= 200 and len(sets["tie"]) > 0
    j, d = _check(oracle, m.lane, cent)
    assert d.max() > lm.LG_MAX_RINGS * H and d.min() == 0.0
