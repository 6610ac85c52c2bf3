"""City-scale lane maps and crafted centroids for the stage-2 tests (csrc/boxes.hip).

`synthetic.make_lane_table` draws tables of 50-450 m: at that size the lane grid keeps its preferred 4 m cell and the
search never leaves its first rings.  A nuScenes map location holds every lane and connector of a whole city district,
discretised at 0.5 m (nusc_io.load_lane_points): kilometres across and a few 10^5 points.  `city_map` builds tables
like that, deterministically from its arguments:

* a street grid of two-way roads, `lanes_per_dir` lanes per direction, 3.5 m apart, points every 0.5 m;
* a junction box at every crossing, filled with straight, left- and right-turn connectors from every incoming lane
  (one grown-grid cell there holds hundreds of points); a connector starts on the last point of its incoming lane
  and ends on the first point of its outgoing lane, so those rows are duplicated, as in discretize_lanes' output;
* one diagonal avenue and one ring road (points off the axes);
* a lane-free park a few hundred metres across;
* the lanes in shuffled order (the row index says nothing about the position).

Rows are float64 (x, y, yaw) like discretize_lanes.  Axis-aligned lanes lie on a 0.25 m lattice, so points and the
centroids placed between them are exact in float32: the equidistant ties below are exact ties.

`crafted_centroids` places float32 centroids where the grid search of k_lane_nn_grid is delicate.  Its cell-boundary
set needs the grid the build kernel will make; `grid_geometry` recomputes it on the host with the kernel's float32
arithmetic (k_lane_grid_build: bounding box, the cell-size growth loop, the bin expression).

Left out on purpose: NaN lane points.  The grid skips them while the reference's np.argmin over a row with a NaN
distance returns the NaN's index, so the two differ by design; no table here holds one.
"""
import functools
from dataclasses import dataclass, field

import numpy as np

# mirrors of csrc/boxes.hip
LG_MAX_CELLS = 32768
LG_CELL0 = 4.0
LG_MAX_RINGS = 64
LG_BIG_CELL = 12

STEP = 0.5          # discretisation of the lanes [m]
LANE_W = 3.5        # lateral distance of neighbouring lanes [m]
_DIRS = [(1, 0), (0, 1), (-1, 0), (0, -1)]     # E, N, W, S


@dataclass
class CityMap:
    lane: np.ndarray                  # (L, 3) float64 x, y, yaw
    origin: tuple
    extent: tuple
    park: tuple                       # (x0, y0, x1, y1): no lane point inside
    junctions: np.ndarray             # (J, 2) junction centres
    junction_half: float
    ties: np.ndarray = field(default=None)      # (T, 2) float64 centroids equidistant from >= 2 lane points


def _right(d):
    return (d[1], -d[0])


def _line(p0, d, n):
    """n points from p0 along the unit axis vector d, STEP apart (exact on the lattice)."""
    k = np.arange(n, dtype=np.float64) * STEP
    yaw = np.arctan2(float(d[1]), float(d[0]))
    return np.stack([p0[0] + k * d[0], p0[1] + k * d[1], np.full(n, yaw)], 1)


def _bezier(p0, c, p1):
    """Quadratic Bezier p0 -> p1 with control c, resampled at STEP arc length; yaw along the tangent."""
    t = np.linspace(0.0, 1.0, 400)[:, None]
    p0, c, p1 = (np.asarray(v, np.float64) for v in (p0, c, p1))
    P = (1 - t) ** 2 * p0 + 2 * (1 - t) * t * c + t ** 2 * p1
    s = np.concatenate([[0.0], np.cumsum(np.hypot(*np.diff(P, axis=0).T))])
    n = max(2, int(np.floor(s[-1] / STEP)) + 1)
    sq = np.linspace(0.0, s[-1], n)
    tq = np.interp(sq, s, t[:, 0])[:, None]
    Q = (1 - tq) ** 2 * p0 + 2 * (1 - tq) * tq * c + tq ** 2 * p1
    D = 2 * (1 - tq) * (c - p0) + 2 * tq * (p1 - c)
    Q[0], Q[-1] = p0, p1                   # the end points exactly (shared with the lanes they join)
    return np.concatenate([Q, np.arctan2(D[:, 1], D[:, 0])[:, None]], 1)


def _arc(cx, cy, r, a0, a1, ccw):
    n = max(2, int(abs(a1 - a0) * r / STEP))
    a = np.linspace(a0, a1, n, endpoint=False)
    yaw = a + (np.pi / 2 if ccw else -np.pi / 2)
    return np.stack([cx + r * np.cos(a), cy + r * np.sin(a), np.arctan2(np.sin(yaw), np.cos(yaw))], 1)


def city_map(origin=(30.0, 45.0), extent=(2000.0, 2000.0), block=(160.0, 150.0), lanes_per_dir=2, park=None,
             seed=0, shift=(0.0, 0.0)) -> CityMap:
    """One map location.  origin, extent, block: multiples of 0.5 m; park (x0, y0, x1, y1) relative to the origin
    (default: a 420 m x 360 m block at 60 %/30 % of the extent); shift: added to every coordinate (a multiple of 0.5 m
    keeps the lattice)."""
    rng = np.random.default_rng(seed)
    ox, oy = float(origin[0]) + shift[0], float(origin[1]) + shift[1]
    ex, ey = float(extent[0]), float(extent[1])
    bx, by = float(block[0]), float(block[1])
    nx, ny = int(ex // bx), int(ey // by)
    J = lanes_per_dir * LANE_W + 3.0                       # junction box half size
    offs = [(k + 0.5) * LANE_W for k in range(lanes_per_dir)]
    if park is None:
        px, py = np.floor(0.6 * ex / 2) * 2, np.floor(0.3 * ey / 2) * 2
        park = (px, py, px + 420.0, py + 360.0)
    pk = (ox + park[0], oy + park[1], ox + park[2], oy + park[3])
    centre = lambda i, j: (ox + i * bx, oy + j * by)
    exists = lambda i, j: 0 <= i <= nx and 0 <= j <= ny
    lanes = []
    # street segments between neighbouring junctions, both directions
    for i in range(nx + 1):
        for j in range(ny + 1):
            for d in ((1, 0), (0, 1)):
                if not exists(i + d[0], j + d[1]):
                    continue
                c1, c2 = centre(i, j), centre(i + d[0], j + d[1])
                length = abs(c2[0] - c1[0]) + abs(c2[1] - c1[1]) - 2 * J
                n = int(round(length / STEP)) + 1
                for dd, start in ((d, c1), ((-d[0], -d[1]), c2)):
                    r = _right(dd)
                    for o in offs:
                        p0 = (start[0] + J * dd[0] + o * r[0], start[1] + J * dd[1] + o * r[1])
                        lanes.append(_line(p0, dd, n))
    # junction connectors: every incoming lane straight on, left and right onto the same lane of the exit road
    junctions = []
    for i in range(nx + 1):
        for j in range(ny + 1):
            c = centre(i, j)
            junctions.append(c)
            for d in _DIRS:
                if not exists(i - d[0], j - d[1]):                  # no road to come in from
                    continue
                for e in (d, _right(d), (-_right(d)[0], -_right(d)[1])):
                    if not exists(i + e[0], j + e[1]):
                        continue
                    for o in offs:
                        rd, re = _right(d), _right(e)
                        p0 = (c[0] - J * d[0] + o * rd[0], c[1] - J * d[1] + o * rd[1])
                        p1 = (c[0] + J * e[0] + o * re[0], c[1] + J * e[1] + o * re[1])
                        if e == d:
                            ctl = ((p0[0] + p1[0]) / 2, (p0[1] + p1[1]) / 2)
                        else:
                            t = (p1[0] - p0[0]) * d[0] + (p1[1] - p0[1]) * d[1]
                            ctl = (p0[0] + t * d[0], p0[1] + t * d[1])
                        lanes.append(_bezier(p0, ctl, p1))
    # a diagonal avenue from the south-west towards the north-east, and a ring road
    ang = np.deg2rad(33.0)
    u, v = np.array([np.cos(ang), np.sin(ang)]), np.array([np.sin(ang), -np.cos(ang)])
    a0 = np.array([ox + 0.05 * ex, oy + 0.1 * ey])
    span = min((ex * 0.9) / u[0], (ey * 0.85) / u[1])
    s = np.arange(0.0, span, STEP)[:, None]
    for o in offs:
        fwd = a0 + o * v + s * u
        lanes.append(np.concatenate([fwd, np.full((fwd.shape[0], 1), ang)], 1))
        back = (a0 - o * v + s * u)[::-1]
        lanes.append(np.concatenate([back, np.full((back.shape[0], 1), ang - np.pi)], 1))
    rc = (ox + 0.45 * ex, oy + 0.55 * ey)
    R = 0.3 * min(ex, ey)
    for o in offs:
        lanes.append(_arc(rc[0], rc[1], R + o, 0.0, 2 * np.pi, True))
        lanes.append(_arc(rc[0], rc[1], R - o, 2 * np.pi, 0.0, False))
    # the park: no lane inside; the lanes are shuffled lane by lane
    kept = []
    for ln in lanes:
        inside = (ln[:, 0] > pk[0]) & (ln[:, 0] < pk[2]) & (ln[:, 1] > pk[1]) & (ln[:, 1] < pk[3])
        if (~inside).any():
            kept.append(ln[~inside])
    order = rng.permutation(len(kept))
    lane = np.concatenate([kept[k] for k in order], 0)
    m = CityMap(lane=lane, origin=(ox, oy), extent=(ex, ey), park=pk, junctions=np.array(junctions), junction_half=J)
    # exact ties: on the centre line of a straight road (lane points of both directions at the same distance), and a
    # quarter metre further (four of them at once); and between two consecutive points of one lane
    ties = []
    for _ in range(64):
        i, j = int(rng.integers(0, nx)), int(rng.integers(0, ny + 1))          # east-west segment (i, j) -> (i + 1, j)
        c = centre(i, j)
        x = c[0] + J + STEP * int(rng.integers(0, int((bx - 2 * J) / STEP)))
        ties.append((x, c[1]))
        ties.append((x + 0.25, c[1]))
        ties.append((x + 0.25, c[1] - offs[-1] + 0.375))                    # two neighbours on the outer lane
        i, j = int(rng.integers(0, nx + 1)), int(rng.integers(0, ny))          # north-south segment
        c = centre(i, j)
        y = c[1] + J + STEP * int(rng.integers(0, int((by - 2 * J) / STEP)))
        ties.append((c[0], y))
        ties.append((c[0] + offs[0] - 0.625, y + 0.25))
    t = np.array(ties)
    inpark = (t[:, 0] > pk[0] - 5) & (t[:, 0] < pk[2] + 5) & (t[:, 1] > pk[1] - 5) & (t[:, 1] < pk[3] + 5)
    t = t[~inpark]
    # where the avenue or the ring road crosses a street, their points may come nearer than the tied pair: drop those
    yaw = lane[:, 2]
    off_axis = lane[~(np.isin(yaw, [0.0, np.pi / 2, np.pi, -np.pi / 2])), :2]
    near = np.zeros(t.shape[0], bool)
    for a in range(0, off_axis.shape[0], 20000):
        q = off_axis[a:a + 20000]
        near |= ((t[:, 0, None] - q[None, :, 0]) ** 2 + (t[:, 1, None] - q[None, :, 1]) ** 2 < 36.0).any(1)
    m.ties = t[~near]
    return m


@functools.lru_cache(maxsize=1)
def city_maps():
    """The four maps of the tests (extents 1.5-4 km; every one covers the ego of synthetic.make_frame's default pose,
    ~(600, 1600) +- 200 m) and a copy of the first one shifted out to ~10 km (it covers the ego of ego_magnitude=10000)."""
    maps = [
        city_map(origin=(30.0, 45.0), extent=(1500.0, 2000.0), block=(150.0, 160.0), lanes_per_dir=2, seed=1),
        city_map(origin=(12.5, 20.0), extent=(2600.0, 2400.0), block=(290.0, 275.0), lanes_per_dir=2, seed=2),
        city_map(origin=(55.0, 8.0), extent=(4000.0, 2200.0), block=(360.0, 300.0), lanes_per_dir=2, seed=3),
        city_map(origin=(5.0, 70.0), extent=(3000.0, 3800.0), block=(1000.0, 950.0), lanes_per_dir=3, seed=4),
    ]
    maps.append(city_map(origin=(30.0, 45.0), extent=(1500.0, 2000.0), block=(150.0, 160.0), lanes_per_dir=2, seed=1,
                         shift=(3000.0, 8500.0)))
    return tuple(maps)


# ------------------------------------------------------------------------------------------ grid geometry on the host
def grid_geometry(lane):
    """(x0, y0, h, inv_h, gw, gh) of the index k_lane_grid_build makes of one table, in the kernel's float32
    arithmetic: bounding box of the float32 points, h grown by 1.25 until (floor(ex/h)+2)(floor(ey/h)+1) cells fit
    LG_MAX_CELLS, gw made odd."""
    f = np.float32
    l32 = np.asarray(lane, np.float64).astype(np.float32).reshape(-1, 3)
    ok = ~(np.isnan(l32[:, 0]) | np.isnan(l32[:, 1]))
    x, y = l32[ok, 0], l32[ok, 1]
    mnx, mxx, mny, mxy = (x.min(), x.max(), y.min(), y.max()) if x.size else (f(0), f(0), f(0), f(0))
    ex, ey = f(mxx - mnx), f(mxy - mny)
    h = f(LG_CELL0)
    while float(np.floor(f(ex / h)) + f(2)) * float(np.floor(f(ey / h)) + f(1)) > LG_MAX_CELLS:
        h = f(h * f(1.25))
    gw, gh = int(np.floor(f(ex / h))) + 1, int(np.floor(f(ey / h))) + 1
    return f(mnx), f(mny), h, f(f(1.0) / h), gw | 1, gh


def cell_counts(lane):
    """Points per cell of the index (the build's float32 bin expression; (gh, gw) array)."""
    x0, y0, h, inv_h, gw, gh = grid_geometry(lane)
    l32 = np.asarray(lane, np.float64).astype(np.float32).reshape(-1, 3)
    cx = np.clip(np.floor((l32[:, 0] - x0) * inv_h).astype(np.int64), 0, gw - 1)
    cy = np.clip(np.floor((l32[:, 1] - y0) * inv_h).astype(np.int64), 0, gh - 1)
    return np.bincount(cy * gw + cx, minlength=gw * gh).reshape(gh, gw)


# ------------------------------------------------------------------------------------------ crafted centroids
def _ulps(v, k):
    """float32 v moved by k ulps (k may be negative)."""
    v = np.float32(v)
    for _ in range(abs(k)):
        v = np.nextafter(v, np.float32(np.inf) if k > 0 else np.float32(-np.inf), dtype=np.float32)
    return v


def crafted_centroids(m: CityMap, seed=0, n=(300, 100, 120, 60, 60, 40, 40)):
    """float32 (K, 3) centroid sets for map m, by name:
    near (0-5 m from a lane point), on (exactly on lane points, duplicated connector ends among them), tie (m.ties),
    junction (inside junction boxes), cell (on grown-grid cell boundaries x0 + k h / y0 + k h and 1-2 ulp either side),
    park (inside the park, >= 2 h + 10 m from its edges), fallback (more than 64 h outside the bounding box: the ring
    search gives up at once), far (10-60 h outside: the far rings)."""
    n_near, n_on, n_junc, n_cellb, n_park, n_fall, n_far = n
    rng = np.random.default_rng(seed)
    l32 = m.lane.astype(np.float32)
    L = l32.shape[0]
    x0, y0, h, inv_h, gw, gh = grid_geometry(m.lane)
    out = {}
    p = l32[rng.integers(0, L, n_near), :2].astype(np.float64)
    r, a = 5.0 * np.sqrt(rng.uniform(0, 1, n_near)), rng.uniform(-np.pi, np.pi, n_near)
    out["near"] = np.stack([p[:, 0] + r * np.cos(a), p[:, 1] + r * np.sin(a)], 1)
    # duplicated rows (a connector's first point is its incoming lane's last): half of the on-lane set
    _, first, cnt = np.unique(l32[:, :2], axis=0, return_index=True, return_counts=True)
    dup = first[cnt > 1]
    pick = np.concatenate([rng.choice(dup, min(dup.size, n_on // 2), replace=False), rng.integers(0, L, n_on - min(dup.size, n_on // 2))])
    out["on"] = l32[pick, :2].astype(np.float64)
    out["tie"] = m.ties
    jc = m.junctions[rng.integers(0, len(m.junctions), n_junc)]
    out["junction"] = jc + rng.uniform(-m.junction_half, m.junction_half, (n_junc, 2))
    # cell boundaries near lane points: x = x0 + k h (rounded to float32) and +-1, +-2 ulp; the other coordinate
    # within 3 m of the lane point
    rows = []
    for q in l32[rng.integers(0, L, n_cellb), :2].astype(np.float64):
        axis = int(rng.integers(0, 2))
        base = (x0, y0)[axis]
        k = int(np.round((q[axis] - float(base)) / float(h)))
        b = np.float32(float(base) + k * float(h))
        other = q[1 - axis] + rng.uniform(-3, 3)
        for u in (-2, -1, 0, 1, 2):
            c = [0.0, 0.0]
            c[axis], c[1 - axis] = float(_ulps(b, u)), other
            rows.append(c)
    out["cell"] = np.array(rows)
    px0, py0, px1, py1 = m.park
    mg = 2 * float(h) + 10.0
    out["park"] = np.stack([rng.uniform(px0 + mg, px1 - mg, n_park), rng.uniform(py0 + mg, py1 - mg, n_park)], 1)
    bb = (float(l32[:, 0].min()), float(l32[:, 1].min()), float(l32[:, 0].max()), float(l32[:, 1].max()))

    def outside(k, lo, hi):
        side = rng.integers(0, 4, k)
        dist = rng.uniform(lo, hi, k)
        along = rng.uniform(0, 1, k)
        x = np.where(side == 0, bb[0] - dist, np.where(side == 1, bb[2] + dist, bb[0] + along * (bb[2] - bb[0])))
        y = np.where(side == 2, bb[1] - dist, np.where(side == 3, bb[3] + dist, bb[1] + along * (bb[3] - bb[1])))
        return np.stack([x, y], 1)
    out["fallback"] = outside(n_fall, LG_MAX_RINGS * float(h) + 20.0, LG_MAX_RINGS * float(h) + 3000.0)
    out["far"] = outside(n_far, 10 * float(h), 60 * float(h))
    return {k: np.concatenate([v, rng.uniform(-2, 2, (v.shape[0], 1))], 1).astype(np.float32) for k, v in out.items()}


def degenerate_tables(seed=0):
    """Tables a grid gets wrong first: 1 point, 2 points, all on one horizontal line (gh = 1), all on one vertical
    line (gw = 1), all identical (extent 0), every row twice or three times.  Returns (name, float64 (L, 3)) pairs."""
    rng = np.random.default_rng(seed)
    yaw = lambda n: rng.uniform(-np.pi, np.pi, n)
    xs = 812.5 + np.arange(4000) * STEP
    base = rng.uniform(-150, 150, (700, 2)) + [2400.0, 900.0]
    rep = np.repeat(np.arange(700), rng.integers(2, 4, 700))
    return [
        ("one", np.array([[1234.25, 567.5, 0.3]])),
        ("two", np.array([[100.0, 200.0, 1.0], [130.5, 180.25, -2.0]])),
        ("hline", np.stack([xs, np.full(xs.size, 1500.25), yaw(xs.size)], 1)),
        ("vline", np.stack([np.full(xs.size, -340.75), xs - 3000.0, yaw(xs.size)], 1)),
        ("same", np.tile([[777.5, 1888.25, 0.5]], (300, 1)) + np.stack([np.zeros(300), np.zeros(300), yaw(300)], 1)),
        ("dups", np.concatenate([base[rep], yaw(rep.size)[:, None]], 1)),
    ]


def degenerate_centroids(lane, seed=0, k=150):
    """float32 centroids for a small table: on its points, between two of them, around it and far outside."""
    rng = np.random.default_rng(seed)
    l32 = np.asarray(lane, np.float64).astype(np.float32)
    L = l32.shape[0]
    on = l32[rng.integers(0, L, k // 3), :2].astype(np.float64)
    mid = (l32[rng.integers(0, L, k // 3), :2].astype(np.float64) + l32[rng.integers(0, L, k // 3), :2]) / 2
    c = l32[:, :2].astype(np.float64).mean(0)
    span = float(np.ptp(l32[:, :2], 0).max()) + 10.0
    around = c + rng.uniform(-span, span, (k // 6, 2))
    far = c + rng.choice([-1, 1], (k - len(on) - len(mid) - len(around), 2)) * rng.uniform(500, 5000, (k - len(on) - len(mid) - len(around), 2))
    p = np.concatenate([on, mid, around, far], 0)
    return np.concatenate([p, np.zeros((p.shape[0], 1))], 1).astype(np.float32)


# ------------------------------------------------------------------------------------------ the ring-stop margin
def _f32_bins(lane):
    x0, y0, h, inv_h, gw, gh = grid_geometry(lane)
    l32 = np.asarray(lane, np.float64).astype(np.float32).reshape(-1, 3)
    ci = np.clip(np.floor((l32[:, 0] - x0) * inv_h).astype(np.int64), 0, gw - 1)
    cj = np.clip(np.floor((l32[:, 1] - y0) * inv_h).astype(np.int64), 0, gh - 1)
    return ci, cj


def grid_margin(lane):
    """The ring-stop margin k_lane_grid_build stores: 16 ulp of the largest |coordinate| + 1e-4 h, in float32."""
    f = np.float32
    l32 = np.asarray(lane, np.float64).astype(np.float32).reshape(-1, 3)
    big = np.abs(l32[:, :2]).max()
    return f(f(f(16.0) * f(1.1920929e-7)) * big) + f(f(1e-4) * grid_geometry(lane)[2])


def emulate_lane_nn(lane, c, use_margin=True):
    """Host model of k_lane_nn_grid for one float32 centroid c: points binned in float32, the centroid's cell in double,
    rings searched in the kernel's batches (0-2, 3-5, 6-9, 10-15, ...) with its stop test `best < r h - margin`
    (use_margin=False: without `- margin`), the exact scan after LG_MAX_RINGS; (distance, index) minimum.  Returns the
    index."""
    x0, y0, h, inv_h, gw, gh = grid_geometry(lane)
    ci, cj = _f32_bins(lane)
    l32 = np.asarray(lane, np.float64).astype(np.float32).reshape(-1, 3).astype(np.float64)
    cx, cy = float(np.float32(c[0])), float(np.float32(c[1]))
    d = np.sqrt((cx - l32[:, 0]) ** 2 + (cy - l32[:, 1]) ** 2)
    qi = int(max(-1e6, min(1e6, np.floor((cx - float(x0)) * float(inv_h)))))
    qj = int(max(-1e6, min(1e6, np.floor((cy - float(y0)) * float(inv_h)))))
    out_i = -qi if qi < 0 else (qi - gw + 1 if qi >= gw else 0)
    out_j = -qj if qj < 0 else (qj - gh + 1 if qj >= gh else 0)
    cheb = np.maximum(np.abs(ci - qi), np.abs(cj - qj))
    stop = float(grid_margin(lane)) if use_margin else 0.0
    r_done, seen = max(out_i, out_j) - 1, None
    while r_done < LG_MAX_RINGS:
        r_lo = r_done + 1
        r_hi = 2 if r_lo == 0 else min(LG_MAX_RINGS, r_lo + max(2, r_lo // 2))
        r_done = r_hi
        seen = cheb <= r_done
        wb = d[seen].min() if seen.any() else np.inf
        if wb < r_done * float(h) - stop:
            break
        if qi - r_done <= 0 and qi + r_done >= gw - 1 and qj - r_done <= 0 and qj + r_done >= gh - 1:
            break
    else:
        seen = np.ones(d.size, bool)
    cand = np.flatnonzero(seen)
    return int(cand[np.lexsort((cand, d[cand]))[0]])


def margin_cases(seed=0, per_ring=2):
    """Small float32 tables on which the ring-stop margin decides the answer.  Two corner points set a bounding box that grows
    the cell (12.2-24 m).  The centroid sits at the right edge of its cell; B, to its right, is binned by the float32
    product one cell further out than its true position, so after the stop ring R it is still unvisited although it lies
    nearer than R h; A, to the left, is visited at a distance between B's and R h.  With the
    margin the search goes on and finds B (the brute force's answer); without it the search stops at R and returns A.
    Returns a list of (table float64 (4, 3), centroid float32 (3,), R); every case is checked with emulate_lane_nn."""
    f32 = np.float32
    rng = np.random.default_rng(seed)
    up = lambda v: np.nextafter(f32(v), f32(np.inf), dtype=f32)
    down = lambda v: np.nextafter(f32(v), f32(-np.inf), dtype=f32)
    cases = []
    for corner, ext in (((592.18274, 0.0), 4000.0), ((1.2345678, 3.3), 2000.0), ((3011.4321, 8507.7), 3000.0)):
        corners = np.array([[corner[0], corner[1], 0.0], [corner[0] + ext, corner[1] + ext, 0.0]])
        x0, y0, h, inv_h, gw, gh = grid_geometry(corners)
        bin32 = lambda v: int(np.floor(f32(f32(f32(v) - x0) * inv_h)))
        for R in (5, 9, 15, 24):
            found = 0
            for _ in range(20000):
                qi, qj = int(rng.integers(R + 4, gw - R - 5)), int(rng.integers(R + 4, gh - R - 5))
                # c: the last float32 of its cell (double binning); B: the first float32 the float32 binning puts R + 1 cells
                # further right -- the product rounds up onto the cell edge, so B can lie nearer than R h
                cx = up(up(float(x0) + (qi + 1) / float(inv_h)))
                while np.floor((float(cx) - float(x0)) * float(inv_h)) > qi:
                    cx = down(cx)
                cy = f32(float(y0) + (qj + rng.uniform(0.3, 0.7)) / float(inv_h))
                bx = down(down(float(cx) + R * float(h)))
                while bin32(bx) < qi + R + 1:
                    bx = up(bx)
                by = f32(float(cy) + rng.uniform(-0.02, 0.02))
                dB = np.hypot(float(cx) - float(bx), float(cy) - float(by))
                if dB >= R * float(h):
                    continue
                v = rng.uniform(1.0, 6.0)
                t = dB + rng.uniform(0.0, 1.0) * (R * float(h) - dB)
                ax, ay = f32(float(cx) - np.sqrt(t * t - v * v)), f32(float(cy) + v)
                dA = np.hypot(float(ax) - float(cx), float(ay) - float(cy))
                if not dB < dA < R * float(h):
                    continue
                pts = [[ax, ay], [bx, by]] if rng.random() < 0.5 else [[bx, by], [ax, ay]]
                table = np.concatenate([corners, np.concatenate([np.array(pts, np.float64), rng.uniform(-3, 3, (2, 1))], 1)], 0)
                c = np.array([cx, cy, 0.0], np.float32)
                l32 = table.astype(np.float32)
                d = np.sqrt((float(cx) - l32[:, 0].astype(np.float64)) ** 2 + (float(cy) - l32[:, 1].astype(np.float64)) ** 2)
                j = int(np.argmin(d))
                if emulate_lane_nn(table, c, True) == j and emulate_lane_nn(table, c, False) != j:
                    cases.append((table, c, R))
                    found += 1
                    if found == per_ring:
                        break
    return cases
