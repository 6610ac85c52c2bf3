"""Lists for the tests of the depth clustering (cm3d_amd/cluster.py, cm3d_depth_cluster): hand-written rows, the random recipe, and the
O(n^2) statement both are held against -- clusters as the connected components of "|ri - rj| <= eps"."""
import numpy as np

from cm3d_amd import cluster

EPS, MIN_POINTS = 1.0, 20          # the reference's commented-out values: what the calls over many lists use
ORIGINS = np.array([[0.0, 0.0, 0.0], [600.0, 1600.0, 0.0], [-35.25, 12.5, 1.84]], np.float64)


def brute_force(xyz, origin, eps, min_points, pick):
    """(keep, status) from the connected components of |ri - rj| <= eps, found by flooding the full adjacency matrix."""
    r = cluster.ranges(xyz, origin)
    n = r.size
    if n == 0:
        return np.zeros(0, bool), cluster.EMPTY
    with np.errstate(invalid="ignore"):
        adj = np.abs(r[:, None] - r[None, :]) <= eps
    comp = np.full(n, -1)
    n_comp = 0
    for s in range(n):
        if comp[s] >= 0:
            continue
        todo, comp[s] = [s], n_comp
        while todo:
            i = todo.pop()
            for j in np.flatnonzero(adj[i] & (comp < 0)):
                comp[j] = n_comp
                todo.append(int(j))
        n_comp += 1
    sizes = np.bincount(comp, minlength=n_comp)
    first = np.array([r[comp == c].min() for c in range(n_comp)])
    ok = [c for c in range(n_comp) if sizes[c] >= min_points]
    if not ok:
        return np.ones(n, bool), cluster.KEPT_WHOLE
    pick = cluster.pick_code(pick)
    c = min(ok, key=(lambda c: first[c]) if pick == 1 else (lambda c: (-sizes[c], first[c])))
    return comp == c, cluster.KEPT


def on_axis(ranges_, origin=0, shuffle=None):
    """Points at the given ranges on the x axis through ORIGINS[origin] (origin 0: r is exactly the float32 value)."""
    p = np.zeros((len(ranges_), 3), np.float64)
    p[:, 0] = np.asarray(ranges_, np.float64)
    p += ORIGINS[origin]
    p = p.astype(np.float32)
    if shuffle is not None:
        p = p[np.random.default_rng(shuffle).permutation(len(p))]
    return p


def _blob(centre, n, width=0.5):
    return list(centre + width * (np.arange(n) / max(n - 1, 1) - 0.5))


def crafted():
    """name -> (xyz, origin index, eps, min_points, {pick: (kept positions, status)} or None).  The expectations that are written out
    are the point of the row; every row is also held against brute_force."""
    below_one = float(np.nextafter(1.0, 0.0))
    rows = {}
    # 10 and 11 are one gap of exactly 1.0 apart: joined at eps 1, split at the double below 1 (the gap is that eps plus one ulp)
    pair = on_axis([10.0, 11.0, 12.0, 14.0])
    rows["gap_equals_eps_joins"] = (pair, 0, 1.0, 3, {"largest": ([0, 1, 2], 0), "nearest": ([0, 1, 2], 0)})
    rows["gap_eps_plus_ulp_splits"] = (on_axis([10.0, 11.0, 9.5, 13.0]), 0, below_one, 2, {"largest": ([0, 2], 0), "nearest": ([0, 2], 0)})
    chain = on_axis([5.0, 6.0, 7.0, 8.0, 9.0, 10.0 + 2.0 ** -20, 11.0 + 2.0 ** -20], shuffle=3)
    rows["chain_of_exact_gaps"] = (chain, 0, 1.0, 5, None)
    rows["duplicates"] = (on_axis([7.25] * 9 + [9.0] * 4 + [7.25] * 3 + [9.0] * 2), 0, 1.0, 5, {"largest": ([0, 1, 2, 3, 4, 5, 6, 7, 8, 13, 14, 15], 0)})
    tie = on_axis(_blob(30.0, 25) + _blob(12.0, 25) + _blob(20.0, 7), shuffle=5)
    rows["size_tie_goes_to_nearest"] = (tie, 0, EPS, MIN_POINTS, None)
    rows["largest_is_last_in_range"] = (on_axis(_blob(8.0, 21) + _blob(15.0, 22) + _blob(41.0, 30), shuffle=6), 0, EPS, MIN_POINTS, None)
    rows["no_cluster_qualifies"] = (on_axis(_blob(8.0, 19) + _blob(15.0, 12) + _blob(41.0, 19), shuffle=7), 0, EPS, MIN_POINTS,
                                    {"largest": (list(range(50)), 1), "nearest": (list(range(50)), 1)})
    for k in (MIN_POINTS - 1, MIN_POINTS, MIN_POINTS + 1):
        rows[f"cluster_of_{k}"] = (on_axis(_blob(9.0, k) + _blob(25.0, 5), shuffle=k), 0, EPS, MIN_POINTS, None)
    rows["eps_inf_is_one_cluster"] = (on_axis([3.0, 60.0, 1e6, 12.0, 3.0e7]), 0, float("inf"), 5, {"largest": ([0, 1, 2, 3, 4], 0)})
    rows["eps_inf_too_few"] = (on_axis([3.0, 60.0, 1e6]), 0, float("inf"), 4, {"nearest": ([0, 1, 2], 1)})
    rows["far_origin"] = (on_axis(_blob(6.0, 24) + _blob(9.5, 23), origin=1, shuffle=9), 1, EPS, MIN_POINTS, None)
    rows["min_points_one"] = (on_axis([4.0, 9.0, 9.5, 2.0]), 0, 1.0, 1, {"largest": ([1, 2], 0), "nearest": ([3], 0)})
    return rows


def random_list(rng, origin, n=None, centres=None):
    """The random recipe: 1-4 range centres in 3-60 m, sigma 0.4 m, 0-119 points, inside a narrow frustum seen from `origin`."""
    n = int(rng.integers(0, 120)) if n is None else n
    k = int(rng.integers(1, 5)) if centres is None else centres
    c = rng.uniform(3.0, 60.0, k)
    r = np.abs(c[rng.integers(0, k, n)] + rng.normal(0.0, 0.4, n))
    az = rng.uniform(-0.05, 0.05, n) + rng.uniform(-np.pi, np.pi)
    el = rng.uniform(-0.03, 0.03, n)
    d = np.stack([np.cos(el) * np.cos(az), np.cos(el) * np.sin(az), np.sin(el)], 1)
    return (np.asarray(origin, np.float64) + r[:, None] * d).astype(np.float32)


def random_lists(seed, count):
    """[(xyz, origin index)]"""
    rng = np.random.default_rng(seed)
    out = []
    for _ in range(count):
        o = int(rng.integers(0, len(ORIGINS)))
        out.append((random_list(rng, ORIGINS[o]), o))
    return out
