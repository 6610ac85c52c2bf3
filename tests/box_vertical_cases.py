"""Inputs of the vertical stage's tests (cm3d_box_vertical; numpy only): (a) lists of every length at which the kernel changes its
route and of every kind of value the key order has to get right, (b) tables of the apply step, (c) a geometry case with a bound
derived from its own beam table, and a scalar loop written apart from the host statement (`sorted` on integer keys per mask, Python
floats for the apply step) that both the host statement and the device are held against."""
import math

import numpy as np

BOX_STRIDE = 10
# the kernel's route thresholds (include/cm3d_hip.h): up to LANE_MAX points a list sits one per lane of a wave; above it the workgroup's
# 256 threads select it together (BLOCK_THREADS: the stride of their walk); up to LDS_KEYS keys are staged in LDS, longer lists are streamed
LANE_MAX, BLOCK_THREADS, LDS_KEYS = 64, 256, 4096
LENGTHS = (0, 1, 2, 4, 5, 6, LANE_MAX - 1, LANE_MAX, LANE_MAX + 1, 127, 128, 129, BLOCK_THREADS - 1, BLOCK_THREADS, BLOCK_THREADS + 1, 1000,
           LDS_KEYS - 1, LDS_KEYS, LDS_KEYS + 1, 5003)
_Q = 0.25, 0.75                                  # q (n - 1) is an integer for n = 5, 65, 129, 257, 4097, ...
QUANTILES = ((0.0, 1.0), (0.02, 0.98), (0.5, 0.5), (0.0, 0.0), (1.0, 1.0), _Q,
             (float(np.nextafter(_Q[0], 0.0)), float(np.nextafter(_Q[1], 0.0))))          # ... and lies just below one
DEFAULTS = dict(q_bot=0.02, q_top=0.98, min_points=5, lo=0.7, hi=1.3)
PRIOR = np.array([[2.1, 4.9, 1.7], [0.7, 0.8, 1.75], [2.9, 11.0, 3.5]], np.float64)


def _pack(lists, rng, tail=0):
    """Lists of z values -> (xyz (n + tail, 4) float32, off).  Columns 0, 1 and 3 hold what the stage must not look at: NaN, inf, noise."""
    off = np.concatenate([[0], np.cumsum([len(z) for z in lists])]).astype(np.int32)
    n = int(off[-1])
    xyz = rng.normal(0.0, 50.0, (n + tail, 4)).astype(np.float32)
    xyz[::7, 0], xyz[3::11, 1], xyz[5::13, 3] = np.nan, np.inf, -np.inf
    if n:
        xyz[:n, 2] = np.concatenate([np.asarray(z, np.float32) for z in lists])
    return xyz, off


def _boxes(M, rng, n_classes=len(PRIOR)):
    box = rng.normal(0.0, 20.0, (M, BOX_STRIDE))
    box[:, 8] = rng.integers(0, n_classes, M)
    flags = np.where(rng.random(M) < 0.8, 3, 1).astype(np.int32)
    flags[::9] = 0
    box[:, 9] = flags
    return box, flags


def list_case():
    """(a): every length with mixed-sign values, then the value kinds on the lane route (40), the block route with staged keys (300)
    and, for some, the streamed route (4200 and up)."""
    rng = np.random.default_rng(28)
    names, lists = [], []

    def add(name, z):
        names.append(name), lists.append(np.asarray(z, np.float32))
    for n in LENGTHS:
        add(f"len{n}", rng.normal(0.3, 2.0, n))
    tiny = np.float32(1e-45)                        # the smallest denormal
    for n in (40, 300, 4200):
        add(f"equal{n}", np.full(n, 1.25))
        add(f"rings{n}", rng.choice(np.array([-1.5, 0.25, 0.75], np.float32), n))
        add(f"zeros{n}", rng.choice(np.array([-0.0, 0.0], np.float32), n))
        add(f"upright{n}", rng.uniform(-0.4, 1.35, n))        # about one prior of class 0 tall: judged "both ends" at the defaults
    for n in (40, 300):
        add(f"denormal{n}", (rng.integers(-50, 50, n) * tiny).astype(np.float32))
        add(f"lastbit{n}", (np.float32(1000.0).view(np.uint32) + rng.integers(0, 4, n).astype(np.uint32)).view(np.float32))
        multiset = np.sort(np.concatenate([rng.normal(0.0, 3.0, n - 4), [-0.0, 0.0, 0.0, -0.0]]).astype(np.float32))
        add(f"ascending{n}", multiset), add(f"descending{n}", multiset[::-1]), add(f"shuffled{n}", rng.permutation(multiset))
        for kind, v in (("nan", np.nan), ("pinf", np.inf), ("ninf", -np.inf)):
            for where, i in (("first", 0), ("middle", n // 2), ("last", n - 1)):
                z = rng.normal(0.0, 1.0, n)
                z[i] = v
                add(f"{kind}_{where}{n}", z)
    z = rng.normal(0.0, 1.0, 4500)
    z[-1] = np.nan
    add("nan_last4500", z)
    xyz, off = _pack(lists, rng)
    box, flags = _boxes(len(lists), rng)
    for i, name in enumerate(names):
        if name.startswith("upright"):
            box[i, 8], flags[i], box[i, 9] = 0.0, 3, 3.0
    return dict(name="lists", names=names, xyz=xyz, off=off, idx_cap=int(off[-1]), box=box, flags=flags, prior_wlh=PRIOR, runs=[{}])


def overflow_case():
    """A simulated capacity overflow: the compaction stopped writing at idx_cap, the offsets run on.  Rows from idx_cap on are NaN (a
    read of them shows as status 4 or as a wrong value), offsets lie beyond idx_cap, below zero and below their predecessor."""
    rng = np.random.default_rng(29)
    idx_cap = 700
    xyz, _ = _pack([rng.normal(0.0, 2.0, idx_cap)], rng, tail=600)
    xyz[idx_cap:] = np.nan
    off = np.array([0, 100, 250, 640, 900, 850, 1300, -5, 30, 2 ** 31 - 1, 690, 701, 700, 0, 800], np.int32)
    box, flags = _boxes(off.size - 1, rng)
    flags[:] = 3
    box[:, 9] = 3
    return dict(name="overflow", xyz=xyz, off=off, idx_cap=idx_cap, box=box, flags=flags, prior_wlh=PRIOR, runs=[{}, dict(min_points=1)])


def apply_case():
    """(b): lists of five points whose ends are the order statistics with (0, 1); every row of the rule's table.  The runs move lo and
    hi one ulp around the ratio of mask 0."""
    rng = np.random.default_rng(30)
    prior = np.array([[2.0, 4.5, 1.7], [1.0, 1.0, 0.0], [1.0, 1.0, -1.6], [1.0, 1.0, np.nan], [1.0, 1.0, np.inf], [0.6, 0.7, 1.1]], np.float64)
    rows = []                                       # (name, z list, class column, flags, entry z)

    def five(lo, hi):
        return np.array([lo, hi, lo + (hi - lo) * 0.3, hi, lo], np.float32)
    rows.append(("ratio", five(0.11, 1.93), 0.0, 3, 0.5))
    rows.append(("both_ends", five(-0.2, 1.6), 0.0, 1, 0.7))
    rows.append(("extent_zero", np.full(5, 0.8, np.float32), 0.0, 3, 0.1))
    rows.append(("top_only", five(1.0, 1.5), 0.0, 3, 1.2))
    rows.append(("too_tall", five(-0.5, 4.0), 0.0, 3, 1.0))
    for c, what in ((1.0, "zero"), (2.0, "negative"), (3.0, "nan"), (4.0, "inf")):
        rows.append((f"h0_{what}", five(0.0, 1.5), c, 3, 0.3))
    rows.append(("class_below", five(0.0, 1.7), -1.0, 3, 0.3))
    rows.append(("class_above", five(0.0, 1.7), float(len(prior)), 3, 0.3))
    rows.append(("class_nan", five(0.0, 1.7), np.nan, 3, 0.3))
    rows.append(("class_fraction", five(0.0, 1.0), 5.75, 3, 0.3))
    rows.append(("flags_0", five(0.0, 1.7), 0.0, 0, 0.3))
    rows.append(("flags_2", five(0.0, 1.7), 0.0, 2, 0.3))
    rows.append(("status_empty", np.zeros(0, np.float32), 0.0, 3, 0.3))
    rows.append(("status_few", np.array([0.0, 1.7, 0.5, 0.6], np.float32), 0.0, 3, 0.3))
    rows.append(("status_not_finite", np.array([0.0, 1.7, np.nan, 0.5, 0.6], np.float32), 0.0, 3, 0.3))
    rows.append(("entry_nan_source_0", five(-0.5, 4.0), 0.0, 3, np.nan))
    rows.append(("entry_inf_source_0", five(0.0, 1.7), 0.0, 0, -np.inf))
    rows.append(("entry_nan_source_1", five(0.0, 1.7), 0.0, 3, np.nan))
    rows.append(("entry_inf_source_2", five(1.0, 1.5), 0.0, 3, np.inf))
    M = len(rows)
    xyz, off = _pack([r[1] for r in rows], rng)
    box = rng.normal(0.0, 20.0, (M, BOX_STRIDE))
    box[:, 8], box[:, 2] = [r[2] for r in rows], [r[4] for r in rows]
    flags = np.array([r[3] for r in rows], np.int32)
    box[:, 9] = flags
    z0 = rows[0][1]
    r0 = (float(z0.max()) - float(z0.min())) / float(prior[0, 2])
    up, dn = float(np.nextafter(r0, np.inf)), float(np.nextafter(r0, -np.inf))
    base = dict(q_bot=0.0, q_top=1.0)
    runs = [dict(base), dict(base, lo=up, hi=2.0), dict(base, lo=r0, hi=2.0), dict(base, lo=dn, hi=2.0), dict(base, lo=0.1, hi=up),
            dict(base, lo=0.1, hi=r0), dict(base, lo=0.1, hi=dn), dict(base, lo=r0, hi=r0)]
    # what mask 0 must come out as in each run: r one ulp below lo: top only; on and above: both ends; ... one ulp above hi: untouched
    return dict(name="apply", names=[r[0] for r in rows], xyz=xyz, off=off, idx_cap=int(off[-1]), box=box, flags=flags, prior_wlh=prior,
                runs=runs, mask0_src=[1, 2, 1, 1, 1, 1, 0, 1])


def all_cases():
    return [list_case(), overflow_case(), apply_case()]


# ---- the scalar loop, written apart from the host statement
def _key(bits):
    return bits ^ (0xFFFFFFFF if bits >> 31 else 0x80000000)


def loop_vertical(case, q_bot, q_top, min_points=5, lo=0.7, hi=1.3):
    """The rule of include/cm3d_hip.h, one mask and one value at a time."""
    zcol = np.ascontiguousarray(case["xyz"][:, 2])
    bits, vals = zcol.view(np.uint32).tolist(), zcol.astype(np.float64).tolist()
    cap, prior = case["idx_cap"], case["prior_wlh"]
    box = case["box"].copy()
    M = box.shape[0]
    out = dict(box=box, vert_z=np.zeros((M, 2)), vert_h=np.zeros(M), vert_src=np.zeros(M, np.int32), vert_status=np.zeros(M, np.int32),
               vert_entry_z=box[:, 2].copy())
    for m in range(M):
        a = min(max(int(case["off"][m]), 0), cap)
        b = min(max(int(case["off"][m + 1]), a), cap)
        n = b - a
        status, zb, zt = 0, 0.0, 0.0
        if n == 0:
            status = 2
        elif n < min_points:
            status = 1
        elif any(math.isnan(v) or math.isinf(v) for v in vals[a:b]):
            status = 4
        else:
            order = sorted(range(a, b), key=lambda i: _key(bits[i]))
            zb, zt = vals[order[int(q_bot * float(n - 1))]], vals[order[int(q_top * float(n - 1))]]
        out["vert_status"][m], out["vert_z"][m] = status, (zb, zt)
        c8 = float(box[m, 8])
        cls = int(c8) if 0.0 <= c8 < float(prior.shape[0]) else 0
        h0 = float(prior[cls, 2])
        h, src = prior[cls, 2], 0
        if (int(case["flags"][m]) & 1) and status == 0 and not math.isnan(h0) and not math.isinf(h0) and h0 > 0.0:
            ext = zt - zb
            r = ext / h0
            if r < lo:
                src, box[m, 2] = 2, zt - h0 * 0.5
            elif r <= hi:
                src, h, box[m, 2] = 1, ext, zb + ext * 0.5
        out["vert_h"][m], out["vert_src"][m] = h, src
    return out


def _bits(a):
    return np.ascontiguousarray(a, np.float64).view(np.uint64)


def assert_same(got, exp, what=""):
    """Every output and box to the bit (NaN payloads included: no operation of the rule forms a NaN, they are only ever copied)."""
    for k in ("vert_status", "vert_src"):
        assert np.array_equal(np.asarray(got[k]), np.asarray(exp[k])), (what, k, np.flatnonzero(np.asarray(got[k]) != np.asarray(exp[k]))[:8])
    for k in ("vert_z", "vert_h", "vert_entry_z", "box"):
        g, e = _bits(got[k]).reshape(-1), _bits(exp[k]).reshape(-1)
        assert g.shape == e.shape and np.array_equal(g, e), (what, k, np.flatnonzero(g != e)[:8])


# ---- (c) geometry: an upright box seen face on by a spinning LiDAR
GEO_SIZE = (4.9, 2.1, 1.9)                         # length, width, height of the object, standing on z = 0
GEO_SENSOR_Z, GEO_BEAMS, GEO_ELEV = 1.84, 32, (-30.0, 10.0)
GEO_PRIOR_H = 1.7                                  # the class's prior height: not the object's
GEO_COLUMNS = 9                                    # azimuth steps that hit the face: every ring leaves that many points
GEO_SCENES = [(d, lo) for d in (8.0, 25.0) for lo in (0.0, 0.9)]       # (range, everything below this height is occluded)


def geometry_scene(d, visible_from):
    """The points of one scene and the bound on the stage's error.  The face is the plane at ground range d; a ring is taken as level
    across it.  Beam i hits at z_i = sensor + d tan(e_i); the points are the z_i inside [visible_from, height], GEO_COLUMNS each.
    Bound (DEFAULTS): let dz be the largest gap between beams that are neighbours around the visible span.  The true top lies between
    the highest ring that hits and the next beam above it, so that ring is within dz of it; q_top skips s = n - 1 - kt points from the
    top, which is s // GEO_COLUMNS whole rings: the top value is within tb = (s // GEO_COLUMNS + 1) dz below the top.  The bottom value
    alike within bb = (kb // GEO_COLUMNS + 1) dz above visible_from.
      source 1 (both ends): |h - height| <= tb + bb, and with nothing occluded |z - height / 2| <= max(tb, bb) / 2;
      source 2 (top only):  h is the prior's, |z - height / 2| <= tb + |prior - height| / 2.
    An occluded scene shows at most height - visible_from = 1.0 m = 0.59 priors < lo: source 2 for certain.  A whole one shows at least
    height - tb - bb: source 1 for certain where that is >= lo priors, else either source, each held against its own line."""
    H = GEO_SIZE[2]
    elev = np.deg2rad(np.linspace(GEO_ELEV[0], GEO_ELEV[1], GEO_BEAMS))
    zi = GEO_SENSOR_Z + d * np.tan(elev)
    hit = (zi >= visible_from) & (zi <= H)
    assert hit.any() and zi[0] < visible_from and zi[-1] > H
    first, last = np.flatnonzero(hit)[[0, -1]]
    dz = float(np.diff(zi[first - 1:last + 2]).max())
    rings = zi[hit]
    y = np.linspace(-GEO_SIZE[1] / 2, GEO_SIZE[1] / 2, GEO_COLUMNS)
    pts = np.array([[d, yy, zz, 0.0] for zz in rings for yy in y], np.float32)
    n = len(pts)
    kb, kt = int(DEFAULTS["q_bot"] * float(n - 1)), int(DEFAULTS["q_top"] * float(n - 1))
    tb, bb = ((n - 1 - kt) // GEO_COLUMNS + 1) * dz, (kb // GEO_COLUMNS + 1) * dz
    eps = 1e-5                                      # float32 rounding of coordinates of a few metres
    sources = (2,) if visible_from > 0.0 else ((1,) if (H - tb - bb) / GEO_PRIOR_H >= DEFAULTS["lo"] else (1, 2))
    bound = {1: dict(h=tb + bb + eps, z=max(tb, bb) / 2 + eps), 2: dict(h=abs(GEO_PRIOR_H - H) + eps, z=tb + abs(GEO_PRIOR_H - H) / 2 + eps)}
    return dict(xyz=pts, n=n, dz=dz, tb=tb, bb=bb, sources=sources, bound=bound, true_h=H, true_z=H / 2)


def medoid_z(xyz):
    """z of the point with the smallest sum of distances to the others (what the pass puts into column 2), for the printed comparison."""
    p = np.asarray(xyz, np.float64)[:, :3]
    dist = np.sqrt(((p[:, None] - p[None]) ** 2).sum(-1)).sum(1)
    return float(p[np.argmin(dist), 2])
