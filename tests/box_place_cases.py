"""Case tables of the box placement (cm3d_box_place; host statement cm3d_amd.boxplace.box_place_host).  Numpy only; nothing here
touches the device.  tests/test_box_place_host.py asserts that the tables hold what they are for.

rule_table(waymo)  (a) records and sensors for the rule, one mask per case, each at its own range from its frame's sensor: the four sign
                   quadrants of (pu, pv), pu == 0 and pv == 0 exactly, a and b each below, on and above THIN, a > len and b > wid,
                   centres at 600 / 1200 m and near 10 km, yaw_src == 0, masks without a box, a NaN sensor (nuScenes), non-finite
                   record values, class ids outside the table.  waymo: the sensor is the origin and ego_xyz is None.
nms_table(waymo)   (b) frames of FRAME_SIZES masks: scattered masks with scores from a short list (ties), a third of them placed; and
                   designed pairs in a group of their own -- squared distance exactly on, just below and just above the threshold,
                   two masks the pushed centres keep apart and the placed centres merge, and the converse.  `pairs`: (i, j, the
                   lower-scored j goes).  To be launched with a bound of 64 and of 1024.
cars(faces)        (c) the visible faces of a CAR_L x CAR_W car at 41 yaws x 12 azimuths x {8, 25} m; the sensor at least MARGIN outside
                   the slab of every face that is shown.
"""
import numpy as np

from tests.bev_fit_cases import CAR_L, CAR_W, CAR_YAWS

THIN = 0.5
THINS = (THIN, 0.0, 1.0)
BOUNDS = (64, 1024)
FRAME_SIZES = (0, 1, 2, 63, 64, 65, 130)
# [w, l, h] per class, NMS group per class, squared-distance threshold per group; group 3 belongs to the designed pairs
PRIOR_WLH = np.array([[1.9, 4.5, 1.6], [2.5, 10.0, 3.0], [0.6, 0.8, 1.7], [2.0, 4.0, 1.5]], np.float64)
NMS_GROUP = np.array([0, 1, 2, 3], np.int32)
NMS_THR = np.array([4.0, 12.0, 0.85, 4.0], np.float64)
AZIMUTHS = np.linspace(0.0, 2.0 * np.pi, 13)[:-1] + 0.1
RANGES = (8.0, 25.0)
MARGIN = 0.5


def _freeze(t):
    for v in t.values():
        if isinstance(v, np.ndarray):
            v.setflags(write=False)
    return t


def _table(rows, sensors, waymo, meta=None):
    """rows: dicts f, pushed (x, y), rect (6,), src, fl, cls, score; sorted into frames here."""
    F = len(sensors)
    rows = sorted(rows, key=lambda r: r["f"])                  # (stable: the order inside a frame is the order of construction)
    M = len(rows)
    box = np.zeros((M, 10))
    box[:, 3] = 1.0
    for m, r in enumerate(rows):
        box[m, 0:2], box[m, 2], box[m, 5], box[m, 6] = r["pushed"], 1.0 + 0.01 * m, 0.1 * (m % 7), 0.25 * m
        box[m, 7], box[m, 8], box[m, 9] = r["score"], r["cls"], r["fl"]
    count = np.bincount([r["f"] for r in rows], minlength=F)
    t = dict(box=box, flags=np.array([r["fl"] for r in rows], np.int32), mask_off=np.concatenate([[0], np.cumsum(count)]).astype(np.int32),
             fit_rect=np.array([r["rect"] for r in rows], np.float64).reshape(M, 6), yaw_src=np.array([r["src"] for r in rows], np.int32),
             ego_xyz=None if waymo else np.concatenate([np.asarray(sensors, np.float64), np.full((F, 1), 1.8)], 1),
             prior_wlh=PRIOR_WLH, nms_group=NMS_GROUP, nms_thr=NMS_THR, names=[r.get("name", "") for r in rows])
    t.update(meta or {})
    return _freeze(t)


_RULE, _NMS, _CARS = {}, {}, {}


def rule_table(waymo):
    if waymo in _RULE:
        return _RULE[waymo]
    # nuScenes: one sensor per frame, at global magnitude; Waymo: the origin, whatever the frame
    sensors = [(0.0, 0.0)] * 4 if waymo else [(600.0, 1200.0), (1200.25, -600.5), (-9950.0, 10100.0), (np.nan, 1200.0)]
    rows = []

    def add(f, name, pu, pv, h, a, b, cls=0, src=1, fl=1, rect=None):
        """A record of extents a, b and axis angle h whose centre sees the sensor at (pu, pv) * scale in its own axes; the scale grows
        from case to case, so that no two cases of a frame stand in one place.  The pushed centre lies a little off the record's."""
        sx, sy = sensors[f]
        if not np.isfinite(sx):
            sx = 600.0
        hc, hs = np.cos(h), np.sin(h)                          # (h == 0.0: 1 and 0 exactly)
        k = 1.0 + 0.5 * sum(r["f"] == f for r in rows)
        cx, cy = sx - k * (pu * hc - pv * hs), sy - k * (pu * hs + pv * hc)
        r = [cx, cy, a, b, hc, hs] if rect is None else rect(cx, cy)
        rows.append(dict(f=f, name=name, pushed=(cx + 0.5, cy - 0.25), rect=r, src=src, fl=fl, cls=cls, score=0.3 + 0.001 * len(rows)))

    for f in range(3):
        for q, (pu, pv) in enumerate(((9.0, 7.0), (-9.0, 7.0), (-9.0, -7.0), (9.0, -7.0))):
            add(f, f"quadrant{q}", pu, pv, 0.3 + 1.1 * q + 0.2 * f, 3.1, 1.4)
            add(f, f"quadrant{q}_negated_axis", pu, pv, 0.3 + 1.1 * q + 0.2 * f + np.pi, 3.1, 1.4)
        for a in (0.25, THIN, 3.0):
            for b in (0.25, THIN, 1.5):
                add(f, f"extent_{a}_{b}", 6.0, -11.0, -0.7, a, b, cls=f % 2)
        add(f, "longer_than_the_class", 12.0, 5.0, 2.2, 5.2, 1.0)
        add(f, "wider_than_the_class", 12.0, 5.0, 2.2, 3.0, 2.4)
        add(f, "lane_yaw_kept", 5.0, 5.0, 0.4, 3.0, 1.2, src=0)
        add(f, "no_box", 5.0, 5.0, 0.4, 3.0, 1.2, fl=0)
        add(f, "class_below_the_table", 5.0, -6.0, 1.0, 3.0, 1.2, cls=-3.0)
        add(f, "class_above_the_table", 5.0, -6.0, 1.0, 3.0, 1.2, cls=77.0)
        add(f, "class_nan", 5.0, -6.0, 1.0, 3.0, 1.2, cls=np.nan)
        add(f, "other_class", 5.0, -6.0, 1.0, 3.0, 1.2, cls=2)
        add(f, "rect_nan_extent", 5.0, 5.0, 0.4, np.nan, 1.2)
        add(f, "rect_inf_centre", 5.0, 5.0, 0.4, 3.0, 1.2, rect=lambda cx, cy: [np.inf, cy, 3.0, 1.2, np.cos(0.4), np.sin(0.4)])
        add(f, "rect_nan_axis", 5.0, 5.0, 0.4, 3.0, 1.2, rect=lambda cx, cy: [cx, cy, 3.0, 1.2, np.nan, np.sin(0.4)])
        # pu == 0 and pv == 0 exactly: an axis-aligned record whose centre has the sensor's x, or its y, to the bit
        add(f, "pu_zero", 0.0, 7.0 if f % 2 else -7.0, 0.0, 3.0, 1.5)
        add(f, "pv_zero", -7.0 if f % 2 else 7.0, 0.0, 0.0, 3.0, 1.5)
    if not waymo:
        for q, (pu, pv) in enumerate(((9.0, 7.0), (-9.0, -7.0))):
            add(3, f"nan_sensor{q}", pu, pv, 0.3, 3.1, 1.4)
    _RULE[waymo] = _table(rows, sensors, waymo)
    return _RULE[waymo]


def nms_table(waymo):
    if waymo in _NMS:
        return _NMS[waymo]
    rng = np.random.default_rng(11 + int(waymo))
    sensors = [(0.0, 0.0) if waymo else (600.0 + 50.0 * f, 1200.0) for f in range(len(FRAME_SIZES))]
    rows, pairs = [], []
    scores = (0.2, 0.35, 0.35, 0.5, 0.5, 0.5, 0.8, 0.9)
    base = 0
    for f, n in enumerate(FRAME_SIZES):
        sx, sy = sensors[f]
        ox, oy = sx + 20.0, sy + 30.0
        fr = []

        def unplaced(x, y, score, cls=3, fl=1):
            fr.append(dict(f=f, pushed=(x, y), rect=[0.0] * 6, src=0, fl=fl, cls=cls, score=score))

        def placed(px, py, cx, cy, score, cls=3):
            """axis-aligned, extents = the class's: du == dv == 0 and the placed centre is the record's to the bit"""
            fr.append(dict(f=f, pushed=(px, py), rect=[cx, cy, PRIOR_WLH[cls, 1], PRIOR_WLH[cls, 0], 1.0, 0.0], src=1, fl=1, cls=cls, score=score))

        def pair(goes):
            pairs.append((base + len(fr) - 2, base + len(fr) - 1, goes))
        if n == 2:                                             # the smallest frame that can suppress: exactly on the threshold, equal scores
            unplaced(ox, oy, 0.5); unplaced(ox + 2.0, oy, 0.5)
            pairs.append((base + 1, base, True))               # (the tie goes to the higher index)
        if n >= 63:
            far = 300.0
            for i, (to, goes) in enumerate(((None, True), (-np.inf, True), (np.inf, False))):
                # 2 m apart: dist^2 == 4.0 == the threshold; one ulp of the coordinate nearer or farther: the difference of two
                # neighbouring doubles is exact, and (2 -+ ulp)^2 rounds to a double below or above 4
                x0 = ox + far + 64.0 * i
                x1 = x0 + 2.0 if to is None else np.nextafter(x0 + 2.0, to)
                unplaced(x0, oy, 0.9); unplaced(x1, oy, 0.7); pair(goes)
            # pushed centres 10 m apart, placed centres 1 m apart: merged by the placement; and the converse
            placed(ox + far, oy + 100.0, ox + far, oy + 200.0, 0.9); placed(ox + far + 10.0, oy + 100.0, ox + far + 1.0, oy + 200.0, 0.6); pair(True)
            placed(ox + far, oy + 300.0, ox + far, oy + 400.0, 0.9); placed(ox + far + 1.0, oy + 300.0, ox + far + 10.0, oy + 400.0, 0.6); pair(False)
        while len(fr) < n:
            k = len(fr)
            x, y = ox + rng.uniform(-15.0, 15.0), oy + rng.uniform(-15.0, 15.0)
            cls, sc, fl = int(rng.integers(0, 3)), scores[int(rng.integers(0, len(scores)))], int(k % 9 != 4)
            if k % 3 == 0:
                h = rng.uniform(-np.pi, np.pi)
                fr.append(dict(f=f, pushed=(x, y), rect=[x + rng.uniform(-1, 1), y + rng.uniform(-1, 1), rng.uniform(0.2, 5.0), rng.uniform(0.0, 2.2),
                                                         np.cos(h), np.sin(h)], src=1, fl=fl, cls=cls, score=sc))
            else:
                unplaced(x, y, sc, cls, fl)
        if n > 64:                                             # the ten designed masks last: they straddle or lie beyond the 64th mask
            fr = fr[10:] + fr[:10]
            pairs[-5:] = [(i + n - 10, j + n - 10, g) for i, j, g in pairs[-5:]]
        rows += fr
        base += len(fr)
    _NMS[waymo] = _table(rows, sensors, waymo, dict(pairs=pairs))
    return _NMS[waymo]


# ------------------------------------------------------------------------------------------------ (c) visible-face cars
def cars(faces):
    """faces 2: the long and the short face that look at the sensor, meeting in the sensor-side corner; 1: the long one alone.  A list
    of (xyz (n, 4) float32 in list order, true centre (2,), sensor (2,), yaw); centres at global magnitude.  A geometry whose sensor is
    nearer than MARGIN to the slab of a shown face is left out (it would look along that face): fixed by this table, not by results."""
    if faces in _CARS:
        return _CARS[faces]
    out = []
    centre = np.array([600.0, 1200.0])
    for yaw in CAR_YAWS:
        c, s = np.cos(yaw), np.sin(yaw)
        for az in AZIMUTHS:
            for rng_m in RANGES:
                sensor = centre + rng_m * np.array([np.cos(az), np.sin(az)])
                e = sensor - centre
                pu, pv = e[0] * c + e[1] * s, e[1] * c - e[0] * s
                if abs(pv) < CAR_W / 2 + MARGIN or (faces == 2 and abs(pu) < CAR_L / 2 + MARGIN):
                    continue
                n_long, n_short = 90, 60
                u = np.linspace(-CAR_L / 2, CAR_L / 2, n_long)
                v = np.full(n_long, np.sign(pv) * CAR_W / 2)
                if faces == 2:
                    u = np.concatenate([u, np.full(n_short, np.sign(pu) * CAR_L / 2)])
                    v = np.concatenate([v, np.linspace(-CAR_W / 2, CAR_W / 2, n_short)])
                xy = np.stack([centre[0] + u * c - v * s, centre[1] + u * s + v * c], 1)
                xy = xy[np.random.default_rng(len(xy)).permutation(len(xy))]
                xyz = np.zeros((len(xy), 4), np.float32)
                xyz[:, :2], xyz[:, 2] = xy, 1.5
                xyz.setflags(write=False)
                out.append((xyz, centre.copy(), sensor, float(yaw)))
    _CARS[faces] = out
    return out


N_GEOMETRIES = len(CAR_YAWS) * len(AZIMUTHS) * len(RANGES)      # 984
CARS_LEFT = {2: 764, 1: 908}                                    # of them remain


def placed_bound(K, d0=0.05):
    """(pi / 2K + asin(d0 / CAR_L)) * (CAR_L + CAR_W): bev_fit_cases.known_answer_bound, the angle the fit can be off by, times the lever
    of the corner -- no point of the box is farther from the anchor than CAR_L + CAR_W.  Derived, not measured."""
    from tests.bev_fit_cases import known_answer_bound
    return known_answer_bound(K, CAR_L, d0) * (CAR_L + CAR_W)
