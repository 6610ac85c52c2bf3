"""Waymo 3D detection metrics: a native stand-in for waymo-open-dataset's `compute_detection_metrics_main`.

The binary (mmdetection3d's build) reads two `metrics_pb2.Objects` files and prints mAP / mAPH for 32 breakdowns:
OBJECT_TYPE x {VEHICLE, PEDESTRIAN, SIGN, CYCLIST} and RANGE x type x {[0, 30), [30, 50), [50, +inf)}, each at LEVEL_1
and LEVEL_2.  The rules restated here were pinned against that binary's printed output (tests/golden/g11_waymo_metrics.*):

  - frames are (context_name, frame_timestamp_micros); a frame in one file only still counts (all FP / all FN);
  - ground truth with num_lidar_points_in_box == 0 is dropped; the level is detection_difficulty_level when set (1, 2),
    else LEVEL_2 for at most 5 points and LEVEL_1 above;
  - range = 3D distance of the box centre from the origin; a box at exactly 30 (50) m is in the upper bucket; a
    prediction is sharded by its own range, like the ground truth;
  - score cutoffs float32(i * 0.01), i = 0..100; a prediction takes part when score >= cutoff;
  - per (frame, breakdown shard, cutoff) ONE maximum-weight matching of predictions and ground truth on 3D IoU
    (vehicle 0.7, the other types 0.5; weight = int(IoU x 1e6), pairs below the threshold never match), shared by
    both levels: TP = matched predictions, FP = unmatched predictions, FN = unmatched ground truth of level <= L;
  - heading accuracy of a match 1 - |d| / pi, d the float32 heading difference wrapped to [-pi, pi];
  - precision / recall per cutoff in float32 (0 when the denominator is 0); AP by Waymo's rule (see
    mean_average_precision); APH likewise with the heading-weighted precision and the plain recall.

`evaluate` runs the matching and counting on the GPU (cm3d_waymo_metrics, one call for the whole file);
`evaluate_host` restates the same computation in numpy / scipy for CPU tests.  Both finish on the host: AP / APH
are a few hundred numbers.
"""
import math

import numpy as np

TYPES = ("VEHICLE", "PEDESTRIAN", "SIGN", "CYCLIST")            # label_pb2.Label.Type 1..4
RANGES = ("[0, 30)", "[30, 50)", "[50, +inf)")
IOU_THR = {1: 0.7, 2: 0.5, 3: 0.5, 4: 0.5}
N_CUTOFFS = 101
CUTOFFS = np.array([i * 0.01 for i in range(N_CUTOFFS)], np.float32)
N_BREAKDOWNS = 16            # (type - 1) * 4 + shard; shard 0: all ranges, 1..3: range buckets
HEADING_SCALE = float(1 << 32)     # heading accuracy sums are fixed point, 2^-32 units (matches the kernel)
BOX_STRIDE = 8               # cx, cy, length, width, cos(heading), sin(heading), cz, height (float64)
IOU_KMAX = 1000000


# ------------------------------------------------------------------------------------------------ protobuf
def _rd_varint(b, i):
    v, sh = 0, 0
    while True:
        c = b[i]
        i += 1
        v |= (c & 0x7F) << sh
        sh += 7
        if not c & 0x80:
            return v, i


def _fields(b):
    i, out = 0, []
    while i < len(b):
        key, i = _rd_varint(b, i)
        f, w = key >> 3, key & 7
        if w == 0:
            v, i = _rd_varint(b, i)
        elif w == 1:
            v = float(np.frombuffer(b[i:i + 8], np.float64)[0])
            i += 8
        elif w == 5:
            v = float(np.frombuffer(b[i:i + 4], np.float32)[0])
            i += 4
        elif w == 2:
            n, i = _rd_varint(b, i)
            v = bytes(b[i:i + n])
            i += n
        else:
            raise ValueError(f"unsupported protobuf wire type {w}")
        out.append((f, v))
    return out


def decode_objects(blob):
    """metrics_pb2.Objects -> list of dicts, ground-truth fields included.  Missing fields take their proto defaults:
    score 0, num_lidar_points_in_box 0, detection_difficulty_level 0 (UNKNOWN).  Field numbers (public protos):
    Object object=1 score=2 context_name=4 frame_timestamp_micros=5; Label box=1 type=3 id=4
    detection_difficulty_level=5 num_lidar_points_in_box=7; Box center_x..heading = 1..7 (width=4, length=5)."""
    objs = []
    for f, payload in _fields(blob):
        if f != 1:
            continue
        o = dict(_fields(payload))
        label = dict(_fields(o.get(1, b"")))
        box = dict(_fields(label.get(1, b"")))
        objs.append(dict(center=[box.get(1, 0.0), box.get(2, 0.0), box.get(3, 0.0)], width=box.get(4, 0.0), length=box.get(5, 0.0),
                         height=box.get(6, 0.0), heading=box.get(7, 0.0), type=int(label.get(3, 0)),
                         id=label.get(4, b"").decode(), score=float(o.get(2, 0.0)), context_name=o.get(4, b"").decode(),
                         timestamp_micros=int(o.get(5, 0)), num_lidar_points_in_box=int(label.get(7, 0)),
                         detection_difficulty_level=int(label.get(5, 0))))
    return objs


def encode_gt_object(center, length, width, height, heading, type_id, context_name, timestamp_micros, num_points,
                     difficulty=None, object_id="gt"):
    """One ground-truth metrics_pb2.Object (no score) with num_lidar_points_in_box and, if given,
    detection_difficulty_level."""
    from .waymo import _double, _key, _ld, _varint
    box = (_double(1, center[0]) + _double(2, center[1]) + _double(3, center[2]) + _double(4, width) + _double(5, length) +
           _double(6, height) + _double(7, heading))
    label = _ld(1, box) + _key(3, 0) + _varint(type_id) + _ld(4, object_id.encode())
    if difficulty is not None:
        label += _key(5, 0) + _varint(difficulty)
    label += _key(7, 0) + _varint(num_points)
    return _ld(1, label) + _ld(4, context_name.encode()) + _key(5, 0) + _varint(timestamp_micros)


def read_objects(path):
    with open(path, "rb") as f:
        return decode_objects(f.read())


# ------------------------------------------------------------------------------------------------ packing
def _records(objs):
    n = len(objs)
    rec = np.zeros((n, BOX_STRIDE), np.float64)
    head = np.zeros(n, np.float32)
    typ = np.zeros(n, np.int32)
    dist = np.zeros(n, np.float64)
    if n:
        c = np.array([o["center"] for o in objs], np.float64)
        hd = np.array([o["heading"] for o in objs], np.float64)
        rec[:, 0], rec[:, 1] = c[:, 0], c[:, 1]
        rec[:, 2] = [o["length"] for o in objs]
        rec[:, 3] = [o["width"] for o in objs]
        rec[:, 4], rec[:, 5] = np.cos(hd), np.sin(hd)
        rec[:, 6] = c[:, 2]
        rec[:, 7] = [o["height"] for o in objs]
        head[:] = hd.astype(np.float32)
        typ[:] = [o["type"] for o in objs]
        dist = np.sqrt(c[:, 0] * c[:, 0] + c[:, 1] * c[:, 1] + c[:, 2] * c[:, 2])
    return rec, head, typ, dist


def gt_level(o):
    """Difficulty of a ground-truth object: its detection_difficulty_level when set, else LEVEL_2 for at most 5 lidar
    points and LEVEL_1 above."""
    lv = int(o["detection_difficulty_level"])
    if lv:
        return lv
    return 2 if o["num_lidar_points_in_box"] <= 5 else 1


def _range_shard(dist):
    return np.where(dist < 30.0, 1, np.where(dist < 50.0, 2, 3)).astype(np.int32)


def arrays_from_objects(pred_objects, gt_objects):
    """Decoded Objects -> the flat arrays of pack_arrays (ground truth without lidar points dropped, levels resolved)."""
    keys = {}
    for o in pred_objects:
        keys.setdefault((o["context_name"].encode(), int(o["timestamp_micros"])), None)
    gts = [o for o in gt_objects if o["num_lidar_points_in_box"] > 0]
    for o in gts:
        keys.setdefault((o["context_name"].encode(), int(o["timestamp_micros"])), None)
    frame_of = {k: i for i, k in enumerate(sorted(keys))}
    prec, phead, ptyp, pdist = _records(pred_objects)
    grec, ghead, gtyp, gdist = _records(gts)
    pred = dict(box=prec, head=phead, type=ptyp, dist=pdist, score=np.array([o["score"] for o in pred_objects], np.float32),
                frame=np.array([frame_of[(o["context_name"].encode(), int(o["timestamp_micros"]))] for o in pred_objects], np.int64))
    gt = dict(box=grec, head=ghead, type=gtyp, dist=gdist, level=np.array([gt_level(o) for o in gts], np.int32),
              frame=np.array([frame_of[(o["context_name"].encode(), int(o["timestamp_micros"]))] for o in gts], np.int64))
    return pred, gt, len(frame_of)


def pack(pred_objects, gt_objects):
    """Decoded Objects -> the flat group layout of cm3d_waymo_metrics (see pack_arrays).  Frames are numbered in the
    order of the binary's std::map keys (context_name bytes, then timestamp)."""
    return pack_arrays(*arrays_from_objects(pred_objects, gt_objects))


def _expand(frame, typ, dist):
    """Every box goes to its type's shard 0 and to its range shard: (box index, group key) of the boxes of a known type."""
    n = frame.size
    idx = np.concatenate([np.arange(n), np.arange(n)])
    shard = np.concatenate([np.zeros(n, np.int32), _range_shard(dist)])
    t = np.clip(np.concatenate([typ, typ]), 1, 4)
    gkey = np.concatenate([frame, frame]).astype(np.int64) * N_BREAKDOWNS + (t - 1) * 4 + shard
    ok = np.concatenate([(typ >= 1) & (typ <= 4)] * 2)
    return idx[ok], gkey[ok]


def pack_arrays(pred, gt, n_frames):
    """Per-box arrays -> groups.  pred: box (n, BOX_STRIDE), head float32, type, dist (distance of the centre from the
    origin), score float32, frame; gt: the same with level (1, 2) instead of score.  A group is (frame, type, shard):
    shard 0 holds every box of the type, shards 1..3 the boxes of one range bucket; groups are ordered by frame, then
    breakdown, predictions in a group by descending score (stable)."""
    ptyp, gtyp = pred["type"], gt["type"]
    bad = int(np.sum((ptyp < 1) | (ptyp > 4)) + np.sum((gtyp < 1) | (gtyp > 4)))
    pidx, pkey = _expand(pred["frame"], ptyp, pred["dist"])
    gidx, gkey = _expand(gt["frame"], gtyp, gt["dist"])
    order = np.lexsort((pidx, -pred["score"][pidx].astype(np.float64), pkey))
    pidx, pkey = pidx[order], pkey[order]
    order = np.lexsort((gidx, gkey))
    gidx, gkey = gidx[order], gkey[order]
    ukeys = np.unique(np.concatenate([pkey, gkey]))
    pred_off = np.concatenate([np.searchsorted(pkey, ukeys, "left"), [pkey.size]]).astype(np.int64)
    gt_off = np.concatenate([np.searchsorted(gkey, ukeys, "left"), [gkey.size]]).astype(np.int64)
    return dict(n_frames=int(n_frames), group_bd=(ukeys % N_BREAKDOWNS).astype(np.int32), group_frame=(ukeys // N_BREAKDOWNS),
                pred_off=pred_off, gt_off=gt_off, pred_box=pred["box"][pidx], pred_head=pred["head"][pidx],
                pred_score=pred["score"][pidx], gt_box=gt["box"][gidx], gt_head=gt["head"][gidx], gt_level=gt["level"][gidx],
                bad_type=bad)


# ------------------------------------------------------------------------------------------------ host restatement
def _clip_area(a, b):
    """Vectorised bev intersection area of record rows a, b (same algorithm and operation order as bev_inter_area in
    cm3d_amd/csrc/bev_iou.h: clip A against B's edges in coordinates relative to A's centre)."""
    n = a.shape[0]
    out = np.zeros(n)
    dx, dy = b[:, 0] - a[:, 0], b[:, 1] - a[:, 1]
    ra2, rb2 = a[:, 2] * a[:, 2] + a[:, 3] * a[:, 3], b[:, 2] * b[:, 2] + b[:, 3] * b[:, 3]
    r = 0.5 * (np.sqrt(ra2) + np.sqrt(rb2))
    live = ~(dx * dx + dy * dy > r * r)
    if not live.any():
        return out
    a, b = a[live], b[live]
    m = a.shape[0]

    def corners(bb, ox, oy):
        hl, hw, c, s = bb[:, 2] * 0.5, bb[:, 3] * 0.5, bb[:, 4], bb[:, 5]
        ddx, ddy = bb[:, 0] - ox, bb[:, 1] - oy
        lc, ls, wc, wsn = hl * c, hl * s, hw * c, hw * s
        X = np.stack([(ddx + lc) - wsn, (ddx - lc) - wsn, (ddx - lc) + wsn, (ddx + lc) + wsn], 1)
        Y = np.stack([(ddy + ls) + wc, (ddy - ls) + wc, (ddy - ls) - wc, (ddy + ls) - wc], 1)
        return X, Y
    px, py = corners(a, a[:, 0], a[:, 1])
    bx, by = corners(b, a[:, 0], a[:, 1])
    W = 20          # clip buffer slots: one clip of an n-gon emits at most floor(1.5 n) vertices, 4 -> 6 -> 9 -> 13 -> 19
    PX, PY = np.zeros((m, W)), np.zeros((m, W))
    PX[:, :4], PY[:, :4] = px, py
    cnt = np.full(m, 4)
    rows = np.arange(m)
    for e in range(4):
        x1, y1 = bx[:, e], by[:, e]
        ex, ey = bx[:, (e + 1) & 3] - x1, by[:, (e + 1) & 3] - y1
        QX, QY = np.zeros((m, W)), np.zeros((m, W))
        k = np.zeros(m, np.int64)
        prx, pry = PX[rows, np.maximum(cnt - 1, 0)], PY[rows, np.maximum(cnt - 1, 0)]
        dp = ex * (pry - y1) - ey * (prx - x1)
        for i in range(int(cnt.max())):                # every input vertex
            act = i < cnt
            cx, cy = PX[:, i], PY[:, i]
            dc = ex * (cy - y1) - ey * (cx - x1)
            cross = act & ((dc >= 0.0) != (dp >= 0.0))
            with np.errstate(divide="ignore", invalid="ignore"):
                t = dp / (dp - dc)
                ix, iy = prx + t * (cx - prx), pry + t * (cy - pry)
            r_ = rows[cross]
            QX[r_, k[cross]], QY[r_, k[cross]] = ix[cross], iy[cross]
            k += cross
            ins = act & (dc >= 0.0)
            r_ = rows[ins]
            QX[r_, k[ins]], QY[r_, k[ins]] = cx[ins], cy[ins]
            k += ins
            prx, pry, dp = np.where(act, cx, prx), np.where(act, cy, pry), np.where(act, dc, dp)
        cnt = np.where(cnt > 0, k, 0)
        PX, PY = QX, QY
    acc = np.zeros(m)
    for i in range(W):
        j = np.where(i + 1 >= cnt, 0, i + 1)
        act = i < cnt
        acc = np.where(act, acc + (PX[:, i] * PY[rows, j] - PX[rows, j] * PY[:, i]), acc)
    area = np.where(cnt >= 3, 0.5 * np.abs(acc), 0.0)
    out[live] = area
    return out


def iou3d(a, b):
    """3D IoU of record rows a, b (BOX_STRIDE layout), as k_wm_weights computes it."""
    a, b = np.atleast_2d(a), np.atleast_2d(b)
    va, vb = a[:, 2] * a[:, 3] * a[:, 7], b[:, 2] * b[:, 3] * b[:, 7]
    ok = (a[:, 2] * a[:, 3] > 0.0) & (b[:, 2] * b[:, 3] > 0.0) & (a[:, 7] > 0.0) & (b[:, 7] > 0.0)
    inter = _clip_area(a, b)
    zlo = np.maximum(a[:, 6] - 0.5 * a[:, 7], b[:, 6] - 0.5 * b[:, 7])
    zhi = np.minimum(a[:, 6] + 0.5 * a[:, 7], b[:, 6] + 0.5 * b[:, 7])
    inter = inter * np.maximum(zhi - zlo, 0.0)
    uni = (va + vb) - inter
    with np.errstate(divide="ignore", invalid="ignore"):
        iou = np.where(ok & (uni > 0.0), inter / uni, 0.0)
    return np.minimum(iou, 1.0)


def heading_accuracy_fixed(pd_head, gt_head):
    """Heading accuracy of matched pairs (float32 headings) in 2^-32 fixed point, as the kernel computes it."""
    d = (np.asarray(gt_head, np.float32) - np.asarray(pd_head, np.float32)).astype(np.float32).astype(np.float64)
    d = np.abs(np.remainder(d + math.pi, 2.0 * math.pi) - math.pi).astype(np.float32).astype(np.float64)
    d = np.where(d > math.pi, (2.0 * math.pi - d).astype(np.float32).astype(np.float64), d)
    acc = np.clip(1.0 - d / math.pi, 0.0, 1.0).astype(np.float32).astype(np.float64)
    return np.rint(acc * HEADING_SCALE).astype(np.int64)


def _cutoff_counts(scores_desc):
    """k(c) = number of predictions with score >= cutoff c, for scores sorted in descending order."""
    return np.searchsorted(-scores_desc.astype(np.float32), -CUTOFFS, side="right")


_PAIR_CHUNK = 1 << 15          # pairs per vectorised iou3d call of pair_weights
_SMALL_PAIRS = 4               # counts_host: groups with one box on a side and at most this many pairs skip scipy


def pair_weights(packed):
    """Integer weights of all pairs of all groups, as k_wm_weights writes them: group g's (P, G) matrix is
    w[pair_off[g]:pair_off[g + 1]], row-major.  Returns (w int64, pair_off).  A pair of equal boxes is clipped once: every
    pair of a range shard is also a pair of its type's shard 0."""
    po, go = packed["pred_off"], packed["gt_off"]
    P, G = np.diff(po), np.diff(go)
    pair_off = np.concatenate([[0], np.cumsum(P * G)]).astype(np.int64)
    w = np.zeros(int(pair_off[-1]), np.int64)
    thr_of = np.array([IOU_THR[bd // 4 + 1] for bd in range(N_BREAKDOWNS)])
    pid = np.unique(packed["pred_box"], axis=0, return_inverse=True)[1].reshape(-1).astype(np.int64)
    gid = np.unique(packed["gt_box"], axis=0, return_inverse=True)[1].reshape(-1).astype(np.int64)
    for lo in range(0, w.size, _PAIR_CHUNK):
        q = np.arange(lo, min(lo + _PAIR_CHUNK, w.size))
        g = np.searchsorted(pair_off, q, "right") - 1
        loc = q - pair_off[g]
        i, j = po[g] + loc // G[g], go[g] + loc % G[g]
        _, first, inv = np.unique(pid[i] * (gid.size + 1) + gid[j], return_index=True, return_inverse=True)
        iou = iou3d(packed["pred_box"][i[first]], packed["gt_box"][j[first]])[inv.reshape(-1)]
        w[q] = np.where(iou >= thr_of[packed["group_bd"][g]], (iou * IOU_KMAX).astype(np.int64), 0)
    return w, pair_off


def _small_groups(packed, w_all, pair_off, counts, hsum):
    """counts_host for the groups that need no assignment solver, all at once: a side empty, or one box on a side, at most
    _SMALL_PAIRS pairs and a unique largest weight in every prefix of the rows (the optimum is then that one pair).
    Adds to counts / hsum and returns the mask of the groups it took."""
    po, go, bd = packed["pred_off"], packed["gt_off"], packed["group_bd"].astype(np.int64)
    P, G = np.diff(po), np.diff(go)
    n = P.size
    # K[g, c]: predictions of group g with score >= cutoff c
    adm = np.searchsorted(CUTOFFS, packed["pred_score"].astype(np.float32), "right")
    K = np.zeros((n, N_CUTOFFS + 1), np.int32)
    np.add.at(K, (np.repeat(np.arange(n), P), adm), 1)
    K = (K[:, ::-1].cumsum(1)[:, ::-1])[:, 1:]
    lvl1 = np.zeros(packed["gt_level"].size + 1, np.int64)
    lvl1[1:] = np.cumsum(packed["gt_level"] == 1)
    n1 = lvl1[go[1:]] - lvl1[go[:-1]]
    taken = np.zeros(n, bool)

    def add(sel, tp, hs, fn1, fn2):      # per group and k = 0..kmax: (m, kmax + 1) tables, looked up by K
        k = K[sel].astype(np.int64)
        t = np.take_along_axis(tp, k, 1)
        rows = np.stack([t, k - t, np.take_along_axis(fn1, k, 1), np.take_along_axis(fn2, k, 1)], 2)
        h = np.take_along_axis(hs, k, 1)
        for b in np.unique(bd[sel]):
            of = bd[sel] == b
            counts[b] += rows[of].sum(0)
            hsum[b] += h[of].sum(0)
        taken[sel] = True
    for p, g in sorted({(int(a), int(b_)) for a, b_ in zip(P, G)}):
        sel = np.flatnonzero((P == p) & (G == g))
        m = sel.size
        z = np.zeros((m, p + 1), np.int64)
        if p == 0 or g == 0:
            add(sel, z, z, z + n1[sel][:, None], z + g)
            continue
        if min(p, g) > 1 or p * g > _SMALL_PAIRS:
            continue
        w = w_all[pair_off[sel][:, None] + np.arange(p * g)[None, :]]
        tp, hs, fn1, fn2 = z.copy(), z.copy(), z + n1[sel][:, None], z + g
        unique = np.ones(m, bool)
        for k in range(1, p + 1):
            sub = w[:, :k * g]
            best = sub.max(1)
            at = sub.argmax(1)
            unique &= (best == 0) | ((sub == best[:, None]).sum(1) == 1)
            hit = best > 0
            r, c = po[sel] + at // g, go[sel] + at % g
            tp[:, k] = hit
            hs[:, k] = np.where(hit, heading_accuracy_fixed(packed["pred_head"][r], packed["gt_head"][c]), 0)
            fn1[:, k] -= hit & (packed["gt_level"][c] == 1)
            fn2[:, k] -= hit
        add(sel[unique], tp[unique], hs[unique], fn1[unique], fn2[unique])
    return taken


def counts_host(packed, weights=None):
    """Host restatement of cm3d_waymo_metrics: counts int64[16][101][4] (TP, FP, FN L1, FN L2) and heading sums
    int64[16][101] (fixed point).  Matching by scipy's linear_sum_assignment on the integer weights (max weight); groups
    whose optimum is a single pair with a unique largest weight are counted without it (_small_groups).  weights: the
    result of pair_weights(packed), if the caller has it."""
    from scipy.optimize import linear_sum_assignment
    counts = np.zeros((N_BREAKDOWNS, N_CUTOFFS, 4), np.int64)
    hsum = np.zeros((N_BREAKDOWNS, N_CUTOFFS), np.int64)
    po, go = packed["pred_off"], packed["gt_off"]
    w_all, pair_off = weights if weights is not None else pair_weights(packed)
    taken = _small_groups(packed, w_all, pair_off, counts, hsum)
    for g in np.flatnonzero(~taken):
        bd = int(packed["group_bd"][g])
        p0, p1, g0, g1 = int(po[g]), int(po[g + 1]), int(go[g]), int(go[g + 1])
        P, G = p1 - p0, g1 - g0
        lvl = packed["gt_level"][g0:g1]
        ks = _cutoff_counts(packed["pred_score"][p0:p1])
        w = w_all[pair_off[g]:pair_off[g + 1]].reshape(P, G)
        for k in np.unique(ks):
            sel = ks == k
            tp, hs, fn1, fn2 = 0, 0, int(np.sum(lvl == 1)), G
            if k and G:
                r, c = linear_sum_assignment(w[:k], maximize=True)
                keep = w[:k][r, c] > 0
                r, c = r[keep], c[keep]
                tp = r.size
                hs = int(heading_accuracy_fixed(packed["pred_head"][p0 + r], packed["gt_head"][g0 + c]).sum())
                matched = np.zeros(G, bool)
                matched[c] = True
                fn1, fn2 = int(np.sum((lvl == 1) & ~matched)), int(np.sum(~matched))
            counts[bd, sel] += np.array([tp, int(k) - tp, fn1, fn2], np.int64)
            hsum[bd, sel] += hs
    return counts, hsum


# ------------------------------------------------------------------------------------------------ alpha sweep
def pack_candidates(cand_objects, kind, p, s, gt_objects):
    """The candidate superset of the SAM3D fusion grid search (fusion.waymo_candidates) -> the group layout of
    cm3d_waymo_metrics_sweep.  cand_objects are decoded-Object-like dicts (center, length, width, height, heading, type,
    context_name, timestamp_micros) in candidate order, kind / p / s as in include/cm3d_hip.h.  Groups are pack_arrays' groups
    with candidates in the place of predictions: every candidate goes to shard 0 and to its own range shard (the two boxes
    of a pair may differ there), frames are the union of candidate and ground-truth keys, ground truth without lidar
    points is dropped; inside a group candidates keep candidate order.  group_static marks the groups of kind 0 only."""
    kind = np.asarray(kind, np.int32)
    pred, gt, n_frames = arrays_from_objects([dict(o, score=0.0) for o in cand_objects], gt_objects)
    ctyp, gtyp = pred["type"], gt["type"]
    bad = int(np.sum((ctyp < 1) | (ctyp > 4)) + np.sum((gtyp < 1) | (gtyp > 4)))
    cidx, ckey = _expand(pred["frame"], ctyp, pred["dist"])
    gidx, gkey = _expand(gt["frame"], gtyp, gt["dist"])
    order = np.lexsort((cidx, ckey))
    cidx, ckey = cidx[order], ckey[order]
    order = np.lexsort((gidx, gkey))
    gidx, gkey = gidx[order], gkey[order]
    ukeys = np.unique(np.concatenate([ckey, gkey]))
    cand_off = np.concatenate([np.searchsorted(ckey, ukeys, "left"), [ckey.size]]).astype(np.int64)
    gt_off = np.concatenate([np.searchsorted(gkey, ukeys, "left"), [gkey.size]]).astype(np.int64)
    moving = np.concatenate([[0], np.cumsum(kind[cidx] != 0)])
    return dict(n_frames=int(n_frames), group_bd=(ukeys % N_BREAKDOWNS).astype(np.int32), group_frame=(ukeys // N_BREAKDOWNS),
                cand_off=cand_off, gt_off=gt_off, cand_box=pred["box"][cidx], cand_head=pred["head"][cidx], cand_kind=kind[cidx],
                cand_p=np.asarray(p, np.float64)[cidx], cand_s=np.asarray(s, np.float64)[cidx], cand_index=cidx,
                gt_box=gt["box"][gidx], gt_head=gt["head"][gidx], gt_level=gt["level"][gidx],
                group_static=(moving[cand_off[1:]] == moving[cand_off[:-1]]).astype(np.int32), bad_type=bad)


def candidate_scores(kind, p, s, alpha):
    """(active, float32 score) of candidates at one alpha, the rule of fusion.fuse_waymo: s * alpha in float64, compared
    unclipped with p, then clipped to [0, 1] and rounded once to float32."""
    prod = s * float(alpha)
    sam = prod > p
    active = (kind == 0) | (kind == 1) | ((kind == 2) & ~sam) | ((kind == 3) & sam)
    score = np.where((kind == 0) | (kind == 2), p, np.clip(prod, 0, 1)).astype(np.float32)
    return active, score


def counts_sweep_host(packed_candidates, alphas):
    """Host restatement of cm3d_waymo_metrics_sweep: (counts int64[A][16][101][4], hsum int64[A][16][101]).  Per alpha the
    active candidates of every group are sorted (descending score, then candidate order) and counted by counts_host; the
    weights of all candidates x ground truth are computed once and their rows gathered."""
    pc = packed_candidates
    co, go = pc["cand_off"], pc["gt_off"]
    full = dict(pred_off=co, gt_off=go, pred_box=pc["cand_box"], gt_box=pc["gt_box"], group_bd=pc["group_bd"])
    w_full, pair_off = pair_weights(full)
    n_groups = co.size - 1
    group_of = np.repeat(np.arange(n_groups), np.diff(co))
    G = np.diff(go)
    counts = np.zeros((len(alphas), N_BREAKDOWNS, N_CUTOFFS, 4), np.int64)
    hsum = np.zeros((len(alphas), N_BREAKDOWNS, N_CUTOFFS), np.int64)
    pos = np.arange(group_of.size)
    for a, alpha in enumerate(alphas):
        active, score = candidate_scores(pc["cand_kind"], pc["cand_p"], pc["cand_s"], alpha)
        sel = np.flatnonzero(active)
        sel = sel[np.lexsort((pos[sel], -score[sel].astype(np.float64), group_of[sel]))]
        pred_off = np.concatenate([[0], np.cumsum(np.bincount(group_of[sel], minlength=n_groups))]).astype(np.int64)
        g_sel = group_of[sel]
        row0 = pair_off[g_sel] + (sel - co[g_sel]) * G[g_sel]             # the candidate's row of its group's weight matrix
        reps = G[g_sel]
        src = np.repeat(row0, reps) + (np.arange(int(reps.sum())) - np.repeat(np.cumsum(reps) - reps, reps))
        w_off = np.concatenate([[0], np.cumsum(np.diff(pred_off) * G)]).astype(np.int64)
        packed = dict(group_bd=pc["group_bd"], pred_off=pred_off, gt_off=go, pred_box=pc["cand_box"][sel],
                      pred_head=pc["cand_head"][sel], pred_score=score[sel], gt_box=pc["gt_box"], gt_head=pc["gt_head"],
                      gt_level=pc["gt_level"])
        counts[a], hsum[a] = counts_host(packed, weights=(w_full[src], w_off))
    return counts, hsum


# ------------------------------------------------------------------------------------------------ AP / APH, text
def mean_average_precision(precision, recall, max_recall_delta=0.05):
    """AP of one PR table, float32 like waymo-open-dataset's ComputeMeanAveragePrecision: a recall -> precision map
    (largest precision per recall, recall 0 seeded with precision 1); walked from the largest recall down with the
    running maximum precision, inserting a point every max_recall_delta where two recalls lie further apart; the
    point at recall 0 takes the precision of its neighbour; trapezoid rule, accumulated in double and rounded to
    float32 after every step."""
    f32 = np.float32
    delta = f32(max_recall_delta)
    m = {f32(0.0): f32(1.0)}
    for p, r in zip(np.asarray(precision, np.float32), np.asarray(recall, np.float32)):
        m[r] = max(m.get(r, f32(0.0)), p)
    keys = sorted(m)
    pr = []                     # (precision, recall), descending recall
    max_p = f32(0.0)
    cur = keys[0]
    k = len(keys) - 1
    gap_max = f32(f32(1e-6) + delta)
    while True:
        r = keys[k]
        if f32(cur - r) > gap_max:
            cur = f32(cur - delta)
            pr.append((max_p, cur))
            continue
        max_p = max(max_p, m[r])
        pr.append((max_p, r))
        cur = r
        if k == 0:
            break
        k -= 1
    if len(pr) >= 2:
        pr[-1] = (pr[-2][0], pr[-1][1])
    ap = f32(0.0)
    for (p0, r0), (p1, r1) in zip(pr[:-1], pr[1:]):
        ap = f32(float(f32(r0 - r1)) * 0.5 * float(f32(p0 + p1)) + float(ap))
    return float(ap)


def metrics_from_counts(counts, hsum):
    """(counts, hsum) -> {(breakdown, level): (mAP, mAPH)} with level 1, 2."""
    out = {}
    for bd in range(N_BREAKDOWNS):
        tp, fp = counts[bd, :, 0], counts[bd, :, 1]
        h = (hsum[bd].astype(np.float64) / HEADING_SCALE).astype(np.float32)
        with np.errstate(divide="ignore", invalid="ignore"):
            den_p = (tp + fp).astype(np.float32)
            prec = np.where(tp + fp > 0, tp.astype(np.float32) / np.where(den_p > 0, den_p, 1), 0).astype(np.float32)
            prec_h = np.where(tp + fp > 0, h / np.where(den_p > 0, den_p, 1), 0).astype(np.float32)
            for lv in (1, 2):
                fn = counts[bd, :, 1 + lv]
                den_r = (tp + fn).astype(np.float32)
                rec = np.where(tp + fn > 0, tp.astype(np.float32) / np.where(den_r > 0, den_r, 1), 0).astype(np.float32)
                out[(bd, lv)] = (mean_average_precision(prec, rec), mean_average_precision(prec_h, rec))
    return out


def breakdown_names():
    """The 32 names in the binary's print order."""
    names = []
    for t in range(4):
        for lv in (1, 2):
            names.append(((t * 4, lv), f"OBJECT_TYPE_TYPE_{TYPES[t]}_LEVEL_{lv}"))
    for t in range(4):
        for r in range(3):
            for lv in (1, 2):
                names.append(((t * 4 + 1 + r, lv), f"RANGE_TYPE_{TYPES[t]}_{RANGES[r]}_LEVEL_{lv}"))
    return names


def _g(x):
    return f"{x:g}"


def format_metrics(metrics):
    """The 32 breakdown lines, in the binary's order and number format (%g, 6 significant digits)."""
    return "".join(f"{name}: [mAP {_g(metrics[k][0])}] [mAPH {_g(metrics[k][1])}]\n" for k, name in breakdown_names())


def _finish(counts, hsum):
    from . import fusion
    text = format_metrics(metrics_from_counts(counts, hsum))
    return fusion.parse_waymo_metrics(text)[0], text


def evaluate_host(pred_objects, gt_objects):
    """numpy / scipy restatement of evaluate() (small inputs).  Returns (ap_dict, text)."""
    packed = pack(pred_objects, gt_objects)
    if packed["bad_type"]:
        raise ValueError("waymo metrics: object of unknown type")
    return _finish(*counts_host(packed))


def evaluate(pred_objects, gt_objects, per_cutoff=False):
    """GPU evaluation (one cm3d_waymo_metrics call) of decoded pred / gt Objects.  Returns (ap_dict, text): ap_dict as
    fusion.parse_waymo_metrics gives it for the binary's output, text the 32 breakdown lines.  per_cutoff=True matches
    every score cutoff on its own instead of once per distinct prediction subset (a check of the deduplication)."""
    return evaluate_packed(pack(pred_objects, gt_objects), per_cutoff)


def evaluate_packed(packed, per_cutoff=False):
    """evaluate() from pack() / pack_arrays() output."""
    from . import ops
    if packed["bad_type"]:
        raise ValueError("waymo metrics: object of unknown type")
    counts, hsum = ops.waymo_metrics(packed, per_cutoff=per_cutoff)
    return _finish(counts, hsum)


def evaluate_files(pred_path, gt_path, device=True):
    objs = read_objects(pred_path), read_objects(gt_path)
    return evaluate(*objs) if device else evaluate_host(*objs)

