"""Cases for the shared assignment solver (cm3d_amd/csrc/assign.h: AssignSolver, k_assign_block_owner, assign_locate).

The solver is reachable only through cm3d_bev_match (k_bev_assign) and cm3d_waymo_metrics (k_wm_match), so every case is a
set of boxes whose weight matrix has the wanted structure.  Pure numpy, seeded, no GPU.  Four families:

  dense   one tight cluster in which every pair overlaps: a dense, generic matrix, many dual updates per phase;
  chain   "domino": equal boxes on a line, prediction i halfway between ground truth i and i + 1, a shade nearer to i,
          and a last prediction on ground truth 0.  When it arrives the optimum shifts every earlier prediction from
          ground truth i to i + 1: ONE augmenting path through all columns with a dual update at every step;
  ties    all boxes identical: a constant 10^6 matrix, only the written tie rule decides;
  seams   very many groups of at most two pairs, empty ones between them, then dense groups whose pairs cross hundreds of
          256-pair blocks, then tiny groups again: the block-owner search and the walk of assign_locate.

BEV form (bev_cases, bev_seams; bev_call as one call's flat arrays): (n, 7) boxes [cx, cy, z, length, width, height, heading] for ops.bev_match / ops.match_records.
Waymo form (waymo_family): the pred / gt dicts of waymo_eval.pack_arrays, one frame per case; every box also lands in its
range shard, which gives shorter sub-groups of the same structure.
"""
import functools
import math

import numpy as np

FAMILIES = ("dense", "chain", "ties", "seams")
INSTANCES = (64, 128, 256, 1024)       # capacities of the launched AssignSolver instances (assign_instance_takes)
BM_LDS = 8192                          # fusion.hip: a sample of at most this many pairs is read from its LDS image
WM_LDS = 4096                          # waymo_metrics.hip: likewise for a group
BLOCK_PAIRS = 256                      # pairs per block of the weight kernels
KMAX = 1000000

# one size on each side of every instance limit, rectangular both ways (P > G is the transposed read of k_bev_assign)
DENSE_SIZES = [(63, 64), (64, 64), (65, 64), (64, 65), (128, 128), (129, 100), (100, 129), (256, 256), (257, 200), (200, 257),
               (1024, 1024), (1024, 300), (300, 1024)]
BEV_LDS_SEAM = [(64, 128), (128, 64), (64, 129), (129, 64)]       # 8192 pairs: LDS, one more row or column: L2
# Waymo form: (64, 64) and (65, 63) are 4096 pairs or fewer: LDS; (65, 64) is read from L2.
WM_DENSE_SIZES = DENSE_SIZES + [(65, 63)]
CHAIN_SIZES = (64, 65, 128, 129, 256, 257, 1024)
CHAIN_VARIANTS = ("square", "mid", "wide", "tall")
TIES_SIZES = [(1024, 1024), (1024, 1000), (257, 1024), (64, 64), (128, 100), (200, 256)]
WM_TIES_SIZES = TIES_SIZES


def instance_of(P, G):
    """Capacity of the solver instance that takes a (P, G) group."""
    big = max(P, G)
    return next(c for c in INSTANCES if big <= c)


def bev_read_paths(P, G):
    """Read paths of k_bev_assign on a (P, G) sample: 'lds' or 'l2', and 'tr' when it reads the matrix transposed."""
    return {"lds" if P * G <= BM_LDS else "l2"} | ({"tr"} if P > G else set())


def wm_read_path(P, G):
    return "lds" if P * G <= WM_LDS else "l2"


def pair_offsets(sizes):
    """pair_off of a call: exclusive prefix sum of P * G over its groups."""
    s = np.asarray(sizes, np.int64).reshape(-1, 2)
    return np.concatenate([[0], np.cumsum(s[:, 0] * s[:, 1])]).astype(np.int64)


def block_stats(pair_off):
    """(number of 256-pair blocks that hold pairs of at least two groups, number of empty groups that lie strictly inside a
    block, the largest number of groups with pairs in one block)."""
    sizes = np.diff(pair_off)
    live = np.flatnonzero(sizes > 0)
    first, last = pair_off[live] // BLOCK_PAIRS, (pair_off[live + 1] - 1) // BLOCK_PAIRS
    n_blocks = int((pair_off[-1] + BLOCK_PAIRS - 1) // BLOCK_PAIRS)
    per_block = np.zeros(n_blocks + 1, np.int64)
    np.add.at(per_block, first, 1)
    np.add.at(per_block, last + 1, -1)
    per_block = np.cumsum(per_block)[:n_blocks]
    empty = np.flatnonzero(sizes == 0)
    inside = int(np.sum((pair_off[empty] % BLOCK_PAIRS != 0) & (pair_off[empty] < pair_off[-1])))
    return int(np.sum(per_block >= 2)), inside, int(per_block.max()) if n_blocks else 0


# ---------------------------------------------------------------------------------------------------- BEV form
def _boxes7(cx, cy, length, width, heading, z=0.0, height=1.5):
    n = np.size(cx)
    b = np.empty((n, 7))
    b[:, 0], b[:, 1], b[:, 2], b[:, 3], b[:, 4], b[:, 5], b[:, 6] = cx, cy, z, length, width, height, heading
    return b


def bev_cluster(rng, n, centre=(0.0, 0.0)):
    """n boxes of one tight cluster: every pair overlaps with IoU above 0.2."""
    return _boxes7(centre[0] + rng.uniform(-0.6, 0.6, n), centre[1] + rng.uniform(-0.6, 0.6, n), rng.uniform(3.5, 5.5, n),
                   rng.uniform(1.6, 2.4, n), rng.uniform(-0.3, 0.3, n))


CHAIN_BEV = dict(L=4.0, W=2.0, d=5.0, eps=1e-4, last=-0.3)     # weights 230788 (strong), 230750 (weak), 860465 (last)
# The records are float32 (ops.match_records).  At pitch 5 the 1024 chain reaches x = 5120, where float32 steps by 4.9e-4
# and the 1e-4 offset rounds away.  The widest chain is therefore the same figure at four fifths of the size, with an
# offset and a last position that are powers of two: every x below 4096 is then exact in float32 and strong > weak at
# every step.  The offset cannot be larger: 1023 steps of (strong - weak), 116 each, must cost less than dropping
# prediction 0 outright (230 000), or the optimum does that and leaves the chain where it is.
CHAIN_BEV_WIDEST = dict(L=3.2, W=1.6, d=4.0, eps=2.0 ** -12, last=-0.25)


def chain_layout(n_chain, n_gt, last_row, L, W, d, eps, last):
    """x of the ground truth (n_gt boxes at pitch d) and of the predictions: n_chain chained ones in order, the last
    prediction (on ground truth 0) inserted as row last_row."""
    gx = np.arange(n_gt) * d
    px = np.arange(n_chain) * d + 0.5 * d - eps
    return gx, np.insert(px, last_row, last)


def bev_chain(n, variant):
    """Chain case of side n.  square: n - 1 chained predictions + the last one, n ground truth.  mid: the last prediction
    is row n // 2, so the re-route happens at an interior phase and the chain keeps growing after it.  wide: n - 2
    chained + last against n ground truth, so a column that nothing wants ends the path.  tall: wide with the sides
    swapped (P > G: the transposed read; the rows of the search are then the ground truth)."""
    c = CHAIN_BEV if n * CHAIN_BEV["d"] < 2048 else CHAIN_BEV_WIDEST
    n_chain = n - 1 if variant in ("square", "mid") else n - 2
    last_row = n // 2 if variant == "mid" else n_chain
    gx, px = chain_layout(n_chain, n, last_row, c["L"], c["W"], c["d"], c["eps"], c["last"])
    pred, gt = _boxes7(px, 0.0, c["L"], c["W"], 0.0), _boxes7(gx, 0.0, c["L"], c["W"], 0.0)
    # shifted[i]: the partner of row i after the re-route (chained row k -> column k + 1, the last row -> column 0)
    shifted = np.insert(np.arange(n_chain) + 1, last_row, 0)
    if variant == "tall":
        return dict(pred=gt, gt=pred, rows="gt", shifted=shifted, n_chain=n_chain)
    return dict(pred=pred, gt=gt, rows="pred", shifted=shifted, n_chain=n_chain)


def _tiny_sizes(rng, n):
    """n group sizes from (1,1), (1,2), (2,1), (0,k), (k,0), (0,0), mostly the two-pair ones, in random order."""
    kind = rng.choice(6, n, p=[0.1, 0.35, 0.35, 0.07, 0.07, 0.06])
    k = rng.integers(1, 4, n)
    P = np.choose(kind, [1, 1, 2, 0, k, 0])
    G = np.choose(kind, [1, 2, 1, k, 0, 0])
    return np.stack([P, G], 1)


SEAM_DENSE = [(300, 300), (100, 120), (200, 180)]      # the 1024, 128 and 256 column instances; 352 + 47 + 141 blocks
# A block holds 256 pairs and a tiny group at most 2, so 1000 blocks shared by several groups need over 128 000 of them.
SEAM_TINY_BEFORE, SEAM_TINY_AFTER = 180000, 6000
# Waymo form: a frame gives about 4 pairs in 4 groups (every box is in its type's shard 0 and in its range shard)
WM_SEAM_FRAMES_BEFORE, WM_SEAM_FRAMES_AFTER = 45000, 1000


@functools.lru_cache(None)
def bev_seams():
    """One call: pred / gt box arrays of all groups concatenated, with the (n_groups, 2) sizes.  Tiny groups sit in a
    3 m cell each so that some pairs match and some do not."""
    rng = np.random.default_rng(704)
    sizes = np.concatenate([_tiny_sizes(rng, SEAM_TINY_BEFORE), np.array(SEAM_DENSE), _tiny_sizes(rng, SEAM_TINY_AFTER)])
    n_p, n_g = int(sizes[:, 0].sum()), int(sizes[:, 1].sum())
    cell = rng.uniform(-500, 500, (sizes.shape[0], 2))
    pg, gg = np.repeat(np.arange(sizes.shape[0]), sizes[:, 0]), np.repeat(np.arange(sizes.shape[0]), sizes[:, 1])

    def side(group, n):
        c = cell[group] + rng.uniform(-1.5, 1.5, (n, 2))
        return _boxes7(c[:, 0], c[:, 1], rng.uniform(3.5, 5.5, n), rng.uniform(1.6, 2.4, n), rng.uniform(-0.5, 0.5, n))
    pred, gt = side(pg, n_p), side(gg, n_g)
    p_off, g_off = np.concatenate([[0], np.cumsum(sizes[:, 0])]), np.concatenate([[0], np.cumsum(sizes[:, 1])])
    for f in range(SEAM_TINY_BEFORE, SEAM_TINY_BEFORE + len(SEAM_DENSE)):
        pred[p_off[f]:p_off[f + 1]] = bev_cluster(rng, int(sizes[f, 0]), cell[f])
        gt[g_off[f]:g_off[f + 1]] = bev_cluster(rng, int(sizes[f, 1]), cell[f])
    return dict(family="seams", sizes=sizes, pred=pred, gt=gt, pred_off=p_off, gt_off=g_off)


@functools.lru_cache(None)
def bev_cases():
    """The single-sample cases: dicts with family, name, pred (P, 7), gt (G, 7); chain cases also carry rows / shifted."""
    out = []
    rng = np.random.default_rng(701)
    for P, G in DENSE_SIZES + BEV_LDS_SEAM:
        out.append(dict(family="dense", name=f"dense-{P}x{G}", pred=bev_cluster(rng, P), gt=bev_cluster(rng, G)))
    for n in CHAIN_SIZES:
        for v in CHAIN_VARIANTS:
            out.append(dict(family="chain", name=f"chain-{v}-{n}", variant=v, n=n, **bev_chain(n, v)))
    one = _boxes7([12.5], [-3.25], 4.5, 2.0, 0.0)      # axis-aligned: the IoU is exactly 1
    for P, G in TIES_SIZES:
        out.append(dict(family="ties", name=f"ties-{P}x{G}", pred=np.repeat(one, P, 0), gt=np.repeat(one, G, 0)))
    return out


# ---------------------------------------------------------------------------------------------------- Waymo form
WM_CHAIN = {1: dict(L=4.0, W=2.0, d=1.2, eps=1e-4, last=-0.3, end_dy=0.046),      # vehicle, threshold 0.7: IoU 0.7392, 0.7391, third 0.3793
            2: dict(L=1.0, W=1.0, d=0.5, eps=1e-4, last=-0.05, end_dy=0.0877)}    # threshold 0.5: IoU 0.6001, 0.5999, third 0.1428
WM_CHAIN_TALL_EPS = 1e-5     # tall: the shift must cost less than dropping prediction 0 outright, also over 1023 steps
WM_MANY_LEVELS = 300         # groups up to this side carry up to 101 distinct score levels, larger ones at most 5:
                             # waymo_eval.counts_host runs one scipy solve per distinct prediction subset


def _wm_side(frame, typ, cx, cy, cz, length, width, height, heading):
    n = np.size(cx)
    box = np.empty((n, 8))
    hd = np.broadcast_to(np.asarray(heading, np.float64), (n,))
    box[:, 0], box[:, 1], box[:, 2], box[:, 3], box[:, 4], box[:, 5], box[:, 6], box[:, 7] = cx, cy, length, width, np.cos(hd), np.sin(hd), cz, height
    return dict(box=box, head=hd.astype(np.float32), type=np.broadcast_to(np.asarray(typ, np.int32), (n,)).copy(),
                dist=np.sqrt(box[:, 0] ** 2 + box[:, 1] ** 2 + box[:, 6] ** 2), frame=np.broadcast_to(np.asarray(frame, np.int64), (n,)).copy())


def _wm_cluster(rng, frame, typ, n):
    """n boxes of a cluster tight enough for 3D IoU above 0.7 between most pairs, centred 30 m out so that the range
    shards [0, 30) and [30, 50) split it."""
    s = 1.0 if typ == 1 else 0.3
    return _wm_side(frame, typ, 30.0 + s * rng.uniform(-0.25, 0.25, n), s * rng.uniform(-0.12, 0.12, n), rng.uniform(-0.01, 0.01, n),
                    s * rng.uniform(4.4, 4.6, n), s * rng.uniform(1.95, 2.05, n), rng.uniform(1.58, 1.62, n), rng.uniform(-0.01, 0.01, n))


def _few_levels(scores):
    """At most 4 score levels (0.9, 0.7, 0.5, 0.3), keeping the order."""
    return (0.9 - 0.2 * np.minimum((0.99 - np.asarray(scores)) // 0.175, 3)).astype(np.float32)


def _skewed_levels(scores):
    """4 score levels by quartile of a uniform score: 0.9, then 0.025, 0.015, 0.005, so that only cutoffs 0, 1 and 2 admit
    more than a quarter of the predictions: the per-cutoff check mode solves all 101 cutoffs afresh."""
    return np.array([0.005, 0.015, 0.025, 0.9], np.float32)[np.minimum((np.asarray(scores) * 4).astype(int), 3)]


def _wm_chain(rng, frame, typ, n, variant):
    """Waymo chain of side n.  Chained scores fall from 0.99 to 0.30; the last prediction scores 0.105 (it joins at cutoff
    10 and below) or, variant mid, 0.645 (an interior cutoff: the chain keeps growing after the re-route).  wide: n - 2
    chained + last against n ground truth; tall: n - 1 chained + last against n - 1 ground truth, so one prediction
    must go and the path ends in a padded column.  There the chain's end is moved sideways (end_dy: IoU 0.02 above the
    threshold) and the steps are finer, so that the cheapest way is to shift every prediction and drop the end.  Chained prediction i and ground truth i both head pi (i even) or 0 (i odd) -- the footprint is the
    same --, so a pair (i, i) has heading accuracy 1 and a pair (i, i + 1) has 0: the heading sum tells the shifted
    matching from the unshifted one."""
    c = WM_CHAIN[1 if typ == 1 else 2]
    n_chain = n - 2 if variant == "wide" else n - 1
    n_gt = n - 1 if variant == "tall" else n
    gx, px = chain_layout(n_chain, n_gt, n_chain, c["L"], c["W"], c["d"], WM_CHAIN_TALL_EPS if variant == "tall" else c["eps"], c["last"])
    py = np.zeros(n_chain + 1)
    if variant == "tall":
        py[n_chain - 1] = c["end_dy"]
    scores = np.append(0.99 - 0.69 * np.arange(n_chain) / max(n_chain - 1, 1), 0.645 if variant == "mid" else 0.105)
    if n > WM_MANY_LEVELS:
        scores[:-1] = _few_levels(scores[:-1])
    pred = _wm_side(frame, typ, px, py, 0.0, c["L"], c["W"], 1.6, np.append(math.pi * (np.arange(n_chain) % 2 == 0), 0.0))
    gt = _wm_side(frame, typ, gx, 0.0, 0.0, c["L"], c["W"], 1.6, math.pi * (np.arange(n_gt) % 2 == 0))
    pred["score"] = scores.astype(np.float32)
    gt["level"] = rng.integers(1, 3, n_gt).astype(np.int32)
    return pred, gt


def _cat(parts):
    return {k: np.concatenate([p[k] for p in parts]) for k in parts[0]}


_EMPTY_PRED = dict(box=np.zeros((0, 8)), head=np.zeros(0, np.float32), type=np.zeros(0, np.int32), dist=np.zeros(0),
                   frame=np.zeros(0, np.int64), score=np.zeros(0, np.float32))
_EMPTY_GT = dict(box=np.zeros((0, 8)), head=np.zeros(0, np.float32), type=np.zeros(0, np.int32), dist=np.zeros(0),
                 frame=np.zeros(0, np.int64), level=np.zeros(0, np.int32))


@functools.lru_cache(None)
def waymo_family(family):
    """(pred, gt, n_frames, frames) of one cm3d_waymo_metrics call in the form of waymo_eval.pack_arrays; frames lists
    (name, type, P, G, extra) of the single-type frames (the tiny frames of seams are not listed)."""
    rng = np.random.default_rng(dict(dense=721, chain=712, ties=713, seams=714)[family])
    preds, gts, frames = [_EMPTY_PRED], [_EMPTY_GT], []
    n_tiny = [0]                      # frames of tiny(): numbered like the others, not listed

    def add(name, typ, pred, gt, **extra):
        frames.append(dict(name=name, frame=len(frames) + n_tiny[0], type=typ, P=pred["box"].shape[0], G=gt["box"].shape[0], **extra))
        preds.append(pred)
        gts.append(gt)

    def dense(P, G, typ):
        f = len(frames) + n_tiny[0]
        pred, gt = _wm_cluster(rng, f, typ, P), _wm_cluster(rng, f, typ, G)
        s = rng.uniform(0.0, 1.0, P)
        pred["score"] = (_skewed_levels(s) if max(P, G) > WM_MANY_LEVELS else s).astype(np.float32)
        gt["level"] = rng.integers(1, 3, G).astype(np.int32)
        add(f"dense-{P}x{G}-type{typ}", typ, pred, gt)

    def tiny(n):                      # n frames of a few boxes of one to three types: groups of 0, 1 or 2 boxes a side
        f0 = len(frames) + n_tiny[0]
        n_tiny[0] += n
        n_types = rng.integers(1, 4, n)
        types = np.argsort(rng.random((n, 4)), 1) + 1                   # per frame: a random order of the four types
        use = np.arange(4)[None, :] < n_types[:, None]
        frame, typ = np.repeat(np.arange(f0, f0 + n), n_types), types[use]
        sizes = _tiny_sizes(rng, typ.size)
        s = np.where(typ == 1, 1.0, 0.3)
        cx, cy = rng.uniform(-45, 45, (2, typ.size))
        for side, out, key in ((0, preds, "score"), (1, gts, "level")):
            e = np.repeat(np.arange(typ.size), sizes[:, side])
            m = e.size
            b = _wm_side(frame[e], typ[e], cx[e] + s[e] * rng.uniform(-0.4, 0.4, m), cy[e] + s[e] * rng.uniform(-0.2, 0.2, m), 0.0,
                         s[e] * rng.uniform(4.2, 4.8, m), s[e] * rng.uniform(1.9, 2.1, m), 1.6, rng.uniform(-0.1, 0.1, m))
            b[key] = rng.uniform(0, 1, m).astype(np.float32) if key == "score" else rng.integers(1, 3, m).astype(np.int32)
            out.append(b)
    if family == "dense":
        for k, (P, G) in enumerate(WM_DENSE_SIZES):
            dense(P, G, (1, 2, 4)[k % 3])
    elif family == "chain":
        for k, n in enumerate(CHAIN_SIZES):
            for v in CHAIN_VARIANTS:
                typ = (1, 2, 4)[(k + CHAIN_VARIANTS.index(v)) % 3]
                pred, gt = _wm_chain(rng, len(frames), typ, n, v)
                add(f"chain-{v}-{n}-type{typ}", typ, pred, gt, variant=v, n=n)
    elif family == "ties":
        # identical boxes, headings and levels: every maximum assignment gives the same counts and heading sum
        for k, (P, G) in enumerate(WM_TIES_SIZES):
            typ, f = (1, 2, 4)[k % 3], len(frames)
            pred = _wm_side(f, typ, np.full(P, 20.0), -3.25, 0.5, 4.5, 2.0, 1.5, 0.0)
            gt = _wm_side(f, typ, np.full(G, 20.0), -3.25, 0.5, 4.5, 2.0, 1.5, 0.0)
            pred["score"] = _few_levels(0.3 + 0.69 * rng.uniform(0.0, 1.0, P))
            gt["level"] = np.full(G, 1, np.int32)
            add(f"ties-{P}x{G}-type{typ}", typ, pred, gt)
    else:
        tiny(WM_SEAM_FRAMES_BEFORE)
        for k, (P, G) in enumerate(SEAM_DENSE):
            dense(P, G, (1, 2, 4)[k % 3])
        tiny(WM_SEAM_FRAMES_AFTER)
    return _cat(preds), _cat(gts), len(frames) + n_tiny[0], frames


def reversed_gt(packed):
    """The packed call with the ground truth of every group in reverse order: the same problem, other column numbers."""
    go = packed["gt_off"]
    idx = np.concatenate([np.arange(go[g + 1] - 1, go[g] - 1, -1) for g in range(go.size - 1)] + [np.zeros(0, np.int64)]).astype(np.int64)
    out = dict(packed)
    for k in ("gt_box", "gt_head", "gt_level"):
        out[k] = packed[k][idx]
    return out


def reversed_weights(packed, weights):
    """pair_weights of reversed_gt(packed) from those of packed: the columns of every group's matrix in reverse order."""
    w, pair_off = weights
    G = np.diff(packed["gt_off"])
    g = np.repeat(np.arange(G.size), np.diff(pair_off))
    loc = np.arange(w.size) - pair_off[g]
    return w[pair_off[g] + loc // G[g] * G[g] + (G[g] - 1 - loc % G[g])], pair_off


# ---------------------------------------------------------------------------------------------------- shared references
@functools.lru_cache(None)
def bev_call(family):
    """One cm3d_bev_match call of a family as flat arrays: float64 records (ops.match_records of all boxes), the offsets
    of its samples and their names."""
    from cm3d_amd import ops
    if family == "seams":
        s = bev_seams()
        sizes, pred, gt = s["sizes"], s["pred"], s["gt"]
        names = None
    else:
        cs = [c for c in bev_cases() if c["family"] == family]
        sizes = np.array([(c["pred"].shape[0], c["gt"].shape[0]) for c in cs])
        pred, gt = np.concatenate([c["pred"] for c in cs]), np.concatenate([c["gt"] for c in cs])
        names = [c["name"] for c in cs]
    return dict(family=family, names=names, sizes=sizes, pred_rec=np.ascontiguousarray(ops.match_records(pred)),
                gt_rec=np.ascontiguousarray(ops.match_records(gt)), pair_off=pair_offsets(sizes),
                pred_off=np.concatenate([[0], np.cumsum(sizes[:, 0])]), gt_off=np.concatenate([[0], np.cumsum(sizes[:, 1])]))


def sample_name(call, f):
    P, G = call["sizes"][f]
    return call["names"][f] if call["names"] else f"seams-group{f}-{P}x{G}"


@functools.lru_cache(None)
def bev_reference(oracle, family, thr):
    """The oracle's answer for a family's call at one threshold, computed once per process: pred_match and match_iou of
    all predictions, the weights of all pairs (sample f: W[pair_off[f]:pair_off[f + 1]] as (P, G)), per sample the
    oracle's total and the optimum of scipy's linear_sum_assignment on those weights.
    orc_bev_match (what oracle.bev_match wraps) is called on slices of the flat arrays: the wrapper's per-sample array
    handling would cost more than the 186 000 solves of the seams call."""
    from scipy.optimize import linear_sum_assignment
    call = bev_call(family)
    lib = oracle.lib()
    pr, gr, sizes, po, go, pair_off = (call[k] for k in ("pred_rec", "gt_rec", "sizes", "pred_off", "gt_off", "pair_off"))
    pm, gm = np.full(pr.shape[0], -1, np.int32), np.full(gr.shape[0], -1, np.int32)
    iou, W = np.zeros(pr.shape[0]), np.zeros(int(pair_off[-1]), np.int32)
    total, optimum = np.zeros(sizes.shape[0], np.int64), np.zeros(sizes.shape[0], np.int64)
    arrays = (pr, gr, pm, gm, iou, W)                  # addresses of row 0 and row strides: the slices cost more than the solves
    (a_p, a_g, a_pm, a_gm, a_iou, a_w), (s_p, s_g, s_pm, s_gm, s_iou, s_w) = ([x.ctypes.data for x in arrays], [x.strides[0] for x in arrays])
    for f in range(sizes.shape[0]):
        P, G = int(sizes[f, 0]), int(sizes[f, 1])
        if P == 0 or G == 0:
            continue
        p0, g0, w0 = int(po[f]), int(go[f]), int(pair_off[f])
        total[f] = lib.orc_bev_match(a_p + s_p * p0, P, a_g + s_g * g0, G, float(thr), a_pm + s_pm * p0, a_gm + s_gm * g0,
                                     a_iou + s_iou * p0, a_w + s_w * w0)
        Wf = W[w0:w0 + P * G]
        if min(P, G) == 1:
            optimum[f] = Wf.max()
        else:
            Wf = Wf.reshape(P, G)
            r, c = linear_sum_assignment(Wf, maximize=True)
            optimum[f] = Wf[r, c].sum()
    return dict(pred_match=pm, match_iou=iou, W=W, total=total, optimum=optimum)


@functools.lru_cache(None)
def waymo_packed(family):
    """pack_arrays of a family, once per process."""
    from cm3d_amd import waymo_eval as we
    pred, gt, n_frames, _ = waymo_family(family)
    return we.pack_arrays(pred, gt, n_frames)


@functools.lru_cache(None)
def waymo_weights(family):
    """waymo_eval.pair_weights of a family, once per process."""
    from cm3d_amd import waymo_eval as we
    return we.pair_weights(waymo_packed(family))


@functools.lru_cache(None)
def waymo_reference(family):
    """waymo_eval.counts_host of a family, once per process."""
    from cm3d_amd import waymo_eval as we
    return we.counts_host(waymo_packed(family), waymo_weights(family))
