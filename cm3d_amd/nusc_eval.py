"""nuScenes detection scoring with the matching on the GPU (cm3d_nusc_match), for one result file and for every alpha of
the SAM3D fusion grid search.

The device decides integers only -- which candidates are true positives at which distance threshold, and which ground-truth
box each took.  Every float a user sees comes from the numpy statements `eval_detection` uses: the loaders and filters are
its own functions, `curves` is `_accumulate`'s tail (eval_detection.py:384-397) and the summary is `DetectionEval.main`.

  pack        candidates + ground truth -> groups (one sample, or one (sample, class)), offsets, npos, the map back to boxes
  match_host  the kernel's rule in numpy / Python, same outputs: what the device is held to byte for byte
  curves      sorted scores + TP flags -> DetectionMetricData
  evaluate    DetectionEval.main() with the matcher in place of the Python greedy loop; evaluate_host: matcher = match_host
  GridScorer  ground truth loaded and filtered once; score(cands, alphas) -> mAP per alpha from ONE matcher call

The rule differs from `_accumulate` in one stated way: squared distances are compared (d2 = dx * dx + dy * dy < th * th, nearest by
d2) where the reference compares np.linalg.norm(...) with th.  numpy's norm is a BLAS dot followed by a square root and is not
reproducible to the bit from its operands, so it cannot be restated; the two rules can only disagree when a distance lies within
an ulp of a threshold or of another distance (tests/test_nusc_match_host.py measures the margin of its sets).
"""
import time

import numpy as np

from . import eval_detection as ev


def state(kind, p, s, alpha):
    """fusion.fuse's rule for one alpha on candidate arrays -> (active, score): kind 0 an unmatched prediction (score p),
    kind 1 an unmatched SAM3D box (clip(s * alpha, 0, 1)), kind 2 / 3 the prediction's / the SAM3D box of a matched pair, of
    which the SAM3D box is taken iff s * alpha > p."""
    prod = s * np.float64(alpha)
    sam = prod > p
    active = (kind == 0) | (kind == 1) | ((kind == 2) & ~sam) | ((kind == 3) & sam)
    score = np.where((kind == 0) | (kind == 2), p, np.clip(prod, 0, 1))
    return active, score


def candidates_of(eval_boxes):
    """A plain result file as candidates: every box kind 0, in the order of EvalBoxes.all."""
    boxes = eval_boxes.all
    n = len(boxes)
    return boxes, np.zeros(n, np.int32), np.array([b["detection_score"] for b in boxes], np.float64).reshape(n), np.zeros(n, np.float64)


def pack(cands, gt_boxes, class_names=None, dist_ths=(0.5, 1.0, 2.0, 4.0)):
    """cands = (boxes, kind, p, s): box dicts (sample_token, translation, detection_name) in file order with their fusion
    state.  gt_boxes: the filtered EvalBoxes.  class_names None: one group per sample (the "object" scoring); else one per
    (sample, class) and candidates of other names are left out, as accumulate_with_recall never sees them.  Samples come in
    the order the candidates first name them, then the samples only the ground truth has (they count in npos).  Inside a
    group candidates keep file order, so a candidate's index in the packed arrays orders it like its index in the
    reference's per-class prediction list."""
    boxes, kind, p, s = cands
    kind, p, s = np.asarray(kind, np.int32), np.asarray(p, np.float64), np.asarray(s, np.float64)
    names = ["object"] if class_names is None else list(class_names)
    cls_of = {n: i for i, n in enumerate(names)}
    K = len(names)
    samples = {}
    for b in boxes:
        samples.setdefault(b["sample_token"], len(samples))
    for tok in gt_boxes.sample_tokens:
        samples.setdefault(tok, len(samples))
    n_groups = len(samples) * K
    c_cls = np.array([0 if class_names is None else cls_of.get(b["detection_name"], -1) for b in boxes], np.int64).reshape(len(boxes))
    c_grp = np.array([samples[b["sample_token"]] for b in boxes], np.int64).reshape(len(boxes)) * K + c_cls
    keep = np.flatnonzero(c_cls >= 0)
    src = keep[np.argsort(c_grp[keep], kind="stable")]
    cand_off = np.concatenate([[0], np.cumsum(np.bincount(c_grp[src], minlength=n_groups))]).astype(np.int64)
    gt_list, g_grp, g_cls = [], [], []
    for tok in gt_boxes.sample_tokens:
        for b in gt_boxes[tok]:
            c = 0 if class_names is None else cls_of.get(b["detection_name"], -1)
            if c >= 0:
                gt_list.append(b); g_grp.append(samples[tok] * K + c); g_cls.append(c)
    g_grp, g_cls = np.array(g_grp, np.int64), np.array(g_cls, np.int64)
    g_order = np.argsort(g_grp, kind="stable")
    gt_off = np.concatenate([[0], np.cumsum(np.bincount(g_grp, minlength=n_groups))]).astype(np.int64)
    return dict(
        class_names=names, dist_th=np.array(dist_ths, np.float64), cand_off=cand_off, gt_off=gt_off,
        cand_xy=np.array([boxes[i]["translation"][:2] for i in src], np.float64).reshape(-1, 2), cand_kind=kind[src], cand_p=p[src],
        cand_s=s[src], cand_src=src, cand_class=c_cls[src], cand_group=c_grp[src],
        gt_xy=np.array([gt_list[i]["translation"][:2] for i in g_order], np.float64).reshape(-1, 2), gt_box=[gt_list[i] for i in g_order],
        npos=np.bincount(g_cls, minlength=K).astype(np.int64))


def _walk(order, d2, th2):
    """One group at one alpha: the active candidates `order` (descending score, equal scores by descending position) against
    the d2 rows.  Per threshold on its own: nearest box not yet taken, lowest index on equal d2, taken iff d2 < th * th."""
    bits = np.full(len(order), 0x80, np.uint8)
    idx = np.full((len(order), len(th2)), -1, np.int32)
    for t, lim in enumerate(th2):
        taken = np.zeros(d2.shape[1], bool)
        for r, c in enumerate(order):
            row = np.where(taken, np.inf, d2[c])
            j = int(np.argmin(row))
            if row[j] < lim:
                taken[j] = True
                bits[r] |= 1 << t
                idx[r, t] = j
    return bits, idx


def match_host(packed, alphas, want_idx=False, device_ms=None):
    """The rule of cm3d_nusc_match (include/cm3d_hip.h) on the host: (tp_bits uint8[A][C], match_idx int32[A][C][T] or None)."""
    alphas = np.asarray(alphas, np.float64).reshape(-1)
    co, go = packed["cand_off"], packed["gt_off"]
    C, T = int(co[-1]), len(packed["dist_th"])
    th2 = [float(np.float64(th) * np.float64(th)) for th in packed["dist_th"]]
    tp_bits = np.zeros((alphas.size, C), np.uint8)
    match_idx = np.full((alphas.size, C, T), -1, np.int32)
    todo = [g for g in range(co.size - 1) if co[g + 1] > co[g]]
    d2, seen = {}, {}
    for g in todo:
        if go[g + 1] > go[g]:
            dx = packed["cand_xy"][co[g]:co[g + 1], None, 0] - packed["gt_xy"][None, go[g]:go[g + 1], 0]
            dy = packed["cand_xy"][co[g]:co[g + 1], None, 1] - packed["gt_xy"][None, go[g]:go[g + 1], 1]
            d2[g] = dx * dx + dy * dy
    for a, alpha in enumerate(alphas):
        active, score = state(packed["cand_kind"], packed["cand_p"], packed["cand_s"], alpha)
        tp_bits[a, active] = 0x80
        # sorted((score, position)) of every group's active candidates in one lexsort; a group's walk is its segment reversed
        asc = np.lexsort((np.arange(C), score + 0.0, packed["cand_group"]))
        asc = asc[active[asc]]
        seg = np.concatenate([[0], np.cumsum(np.bincount(packed["cand_group"][asc], minlength=co.size - 1))])
        for g in d2:
            order = asc[seg[g]:seg[g + 1]][::-1]
            key = (g, order.tobytes())           # the walk depends on the order alone: alphas that agree on it share it
            if key not in seen:
                seen[key] = _walk(order - co[g], d2[g], th2)
            tp_bits[a, order], match_idx[a, order] = seen[key]
    return tp_bits, (match_idx if want_idx else None)


def curves(scores, positions, tp_flags, npos, errs=None, order=None):
    """`_accumulate`'s tail (eval_detection.py:382-399) from decided matches: the scores, positions (index in the per-class
    prediction list) and TP flags of the active candidates of one class at one threshold -> (DetectionMetricData, actual
    recall).  errs: the five TP errors per candidate (read at the TPs only); None leaves the error curves at 1 (the AP does
    not read them).  order: the walk order when the caller has it already (it is shared by the thresholds)."""
    if npos == 0:
        return ev.DetectionMetricData.no_predictions(), 0
    if order is None:
        order = np.lexsort((positions, scores))[::-1]           # sorted((v, i))[::-1]
    hit = np.asarray(tp_flags, bool)[order]
    if not hit.any():
        return ev.DetectionMetricData.no_predictions(), 0
    tp = np.cumsum(hit.astype(int)).astype(float)
    fp = np.cumsum((~hit).astype(int)).astype(float)
    conf = np.array(scores, float)[order]
    match_conf = conf[hit]
    prec = tp / (fp + tp)
    rec = tp / float(npos)
    rec_actual = float(np.max(rec))
    rec_interp = np.linspace(0, 1, ev.NELEM)
    prec = np.interp(rec_interp, rec, prec, right=0)
    conf = np.interp(rec_interp, rec, conf, right=0)
    out = {}
    for key in ev.TP_METRICS:
        if errs is None:
            out[key] = np.ones(ev.NELEM)
            continue
        tmp = ev.cummean(np.array(errs[key], dtype=float)[order][hit])
        out[key] = np.interp(conf[::-1], match_conf[::-1], tmp[::-1])[::-1]
    return ev.DetectionMetricData(rec_interp, prec, conf, out['trans_err'], out['vel_err'], out['scale_err'], out['orient_err'],
                                  out['attr_err']), rec_actual


def _tp_errors(g, p, class_name, object_class):
    """The five errors of one match, as `_accumulate` appends them (eval_detection.py:367-378)."""
    if object_class:
        name = g['detection_name']
        return dict(trans_err=ev.center_distance(g, p), vel_err=np.nan if name in ['traffic_cone', 'barrier'] else ev.velocity_l2(g, p),
                    scale_err=1 - ev.scale_iou(g, p), orient_err=np.nan if name in ['traffic_cone'] else ev.yaw_diff(g, p, period=np.pi),
                    attr_err=np.nan if name in ['barrier', 'traffic_cone'] else 1 - ev.attr_acc(g, p))
    return dict(trans_err=ev.center_distance(g, p), vel_err=ev.velocity_l2(g, p), scale_err=1 - ev.scale_iou(g, p),
                orient_err=ev.yaw_diff(g, p, period=np.pi if class_name == 'barrier' else 2 * np.pi), attr_err=1 - ev.attr_acc(g, p))


def _default_matcher():
    from . import ops
    return ops.nusc_match


def _device_on_road(polygons, xy):
    """filter_eval_boxes' hook: point_in_polygons for all boxes in one cm3d_points_in_polygons call."""
    from . import ops
    return ops.points_in_polygons([polygons], xy).astype(bool)


class NativeEval(ev.DetectionEval):
    """DetectionEval with `evaluate` running one matcher call for all groups and thresholds instead of the per-threshold Python
    loops; loading, filtering and `main` (summary, the two json files, the printed table) are the parent's."""

    def __init__(self, *args, matcher=None, **kwargs):
        if matcher is None:                 # the device route: the drivable-area filter, too, is one GPU call per box set
            kwargs.setdefault("on_road", _device_on_road)
        super().__init__(*args, **kwargs)
        self.matcher = matcher or _default_matcher()
        self.recall_actual = {}

    def accumulate(self):
        """-> md_list {(name, th): DetectionMetricData}, with recall_actual filled alongside."""
        names = ["object"] if self.object_only else list(self.cfg.class_names)
        cands = candidates_of(self.pred_boxes)
        boxes = cands[0]
        packed = pack(cands, self.gt_boxes, None if self.object_only else names, self.cfg.dist_ths)
        tp_bits, match_idx = self.matcher(packed, [1.0], want_idx=True)
        bits, idx = tp_bits[0], match_idx[0]
        md_list, cache = {}, {}
        for ci, name in enumerate(names):
            sel = np.flatnonzero((packed["cand_class"] == ci) & ((bits & 0x80) != 0))
            scores = packed["cand_p"][sel]
            order = np.lexsort((sel, scores))[::-1]
            for ti, th in enumerate(self.cfg.dist_ths):
                hit = ((bits[sel] >> ti) & 1).astype(bool)
                errs = {k: np.full(sel.size, np.nan) for k in ev.TP_METRICS}
                for r in np.flatnonzero(hit):
                    c = int(sel[r])
                    gi = int(packed["gt_off"][packed["cand_group"][c]] + idx[c, ti])
                    if (c, gi) not in cache:
                        cache[(c, gi)] = _tp_errors(packed["gt_box"][gi], boxes[packed["cand_src"][c]], name, self.object_only)
                    for k, v in cache[(c, gi)].items():
                        errs[k][r] = v
                md_list[(name, th)], self.recall_actual[(name, th)] = curves(scores, sel, hit, int(packed["npos"][ci]), errs, order)
        return md_list

    def evaluate(self):
        t0 = time.time()
        md_list = self.accumulate()
        names = ["object"] if self.object_only else list(self.cfg.class_names)
        recall_list = []
        for name in names:
            recs = [self.recall_actual[(name, th)] for th in self.cfg.dist_ths]
            recall_list.append(sum(recs) / len(recs))
        metrics = ev.DetectionMetrics(self.cfg)
        for name in names:
            for th in self.cfg.dist_ths:
                metrics.add_label_ap(name, th, ev.calc_ap(md_list[(name, th)], self.cfg.min_recall, self.cfg.min_precision))
            for m in ev.TP_METRICS:
                md = md_list[(name, self.cfg.dist_th_tp)]
                if not self.object_only and name in ['traffic_cone'] and m in ['attr_err', 'vel_err', 'orient_err']:
                    tp = np.nan
                elif not self.object_only and name in ['barrier'] and m in ['attr_err', 'vel_err']:
                    tp = np.nan
                else:
                    tp = ev.calc_tp(md, self.cfg.min_recall, m)
                metrics.add_label_tp(name, m, tp)
        metrics.add_runtime(time.time() - t0)
        return metrics, md_list, recall_list


def evaluate(tables, cfg, result_path, eval_set=None, output_dir=None, drivable_filtering=False, object_only=True, verbose=True,
             matcher=None):
    """What DetectionEval(...).main() returns, writes and prints, with the matching done by `matcher` (default: the GPU,
    ops.nusc_match; a group over the kernel's capacity raises Cm3dError with .status)."""
    return NativeEval(tables, cfg, result_path, eval_set, output_dir, drivable_filtering, object_only, verbose, matcher=matcher).main()


def evaluate_host(tables, cfg, result_path, eval_set=None, output_dir=None, drivable_filtering=False, object_only=True, verbose=True):
    return evaluate(tables, cfg, result_path, eval_set, output_dir, drivable_filtering, object_only, verbose, matcher=match_host)


class GridScorer:
    """The scoring side of the nuScenes SAM3D fusion grid search (src/nuscenes/linear_matching.py:455-478: all classes, no
    drivable filtering): ground truth loaded and filtered once, then score(cands, alphas) -> the mean AP of every alpha's
    fused file from one matcher call."""

    def __init__(self, tables, cfg, eval_set=None):
        self.tables, self.cfg, self.eval_set = tables, cfg, eval_set
        gt = ev.load_gt(tables, eval_set, verbose=False, rare=len(cfg.class_range) > 10)
        gt = ev.add_center_dist(tables, gt)
        self.gt_boxes = ev.filter_eval_boxes(tables, gt, cfg.class_range, False, False)

    def filtered(self, cands):
        """The prediction filters of DetectionEval on every candidate (class range on its own position and emitted class, bike
        racks): they do not depend on alpha.  -> the surviving (boxes, kind, p, s), boxes as EvalBoxes dicts."""
        boxes, kind, p, s = cands
        kind = np.asarray(kind, np.int32)
        eb, emitted = ev.EvalBoxes(), {}
        for i, b in enumerate(boxes):
            tok = b["sample_token"]
            d = ev._box(tok, b["translation"], b["size"], b["rotation"], b.get("velocity", (0, 0)), -1, b["detection_name"], -1.0,
                        b.get("attribute_name", ""))
            d["cand"] = i
            eb.boxes.setdefault(tok, []).append(d)
            emitted[tok] = emitted.get(tok, 0) + (kind[i] != 3)          # a pair emits one of its two boxes at every alpha
        for tok, n in emitted.items():
            assert n <= self.cfg.max_boxes_per_sample, "Error: Only <= %d boxes per sample allowed!" % self.cfg.max_boxes_per_sample
        eb = ev.add_center_dist(self.tables, eb)
        eb = ev.filter_eval_boxes(self.tables, eb, self.cfg.class_range, False, False)
        kept = eb.all
        ids = np.array([b["cand"] for b in kept], np.int64).reshape(len(kept))
        return kept, kind[ids], np.asarray(p, np.float64)[ids], np.asarray(s, np.float64)[ids]

    def score(self, cands, alphas, matcher=None):
        matcher = matcher or _default_matcher()
        names = list(self.cfg.class_names)
        packed = pack(self.filtered(cands), self.gt_boxes, names, self.cfg.dist_ths)
        tp_bits, _ = matcher(packed, alphas)
        by_class = [np.flatnonzero(packed["cand_class"] == ci) for ci in range(len(names))]
        out = []
        for a, alpha in enumerate(alphas):
            _, score = state(packed["cand_kind"], packed["cand_p"], packed["cand_s"], alpha)
            bits = tp_bits[a]
            metrics = ev.DetectionMetrics(self.cfg)
            for ci, name in enumerate(names):
                sel = by_class[ci][(bits[by_class[ci]] & 0x80) != 0]
                order = np.lexsort((sel, score[sel]))[::-1]         # shared by the thresholds
                for ti, th in enumerate(self.cfg.dist_ths):
                    md, _ = curves(score[sel], sel, (bits[sel] >> ti) & 1, int(packed["npos"][ci]), None, order)
                    metrics.add_label_ap(name, th, ev.calc_ap(md, self.cfg.min_recall, self.cfg.min_precision))
            out.append(metrics.mean_ap)
        return out
