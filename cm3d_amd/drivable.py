"""Host side of the drivable-area test and of the stage-2 filters (include/cm3d_hip.h: cm3d_points_in_polygons, cm3d_stage2_filter; a stage of
cm3d_lift_pass_opt).

The reference tests box centres against the map's drivable-area polygons in two places: the evaluator's filter
(eval_custom.py:496-526) and the stage-2 filters it ships commented out (src/nuscenes/2d_to_3d.py:755-785, labels "Object lane
thresh", "Uncomment for drivable filtering", "Vehicle lane thresh").  The test itself is eval_detection.point_in_polygons; this
module builds the y-slab index the kernels walk -- static data, one index per map location, built with numpy and uploaded once --,
restates the query (query_index: the kernel's walk, chunk for chunk) and the filter rule (filter_rule) for the tests, and holds the
switches of the filtered pass (Stage2Filters).

A polygon table is what eval_detection.load_drivable_polygons returns: a list of (exterior (n, 2) float64, [hole (k, 2), ...]).
"""
from dataclasses import dataclass
from typing import Sequence

import numpy as np

INDEX_ARRAYS = ("tab_y", "tab_slab", "slab_off", "ent_edge", "ent_ring", "edge", "ring_info")
EDGES_PER_SLAB = 8          # slabs of a table: its edges / this (at least 1, at most MAX_SLABS)
MAX_SLABS = 1 << 16
PAD_SLABS = 1               # an edge is also listed in this many slabs on either side of those its y-interval touches
WAVE = 64

NEEDS_ROAD_CLASSES = ["car", "truck", "bus"]        # 2d_to_3d.py:775: the vehicles minus construction_vehicle, trailer, barrier


@dataclass
class Stage2Filters:
    """The opt-in stage-2 filters of a LiftEngine.  drivable: drop car / truck / bus masks whose medoid is not on a drivable-area
    polygon of the frame's map (the batch then carries polygon tables); lane_max_dist: drop masks farther than this from the nearest
    lane point; vehicle_lane_max_dist: the same for the pushed classes.  Strict `>` on float64; inf = off.  The reference's commented
    values are 20 and 4."""
    drivable: bool = False
    lane_max_dist: float = float("inf")
    vehicle_lane_max_dist: float = float("inf")

    def __post_init__(self):
        self.lane_max_dist, self.vehicle_lane_max_dist = float(self.lane_max_dist), float(self.vehicle_lane_max_dist)
        if np.isnan(self.lane_max_dist) or np.isnan(self.vehicle_lane_max_dist):
            raise ValueError("a lane threshold is a number or inf")

    @property
    def active(self):
        return bool(self.drivable) or self.lane_max_dist != float("inf") or self.vehicle_lane_max_dist != float("inf")

    @staticmethod
    def from_args(drivable=False, lane_max_dist=None, vehicle_lane_max_dist=None):
        """From an entry point's flags (None = flag not given); None when no flag asks for anything."""
        f = Stage2Filters(bool(drivable), float("inf") if lane_max_dist is None else lane_max_dist,
                          float("inf") if vehicle_lane_max_dist is None else vehicle_lane_max_dist)
        return f if f.active else None


def needs_road(class_names):
    return np.array([n in NEEDS_ROAD_CLASSES for n in class_names], np.int32)


def table_rings(polygons):
    """The rings of one table that count, in the index's order: per polygon with an exterior of at least 3 nodes the exterior, then
    its holes of at least 3 nodes.  Returns [(ring (n, 2) float64, info)], info = 2 * polygon number + (1 for a hole)."""
    out = []
    for p, (ext, holes) in enumerate(polygons):
        ext = np.asarray(ext, np.float64).reshape(-1, 2)
        if ext.shape[0] < 3:
            continue                     # point_in_polygons never looks at the holes of such a polygon
        out.append((ext, 2 * p))
        for h in holes:
            h = np.asarray(h, np.float64).reshape(-1, 2)
            if h.shape[0] >= 3:
                out.append((h, 2 * p + 1))
    return out


def slab_of(y, ymin, per_y, n_slabs):
    """The slab of y in [ymin, ymax]: the expression the kernel evaluates (float64, one subtraction, one multiplication, truncation).
    It is monotone in y, so an edge listed from slab_of(its lowest y) to slab_of(its highest y) is listed wherever a point of its
    y-interval can land, whatever the rounding."""
    f = (np.asarray(y, np.float64) - ymin) * per_y
    return np.where(f < float(n_slabs - 1), f, float(n_slabs - 1)).astype(np.int64)


def build_index(polygon_tables: Sequence, edges_per_slab=EDGES_PER_SLAB, max_slabs=MAX_SLABS, pad=PAD_SLABS):
    """The y-slab index of T polygon tables as a dict of numpy arrays (INDEX_ARRAYS, layouts in include/cm3d_hip.h) plus `n_tables`.
    Every size is known here; one that does not fit a signed 32-bit offset raises."""
    T = len(polygon_tables)
    tab_y, tab_slab = np.zeros((max(T, 1), 3), np.float64), np.zeros((max(T, 1), 2), np.int32)
    edges, ring_info, slab_offs, ent_edge, ent_ring = [], [], [np.zeros(1, np.int64)], [], []
    n_edges = n_rings = n_slabs_total = n_entries = 0
    for t, polygons in enumerate(polygon_tables):
        rings = table_rings(polygons)
        tab_slab[t, 0] = n_slabs_total
        if not rings:
            continue
        xy = np.concatenate([r for r, _ in rings], 0)
        nxt = np.concatenate([np.roll(r, -1, axis=0) for r, _ in rings], 0)
        e = np.concatenate([xy, nxt], 1)                                   # xs, ys, xn, yn
        ring_of = np.repeat(np.arange(len(rings), dtype=np.int64), [r.shape[0] for r, _ in rings]) + n_rings
        ymin, ymax = float(xy[:, 1].min()), float(xy[:, 1].max())
        E = e.shape[0]
        n = int(min(max(E // max(1, edges_per_slab), 1), max_slabs))
        with np.errstate(all="ignore"):
            per_y = n / (ymax - ymin) if ymax > ymin else 0.0
        if not (np.isfinite(ymin) and np.isfinite(ymax)):
            raise ValueError(f"polygon table {t}: a node's y is not finite")
        if not np.isfinite(per_y) or per_y <= 0.0:
            n, per_y = 1, 0.0
        lo, hi = np.minimum(e[:, 1], e[:, 3]), np.maximum(e[:, 1], e[:, 3])
        s_lo = np.maximum(slab_of(lo, ymin, per_y, n) - pad, 0)
        s_hi = np.minimum(slab_of(hi, ymin, per_y, n) + pad, n - 1)
        cnt = s_hi - s_lo + 1
        total = int(cnt.sum())
        if n_entries + total > 0x7FFFFFFF:
            raise ValueError(f"polygon index: more than 2^31 - 1 slab entries (table {t}: {E} edges over {n} slabs)")
        first = np.cumsum(cnt) - cnt
        which = np.repeat(np.arange(E, dtype=np.int64), cnt)               # entries in edge order
        slab = np.repeat(s_lo, cnt) + (np.arange(total, dtype=np.int64) - np.repeat(first, cnt))
        order = np.argsort(slab, kind="stable")                              # by slab; inside a slab still in edge (= ring) order
        ent_edge.append(which[order] + n_edges)
        ent_ring.append(ring_of[which[order]])
        slab_offs.append(n_entries + np.cumsum(np.bincount(slab, minlength=n)))
        tab_y[t] = (ymin, ymax, per_y)
        tab_slab[t, 1] = n
        edges.append(e)
        ring_info.extend(info for _, info in rings)
        n_edges, n_rings, n_slabs_total, n_entries = n_edges + E, n_rings + len(rings), n_slabs_total + n, n_entries + total
    if max(n_edges * 4, n_rings, n_slabs_total + 1, n_entries) > 0x7FFFFFFF:
        raise ValueError("polygon index: a count exceeds a signed 32-bit offset")

    def cat(parts, dtype, shape):
        return np.ascontiguousarray(np.concatenate(parts, 0) if parts else np.zeros(shape, dtype), dtype)
    return dict(tab_y=tab_y, tab_slab=tab_slab, slab_off=cat(slab_offs, np.int32, (1,)), ent_edge=cat(ent_edge, np.int32, (0,)),
                ent_ring=cat(ent_ring, np.int32, (0,)), edge=cat(edges, np.float64, (0, 4)).reshape(-1, 4),
                ring_info=np.asarray(ring_info, np.int32), n_tables=T)


def query_index(ix, xy, table_of_point):
    """The kernel's query through the index, on the host and step for step (chunks of WAVE entries, runs of equal ring ids inside a
    chunk, parity per ring, rings into polygons, OR over polygons, stop at the first polygon that holds the point): what the tests hold
    against eval_detection.point_in_polygons.  Returns uint8 (n,)."""
    xy = np.asarray(xy, np.float64).reshape(-1, 2)
    tp = np.asarray(table_of_point, np.int64).reshape(-1)
    out = np.zeros(xy.shape[0], np.uint8)
    edge, ent_edge, ent_ring, ring_info = ix["edge"], ix["ent_edge"], ix["ent_ring"], ix["ring_info"]
    for p in range(xy.shape[0]):
        t, (x, y) = int(tp[p]), xy[p]
        if t < 0 or t >= ix["n_tables"]:
            continue
        ymin, ymax, per_y = ix["tab_y"][t]
        s0, n = (int(v) for v in ix["tab_slab"][t])
        if n <= 0 or not (y >= ymin and y <= ymax):
            continue
        s = int(slab_of(y, ymin, per_y, n))
        e0, e1 = int(ix["slab_off"][s0 + s]), int(ix["slab_off"][s0 + s + 1])
        cur_ring, cur_info, cur_poly, par = -1, 0, -1, 0
        ext_odd = hole_odd = inside = False
        c = e0
        while c < e1 and not inside:
            sl = slice(c, min(c + WAVE, e1))
            ring = ent_ring[sl]
            xs, ys, xn, yn = edge[ent_edge[sl]].T
            with np.errstate(all="ignore"):
                cross = ((ys > y) != (yn > y)) & (x < ((xn - xs) * (y - ys)) / np.where(yn == ys, 1.0, yn - ys) + xs)
            k = 0
            while k < ring.size:
                r = int(ring[k])
                k1 = k
                while k1 < ring.size and ring[k1] == r:
                    k1 += 1
                if r != cur_ring:
                    if cur_ring >= 0:
                        if cur_info & 1:
                            hole_odd |= bool(par)
                        else:
                            ext_odd = bool(par)
                    cur_ring, cur_info, par = r, int(ring_info[r]), 0
                    if (cur_info >> 1) != cur_poly:
                        inside |= ext_odd and not hole_odd
                        ext_odd = hole_odd = False
                        cur_poly = cur_info >> 1
                par ^= int(np.count_nonzero(cross[k:k1])) & 1
                k = k1
            c += WAVE
        if cur_ring >= 0:
            if cur_info & 1:
                hole_odd |= bool(par)
            else:
                ext_odd = bool(par)
        out[p] = inside or (ext_odd and not hole_odd)
    return out


def filter_rule(medoid_pos, class_id, lane_dist, on_road, is_vehicle, needs_road_of_class, lane_max_dist=float("inf"),
                vehicle_lane_max_dist=float("inf")):
    """Host restatement of cm3d_stage2_filter's rule: medoid_pos_kept.  on_road None: no polygons, no road test."""
    med = np.asarray(medoid_pos, np.int32)
    cls = np.asarray(class_id, np.int64)
    ld = np.asarray(lane_dist, np.float64)
    with np.errstate(invalid="ignore"):
        drop = (ld > lane_max_dist) | ((np.asarray(is_vehicle)[cls] != 0) & (ld > vehicle_lane_max_dist))
    if on_road is not None:
        drop |= (np.asarray(needs_road_of_class)[cls] != 0) & (np.asarray(on_road) == 0)
    return np.where((med >= 0) & drop, -1, med).astype(np.int32)


def points_on_road(polygon_tables, xy, table_of_point):
    """eval_detection.point_in_polygons for many points, on the host (the reference of the tests and of the Python route)."""
    from .eval_detection import point_in_polygons
    xy = np.asarray(xy, np.float64).reshape(-1, 2)
    with np.errstate(invalid="ignore"):         # (a point at infinity: inf * 0 in the crossing formula, compared false)
        return np.array([point_in_polygons(polygon_tables[int(t)], x, y) for (x, y), t in zip(xy, table_of_point)], np.uint8).reshape(-1)


def tables_key(polygon_tables):
    """A checksum key of polygon tables for callers that have no better one (LiftEngine's cache)."""
    import zlib
    crc = 0
    for polys in polygon_tables:
        crc = zlib.crc32(b"T", crc)
        for ext, holes in polys:
            for r in [ext] + list(holes):
                crc = zlib.crc32(np.ascontiguousarray(r, np.float64).view(np.uint8), zlib.crc32(b"R", crc))
    return ("crc", len(polygon_tables), crc)
