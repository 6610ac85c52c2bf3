"""Single-call mirrors of the reference's helper functions, each running on the GPU
through the C-ABI (no CPU fallback).  Same names and argument meaning as in the reference's
src/nuscenes/2d_to_3d.py so that parity tests read like calls into the reference:

    get_medoid(points)                                   :116-119
    lane_yaws_distances_and_coords(centroids, lane_pts)  :277-302
    push_centroid(centroid, extents, yaw, poserecord)    :164-198 (+ the rotation of :788-806)
    circle_nms(dets, det_labels, threshs_by_label)       :309-332
    rotated_nms(rec, score, group, frame_off, thr, ...)  the opt-in NMS on the boxes' bird's-eye-view overlap (nms.rotated_nms_host)
    points_in_masks(points, cams, masks, cam_nums)       :553-620 for all masks of a frame
    erode(mask) / decode(rles)                           :526-527 / :425
    obb_yaws(point_lists)                                src/kitti/2d_to_3d.py:855-876 + :1524 for several lists
    points_in_polygons(polygon_tables, xy, table)        eval_custom.py:514-519 for many points
    depth_cluster(point_lists, origins, eps, ...)        the opt-in depth clustering of several lists (cluster.depth_cluster_host)
    bev_fit(xyz, off, ...) / yaw_select(...)             the opt-in yaw fit of several lists and the choice of each mask's yaw (bevfit.*_host)
    box_velocity(box, flags, mask_off, ...)              the opt-in association of consecutive frames' boxes (velocity.track_velocity_host)
    box_tracks(box, flags, mask_frame, next_match, ...)  the opt-in tracks behind it: ids, length filter, scores, smoothed velocity (tracks.box_tracks_host)
    ground_grid(origin, points=... | raw=...)            the opt-in per-frame ground grid from a cloud or from raw rows (groundstrip.ground_grid_host)
    ground_strip(hit_xyz, hit_off, mask_frame, ...)      the opt-in strip of ground points from in-mask lists (groundstrip.ground_strip_host)

They are conveniences for tests and small jobs; the batched path is lifting.LiftEngine.
"""
import numpy as np
import torch

from . import _lib
from . import rle as rlemod
from ._lib import check


def _dev():
    if not torch.cuda.is_available():
        raise _lib.Cm3dError("no HIP device: cm3d_amd.ops only runs on the GPU")
    return torch.device("cuda", torch.cuda.current_device())


def _t(a, dtype=None):
    a = np.ascontiguousarray(a, dtype=dtype)
    return torch.from_numpy(a).to(_dev())


def _st():
    return torch.cuda.current_stream().cuda_stream


def _e(*shape, dtype=torch.int32):
    return torch.empty(*shape, dtype=dtype, device=_dev())


def _ws(nbytes):
    return torch.empty(max(int(nbytes), 16), dtype=torch.uint8, device=_dev())


# ----------------------------------------------------------------------------- masks
def decode(rles, as_counts=False):
    """pycocotools.mask.decode equivalent on the GPU: list of COCO RLE dicts (size [W,H]) ->
    uint8 tensor (n, H, W) (the reference's `depth_images` after its transpose, :425-428)."""
    L = _lib.lib()
    W, H = rles[0]["size"]
    cnts = [rlemod.string_to_counts(r["counts"]) if not as_counts else np.asarray(r["counts"], np.uint32) for r in rles]
    off = np.concatenate([[0], np.cumsum([c.size for c in cnts])]).astype(np.int32)
    allc = np.concatenate(cnts).astype(np.uint32)
    d_c, d_o = _t(allc.view(np.int32)), _t(off)
    dense = _e(len(rles), H, W, dtype=torch.uint8)
    ws = _ws(L.cm3d_rle_workspace_bytes(allc.size))
    check(L.cm3d_rle_to_dense(d_c.data_ptr(), d_o.data_ptr(), len(rles), allc.size, W, H, dense.data_ptr(), ws.data_ptr(),
                              ws.numel(), _st()), "cm3d_rle_to_dense")
    return dense


def erode(dense_masks):
    """cv2.erode(mask, ones((3,3))) for a stack of masks, bit-packed: returns (packed (n,H,Wp) int32, bbox (n,8): bounds of the eroded
    pixels [0..3] and the rectangle `packed` stores [4..7] -- here the whole image; unpack_bits turns both into pixels)."""
    L = _lib.lib()
    d = dense_masks if torch.is_tensor(dense_masks) else _t(dense_masks, np.uint8)
    n, H, W = d.shape
    packed = _e(n, H, (W + 31) // 32)
    bbox = _e(n, _lib.BBOX_STRIDE)
    check(L.cm3d_erode_pack(d.data_ptr(), n, W, H, packed.data_ptr(), bbox.data_ptr(), _st()), "cm3d_erode_pack")
    return packed, bbox


def erode_rle(rle_counts_list, W, H, fill=0, guard_slots=0, sizes=None):
    """Same result as erode(decode(.)) straight from run lengths (f1).  `packed` holds `fill` (a 32-bit pattern) in every word
    before the call and has `guard_slots` more slots than masks: tests of what the kernels leave unwritten set both.
    sizes: a list of (w, h), one per mask -- run list k then covers its own w x h image and (W, H) is the canvas it is pasted into,
    top-left (cm3d_rle_erode_pack_sized, rule R of include/cm3d_hip.h); None: every list covers W x H."""
    L = _lib.lib()
    off = np.concatenate([[0], np.cumsum([len(c) for c in rle_counts_list])]).astype(np.int32)
    allc = np.concatenate([np.asarray(c, np.uint32) for c in rle_counts_list]).astype(np.uint32)
    n = len(rle_counts_list)
    d_c, d_o = _t(allc.view(np.int32)), _t(off)
    fill = int(np.array(fill & 0xFFFFFFFF, np.uint32).view(np.int32))
    packed = torch.full((n + guard_slots, H, (W + 31) // 32), fill, dtype=torch.int32, device=_dev())
    bbox = _e(n, _lib.BBOX_STRIDE)
    ws = _ws(L.cm3d_rle_workspace_bytes(allc.size))
    if sizes is not None:
        wh = np.ascontiguousarray(sizes, np.int32).reshape(-1, 2)
        if wh.shape[0] != n:
            raise ValueError("erode_rle: one (w, h) per mask")
        d_wh = _t(wh)
        check(L.cm3d_rle_erode_pack_sized(d_c.data_ptr(), d_o.data_ptr(), n, allc.size, W, H, d_wh.data_ptr(), packed.data_ptr(),
                                          bbox.data_ptr(), ws.data_ptr(), ws.numel(), _st()), "cm3d_rle_erode_pack_sized")
        return packed, bbox
    check(L.cm3d_rle_erode_pack(d_c.data_ptr(), d_o.data_ptr(), n, allc.size, W, H, packed.data_ptr(), bbox.data_ptr(),
                                ws.data_ptr(), ws.numel(), _st()), "cm3d_rle_erode_pack")
    return packed, bbox


def unpack_bits(packed, W, bbox=None):
    """(n,H,Wp) int32 bit-packed -> (n,H,W) uint8 numpy (host helper for tests/tools).  bbox (n,8) from erode / erode_rle: a
    mask's slot holds the rows of its stored rectangle (xw0, y0, wc, rows = bbox[:, 4:8]) one behind the other
    (include/cm3d_hip.h); without it the slots are read as whole images."""
    p = packed.cpu().numpy().view(np.uint32)
    n, H, Wp = p.shape
    if bbox is not None:
        rc = (bbox.cpu().numpy() if torch.is_tensor(bbox) else np.asarray(bbox))[:, 4:8]
        full = np.zeros_like(p)
        flat = p.reshape(n, -1)
        for i, (xw0, y0, wc, rows) in enumerate(rc.tolist()):
            if wc > 0 and rows > 0:
                full[i, y0:y0 + rows, xw0:xw0 + wc] = flat[i, :rows * wc].reshape(rows, wc)
        p = full
    bits = ((p[..., None] >> np.arange(32, dtype=np.uint32)) & 1).astype(np.uint8)
    return bits.reshape(n, H, -1)[:, :, :W]


# ----------------------------------------------------------------------------- a4-a8
def points_in_masks(points, cams, packed, bbox, cam_nums, W, H, min_dist=2.3):
    """All masks of ONE frame.  points (N,4) float32 global frame; cams (C,CAM_STRIDE);
    packed/bbox from erode().  Returns the list of ascending index arrays (track_points, :617)."""
    L = _lib.lib()
    pts = _t(points, np.float32)
    N, n = pts.shape[0], len(cam_nums)
    d_cams = _t(np.asarray(cams, np.float32))
    pt_off, mask_off = _t(np.array([0, N], np.int32)), _t(np.array([0, n], np.int32))
    mask_cam = _t(np.asarray(cam_nums, np.int32))
    planes = (n + 31) // 32
    hit_words, hit_count = _e(planes, N), _e(n)
    status = _e(_lib.STATUS_WORDS)
    hit_off, tile_off = _e(n + 1), _e(n + 1)
    cap = max(1024, N * 8)
    hit_idx = _e(cap)
    st = _st()
    ws = _ws(L.cm3d_project_workspace_bytes(1, N, planes))
    check(L.cm3d_batch_begin(status.data_ptr(), hit_count.data_ptr(), n, 0, 0, st), "cm3d_batch_begin")
    check(L.cm3d_project_hits(pts.data_ptr(), pt_off.data_ptr(), 1, N, N, d_cams.data_ptr(), d_cams.shape[0], mask_off.data_ptr(),
                              mask_cam.data_ptr(), bbox.data_ptr(), packed.data_ptr(), n, W, H, float(np.float32(min_dist)), planes,
                              hit_words.data_ptr(), hit_count.data_ptr(), status.data_ptr(), ws.data_ptr(), ws.numel(), 0, 0, st),
          "cm3d_project_hits")
    check(L.cm3d_compact_hits(hit_words.data_ptr(), planes, 1, N, N, mask_off.data_ptr(), n, hit_count.data_ptr(), 0, 0, 0, 0, 0,
                              pts.data_ptr(), hit_off.data_ptr(), tile_off.data_ptr(), hit_idx.data_ptr(), 0, 0, cap, 0,
                              status.data_ptr(), ws.data_ptr(), ws.numel(), st), "cm3d_compact_hits")
    s = status.cpu().numpy()
    if s[0]:
        raise _lib.Cm3dError(f"status {s}")
    off = hit_off.cpu().numpy()
    idx = hit_idx[: off[-1]].cpu().numpy()
    return [idx[off[i]:off[i + 1]] for i in range(n)]


# ----------------------------------------------------------------------------- a9
def get_medoid(points, want_colsum=False, via_rows=False):
    """points: (3,M) float32 like the reference's argument; returns the medoid column index.  via_rows: hand the
    kernel a cloud + row-index list (its gather form) instead of the contiguous per-hit coordinates."""
    L = _lib.lib()
    p = np.asarray(points.cpu() if torch.is_tensor(points) else points, np.float32)
    M = p.shape[1]
    P4 = np.zeros((M, 4), np.float32)
    P4[:, :3] = p[:3].T
    pts = _t(P4)
    pt_off, mask_frame = _t(np.array([0, M], np.int32)), _t(np.array([0], np.int32))
    ntile = (M + _lib.MEDOID_TILE - 1) // _lib.MEDOID_TILE
    hit_off, tile_off = _t(np.array([0, M], np.int32)), _t(np.array([0, ntile], np.int32))
    hit_idx = _t(np.arange(M, dtype=np.int32))
    med, cen = _e(1), _e(1, 3, dtype=torch.float32)
    colsum = _e(max(M, 1), dtype=torch.float32) if want_colsum else None      # None: lists of > 512 points take the two-pass route
    ws = _ws(L.cm3d_medoid_workspace_bytes(1, max(M, 1)))
    check(L.cm3d_medoid(pts.data_ptr(), pt_off.data_ptr() if via_rows else 0, mask_frame.data_ptr() if via_rows else 0, 1,
                        hit_off.data_ptr(), tile_off.data_ptr(), hit_idx.data_ptr() if via_rows else 0, max(M, 1), 0, med.data_ptr(),
                        cen.data_ptr(), colsum.data_ptr() if want_colsum else 0, ws.data_ptr(), ws.numel(), _st()), "cm3d_medoid")
    j = int(med.cpu()[0])
    return (j, colsum.cpu().numpy()[:M]) if want_colsum else j


def get_medoids(point_lists, via_rows=False, want_colsum=False):
    """Several lists in ONE call of the medoid stage (one "mask" each; `get_medoid` is the reference's one-list signature): what the
    lists of a batch do to each other -- the two-pass route is taken by lists of more than 256 points when the batch holds one of
    more than 448 (csrc/medoid.hip) -- can only be tested this way.  point_lists: arrays (M_k, 3); returns the list of medoid indices
    (and the exact column sums with want_colsum, which also forces the one-pass route)."""
    L = _lib.lib()
    Ms = [int(np.asarray(p).shape[0]) for p in point_lists]
    n, tot = len(Ms), int(sum(Ms))
    P4 = np.zeros((max(tot, 1), 4), np.float32)
    if tot:
        P4[:tot, :3] = np.concatenate([np.asarray(p, np.float32).reshape(-1, 3) for p in point_lists], 0)
    hit_off = np.concatenate([[0], np.cumsum(Ms)]).astype(np.int32)
    tiles = [(m + _lib.MEDOID_TILE - 1) // _lib.MEDOID_TILE for m in Ms]
    tile_off = np.concatenate([[0], np.cumsum(tiles)]).astype(np.int32)
    pts = _t(P4)
    # gather form: every list is the cloud of a frame of its own, its rows listed in order
    pt_off, mask_frame = _t(hit_off.copy()), _t(np.arange(n, dtype=np.int32))
    hit_idx = _t(np.concatenate([np.arange(m, dtype=np.int32) for m in Ms]) if tot else np.zeros(1, np.int32))
    d_hit_off, d_tile_off = _t(hit_off), _t(tile_off)
    med, cen = _e(n), _e(n, 3, dtype=torch.float32)
    colsum = _e(max(tot, 1), dtype=torch.float32) if want_colsum else None
    ws = _ws(L.cm3d_medoid_workspace_bytes(n, max(tot, 1)))
    check(L.cm3d_medoid(pts.data_ptr(), pt_off.data_ptr() if via_rows else 0, mask_frame.data_ptr() if via_rows else 0, n,
                        d_hit_off.data_ptr(), d_tile_off.data_ptr(), hit_idx.data_ptr() if via_rows else 0, max(tot, 1), 0, med.data_ptr(),
                        cen.data_ptr(), colsum.data_ptr() if want_colsum else 0, ws.data_ptr(), ws.numel(), _st()), "cm3d_medoid")
    out = [int(v) for v in med.cpu().numpy()]
    if want_colsum:
        cs = colsum.cpu().numpy()
        return out, [cs[hit_off[k]:hit_off[k + 1]] for k in range(n)]
    return out


# ----------------------------------------------------------------------------- depth clustering (opt-in)
def depth_cluster_arrays(point_lists, origins, mask_frame, eps, min_points=20, pick="largest", hit_idx=None, with_idx=True):
    """cm3d_depth_cluster on lists laid out back to back (one "mask" each).  point_lists: arrays (n_k, 3) or (n_k, 4) of float32;
    origins (F, 3) float64; mask_frame: the frame of every list; hit_idx: the index entries that travel with the positions (default:
    each list's own positions 0 .. n_k - 1); with_idx=False: the call without hit_idx / cl_idx.  Returns a dict of numpy arrays:
    cl_off, cl_tile_off, cl_status, cl_xyz (cl_off[-1], 4), cl_idx (or None), and hit_off."""
    from .cluster import pick_code
    L = _lib.lib()
    Ms = [int(np.asarray(p).shape[0]) for p in point_lists]
    n, tot = len(Ms), int(sum(Ms))
    cap = max(tot, 1)
    P4 = np.zeros((cap, 4), np.float32)
    o = 0
    for p, m in zip(point_lists, Ms):
        if m:
            p = np.asarray(p, np.float32).reshape(m, -1)
            P4[o:o + m, :p.shape[1]] = p
        o += m
    hit_off = np.concatenate([[0], np.cumsum(Ms)]).astype(np.int32)
    if hit_idx is None:
        hit_idx = np.concatenate([np.arange(m, dtype=np.int32) for m in Ms]) if tot else np.zeros(0, np.int32)
    idx = np.zeros(cap, np.int32)
    idx[:tot] = np.asarray(hit_idx, np.int32)
    org = np.ascontiguousarray(origins, np.float64).reshape(-1, 3)
    d_xyz, d_idx, d_off, d_mf, d_org = _t(P4), _t(idx), _t(hit_off), _t(mask_frame, np.int32), _t(org)
    cl_off, cl_tile, cl_st = _e(n + 1), _e(n + 1), _e(n)
    cl_idx, cl_xyz = _e(cap), _e(cap, 4, dtype=torch.float32)
    ws = _ws(L.cm3d_depth_cluster_workspace_bytes(n, cap))
    check(L.cm3d_depth_cluster(d_xyz.data_ptr(), d_idx.data_ptr() if with_idx else 0, d_off.data_ptr(), d_mf.data_ptr(), n, cap,
                               d_org.data_ptr(), org.shape[0], float(eps), int(min_points), pick_code(pick), cl_off.data_ptr(),
                               cl_tile.data_ptr(), cl_idx.data_ptr() if with_idx else 0, cl_xyz.data_ptr(), cl_st.data_ptr(), ws.data_ptr(),
                               ws.numel(), _st()), "cm3d_depth_cluster")
    off = cl_off.cpu().numpy()
    k = int(off[-1])
    return dict(hit_off=hit_off, cl_off=off, cl_tile_off=cl_tile.cpu().numpy(), cl_status=cl_st.cpu().numpy(),
                cl_xyz=cl_xyz.cpu().numpy()[:k], cl_idx=cl_idx.cpu().numpy()[:k] if with_idx else None)


def depth_cluster(point_lists, origins, eps, min_points=20, pick="largest"):
    """The depth clustering of each list in ONE call of cm3d_depth_cluster (host statement: cluster.depth_cluster_host).  point_lists:
    arrays (n_k, 3) of float32; origins: (3,) for all lists or (n, 3), one per list.  Returns (kept, status): the kept positions of
    each list, ascending, and cl_status (n,)."""
    n = len(point_lists)
    org = np.array(np.broadcast_to(np.asarray(origins, np.float64).reshape(-1, 3), (n, 3))) if n else np.zeros((1, 3))
    r = depth_cluster_arrays(point_lists, org, np.arange(n, dtype=np.int32), eps, min_points, pick)
    return [r["cl_idx"][r["cl_off"][k]:r["cl_off"][k + 1]] for k in range(n)], r["cl_status"]


# ----------------------------------------------------------------------------- yaw fit (opt-in)
def bev_fit(xyz, off, angles=128, d0=0.05, min_points=20, min_length=1.0, idx_cap=None):
    """cm3d_bev_fit on lists laid out back to back (host statement: bevfit.bev_fit_host).  xyz: (n, 2..4) float32, the points of all
    lists; off: int32 (M + 1,), list m at [off[m], off[m + 1]); idx_cap: the capacity the call is told (default: the rows of xyz) --
    offsets beyond it are clamped by the call, nothing at or beyond it is read.  Returns (fit_k (M,), fit_rect (M, 6), fit_status (M,))."""
    from .bevfit import angle_table
    L = _lib.lib()
    p = np.asarray(xyz, np.float32)
    p = p.reshape(-1, p.shape[-1] if p.ndim > 1 else 3)
    cap = int(p.shape[0] if idx_cap is None else idx_cap)
    P4 = np.zeros((max(p.shape[0], cap, 1), 4), np.float32)
    P4[:p.shape[0], :min(p.shape[1], 4)] = p[:, :4]
    off = np.ascontiguousarray(off, np.int32)
    M = off.size - 1
    d_xyz, d_off, d_cs = _t(P4), _t(off), _t(angle_table(angles))
    fk, fr, fs = _e(max(M, 1)), _e(max(M, 1), _lib.MATCH_BOX_STRIDE, dtype=torch.float64), _e(max(M, 1))
    check(L.cm3d_bev_fit(d_xyz.data_ptr(), d_off.data_ptr(), M, max(cap, 1) if M > 0 else 0, d_cs.data_ptr(), int(angles), float(d0),
                         int(min_points), float(min_length), fk.data_ptr(), fr.data_ptr(), fs.data_ptr(), _st()), "cm3d_bev_fit")
    return fk.cpu().numpy()[:M], fr.cpu().numpy()[:M], fs.cpu().numpy()[:M]


def yaw_select(fit_rect, fit_status, medoid_pos, mask_frame, class_id, is_vehicle, lane_dist, lane, lane_off, frame_lane, lane_idx,
               lane_min_dist=0.0, pose_rt=None):
    """cm3d_yaw_select (host statement: bevfit.yaw_select_host).  lane (L, 3) float32 x, y, yaw with lane_off (T + 1,), frame_lane (F,)
    and lane_idx (M,) as cm3d_lane_nn leaves them; pose_rt (F, 12) float32 on Waymo.  Returns (yaw (M,) float32, yaw_idx, yaw_src)."""
    L = _lib.lib()
    M, F = len(medoid_pos), len(frame_lane)
    lane = np.ascontiguousarray(lane, np.float32).reshape(-1, 3)
    c = lambda a, dt: _t(np.array(a, dt))          # (a copy: the caller's arrays may be read-only)
    d = dict(rect=c(fit_rect, np.float64), st=c(fit_status, np.int32), mp=c(medoid_pos, np.int32), mf=c(mask_frame, np.int32),
             cls=c(class_id, np.int32), veh=c(is_vehicle, np.int32), ld=c(lane_dist, np.float64), lane=c(lane, np.float32), lo=c(lane_off, np.int32),
             fl=c(frame_lane, np.int32), li=c(lane_idx, np.int32))
    prt = c(pose_rt, np.float32) if pose_rt is not None else None
    tab, idx, src = _e(M, 3, dtype=torch.float32), _e(M), _e(M)
    check(L.cm3d_yaw_select(d["rect"].data_ptr(), d["st"].data_ptr(), d["mp"].data_ptr(), d["mf"].data_ptr(), d["cls"].data_ptr(),
                            d["veh"].data_ptr(), len(is_vehicle), d["ld"].data_ptr(), float(lane_min_dist), d["lane"].data_ptr(),
                            d["lo"].data_ptr(), d["fl"].data_ptr(), d["li"].data_ptr(), len(lane_off) - 1, lane.shape[0],
                            prt.data_ptr() if prt is not None else 0, M, F, tab.data_ptr(), idx.data_ptr(), src.data_ptr(), _st()),
          "cm3d_yaw_select")
    t = tab.cpu().numpy()
    assert not t[:, :2].any()
    return t[:, 2].copy(), idx.cpu().numpy(), src.cpu().numpy()


# ----------------------------------------------------------------------------- a18 (KITTI)
def obb_yaws(point_lists, vertices=False):
    """Yaw of the oriented box of each list in ONE call of cm3d_obb (one "mask" per list; src/kitti/2d_to_3d.py:855-876, :1524 with
    the canonical eigenvector signs of include/cm3d_hip.h -- host restatement kitti.obb_canonical).  point_lists: arrays (M_k, 3) of
    float32 coordinates.  Returns (yaw (n,) float64, status (n,) int32, R (n, 3, 3) float64); status 0 fitted, 1 <= 3 points (yaw
    NaN), 2 no hull (yaw 0, R identity), 4 not fitted (more than 512 facets seen in one step).  vertices=True adds the list of hull-vertex positions of each list."""
    L = _lib.lib()
    Ms = [int(np.asarray(p).shape[0]) for p in point_lists]
    n, tot = len(Ms), int(sum(Ms))
    P4 = np.zeros((max(tot, 1), 4), np.float32)
    if tot:
        P4[:tot, :3] = np.concatenate([np.asarray(p, np.float32).reshape(-1, 3) for p in point_lists], 0)
    hit_off = np.concatenate([[0], np.cumsum(Ms)]).astype(np.int32)
    idx_cap = max(tot, 1)
    pts, d_off = _t(P4), _t(hit_off)
    yaw, st = _e(n, dtype=torch.float64), _e(n)
    rot = _e(n, _lib.OBB_ROT_STRIDE, dtype=torch.float64)
    vm = _e(idx_cap, dtype=torch.uint8) if vertices else None
    ws = _ws(L.cm3d_obb_workspace_bytes(n, idx_cap))
    check(L.cm3d_obb(pts.data_ptr(), d_off.data_ptr(), n, idx_cap, yaw.data_ptr(), st.data_ptr(), rot.data_ptr(),
                     vm.data_ptr() if vertices else 0, ws.data_ptr(), ws.numel(), _st()), "cm3d_obb")
    out = (yaw.cpu().numpy(), st.cpu().numpy(), rot.cpu().numpy().reshape(n, 3, 3))
    if vertices:
        marks = vm.cpu().numpy()
        out = out + ([np.flatnonzero(marks[hit_off[k]:hit_off[k + 1]]) for k in range(n)],)
    return out


def obb_selftest_yaw(R):
    """The yaw step of cm3d_obb alone (cm3d_selftest_obb_yaw): as_euler('zyx')[0] of each 3x3 matrix of R (n, 3, 3)."""
    L = _lib.lib()
    R = np.ascontiguousarray(np.asarray(R, np.float64).reshape(-1, 9))
    n = R.shape[0]
    d_R, yaw = _t(R), _e(n, dtype=torch.float64)
    check(L.cm3d_selftest_obb_yaw(d_R.data_ptr(), n, yaw.data_ptr(), _st()), "cm3d_selftest_obb_yaw")
    return yaw.cpu().numpy()


# ----------------------------------------------------------------------------- drivable-area polygons
def upload_polygon_index(ix, device=None):
    """A polygon index (drivable.build_index) as device tensors, in the order cm3d_points_in_polygons takes them, plus `n_tables`.
    (Empty arrays get one element: nothing reads it, and a device pointer is never null.)"""
    d = device or _dev()
    out = {k: torch.from_numpy(np.ascontiguousarray(ix[k] if ix[k].size else np.zeros((1,) + ix[k].shape[1:], ix[k].dtype))).to(d)
           for k in _lib.POLY_INDEX_ARRAYS}
    out["n_tables"] = int(ix["n_tables"])
    return out


def points_in_polygons(polygon_tables, xy, table_of_point=None, device_ms=None):
    """eval_detection.point_in_polygons(polygon_tables[table_of_point[i]], *xy[i]) for every point in ONE cm3d_points_in_polygons
    call (eval_custom.py:514-519 for all boxes at once).  polygon_tables: a list of tables as load_drivable_polygons returns them, or
    an index already on the device (upload_polygon_index).  table_of_point None: every point against table 0.  Returns uint8 (n,).
    device_ms: a list that receives the launch's device time in ms (events)."""
    from . import drivable
    L = _lib.lib()
    xy = np.ascontiguousarray(xy, np.float64).reshape(-1, 2)
    n = xy.shape[0]
    if n >= 2 ** 31:
        raise _lib.Cm3dError("cm3d_points_in_polygons: offsets are 32-bit")
    tp = np.zeros(n, np.int32) if table_of_point is None else np.ascontiguousarray(table_of_point, np.int32).reshape(-1)
    if tp.size != n:
        raise ValueError("points_in_polygons: one table per point")
    dix = polygon_tables if isinstance(polygon_tables, dict) else upload_polygon_index(drivable.build_index(polygon_tables))
    if n == 0 or dix["n_tables"] == 0:
        return np.zeros(n, np.uint8)
    d_xy, d_tp, inside = _t(xy), _t(tp), _e(n, dtype=torch.uint8)
    if device_ms is not None:
        ev = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        ev[0].record()
    check(L.cm3d_points_in_polygons(d_xy.data_ptr(), d_tp.data_ptr(), n, *[dix[k].data_ptr() for k in _lib.POLY_INDEX_ARRAYS],
                                    dix["n_tables"], inside.data_ptr(), _st()), "cm3d_points_in_polygons")
    if device_ms is not None:
        ev[1].record()
        ev[1].synchronize()
        device_ms.append(ev[0].elapsed_time(ev[1]))
    return inside.cpu().numpy()


# ----------------------------------------------------------------------------- a10
def lane_yaws_distances_and_coords(all_centroids, all_lane_pts):
    """Returns (yaws, distances, coords) like the reference; yaws/coords are float32-valued."""
    L = _lib.lib()
    cent = np.asarray(all_centroids, np.float64).astype(np.float32).reshape(-1, 3)
    lane = np.asarray(all_lane_pts, np.float64).astype(np.float32).reshape(-1, 3)
    K = cent.shape[0]
    d_c, d_l = _t(cent), _t(lane)
    med = _t(np.zeros(K, np.int32))
    mask_frame = _t(np.zeros(K, np.int32))
    lane_off, frame_lane = _t(np.array([0, lane.shape[0]], np.int32)), _t(np.array([0], np.int32))
    idx, dist = _e(K), _e(K, dtype=torch.float64)
    ws = _ws(L.cm3d_lane_nn_workspace_bytes(K))
    grid = _ws(L.cm3d_lane_grid_bytes(1, lane.shape[0]))
    check(L.cm3d_lane_grid_build(d_l.data_ptr(), lane_off.data_ptr(), 1, lane.shape[0], grid.data_ptr(), grid.numel(), _st()),
          "cm3d_lane_grid_build")
    check(L.cm3d_lane_nn(d_c.data_ptr(), med.data_ptr(), mask_frame.data_ptr(), K, d_l.data_ptr(), lane_off.data_ptr(),
                         frame_lane.data_ptr(), 1, lane.shape[0], grid.data_ptr(), idx.data_ptr(), dist.data_ptr(), ws.data_ptr(),
                         ws.numel(), _st()), "cm3d_lane_nn")
    j = idx.cpu().numpy()
    return lane[j, 2], dist.cpu().numpy(), lane[j, :2]


# ----------------------------------------------------------------------------- a11-a15
def _box_nms(centroids, class_ids, scores, yaws, ego_xyz, classes, valid=None):
    """One frame through cm3d_box_nms with given lane yaws (a one-point lane table per mask)."""
    L = _lib.lib()
    cent = np.asarray(centroids, np.float32).reshape(-1, 3)
    n = cent.shape[0]
    lane = np.zeros((n, 3), np.float32)
    lane[:, 2] = np.asarray(yaws, np.float32)
    med = np.zeros(n, np.int32) if valid is None else np.where(np.asarray(valid, bool), 0, -1).astype(np.int32)
    d = dict(cent=_t(cent), med=_t(med), mask_off=_t(np.array([0, n], np.int32)), cls=_t(np.asarray(class_ids, np.int32)),
             score=_t(np.asarray(scores, np.float64)), lane=_t(lane), lane_off=_t(np.array([0, n], np.int32)),
             frame_lane=_t(np.array([0], np.int32)), lane_idx=_t(np.arange(n, dtype=np.int32)), lane_dist=_t(np.zeros(n, np.float64)),
             prior=_t(classes.prior_wlh), veh=_t(classes.is_vehicle), thr=_t(classes.nms_thr),
             grp=_t(np.ascontiguousarray(classes.nms_group, np.int32)), ego=_t(np.asarray(ego_xyz, np.float64).reshape(1, 3)))
    box, flags = _e(n, _lib.BOX_STRIDE, dtype=torch.float64), _e(n)
    check(L.cm3d_box_nms(d["cent"].data_ptr(), d["med"].data_ptr(), d["mask_off"].data_ptr(), 1, n, d["cls"].data_ptr(),
                         d["score"].data_ptr(), d["lane"].data_ptr(), d["lane_off"].data_ptr(), d["frame_lane"].data_ptr(),
                         d["lane_idx"].data_ptr(), d["lane_dist"].data_ptr(), d["prior"].data_ptr(), d["veh"].data_ptr(),
                         d["grp"].data_ptr(), d["thr"].data_ptr(), len(classes.names), d["ego"].data_ptr(), 0, box.data_ptr(),
                         flags.data_ptr(), _st()),
          "cm3d_box_nms")
    return box.cpu().numpy(), flags.cpu().numpy()


def push_centroid(centroid, class_name, lane_yaw, poserecord, classes=None):
    """Returns (pushed_centroid (3,), rotation wxyz (4,)) for one box of a pushed class."""
    from .lifting import ClassTable
    classes = classes or ClassTable.nuscenes()
    box, _ = _box_nms([centroid], [classes.index(class_name)], [1.0], [lane_yaw], poserecord["translation"], classes)
    return box[0, 0:3].copy(), np.array([box[0, 3], 0.0, 0.0, box[0, 4]])


def circle_nms(dets, det_labels, threshs_by_label):
    """dets (n,3) x,y,score; det_labels list of class names; returns the kept indices (ascending),
    i.e. sorted(reference circle_nms(...))."""
    L = _lib.lib()
    names = list(threshs_by_label.keys())
    dets = np.asarray(dets, np.float64).reshape(-1, 3)
    n = dets.shape[0]
    if n == 0:
        return []
    x, y, sc = _t(dets[:, 0].copy()), _t(dets[:, 1].copy()), _t(dets[:, 2].copy())
    lab = _t(np.array([names.index(l) for l in det_labels], np.int32))
    thr = _t(np.array([threshs_by_label[k] for k in names], np.float64))
    off = _t(np.array([0, n], np.int32))
    keep = _e(n)
    check(L.cm3d_circle_nms(x.data_ptr(), y.data_ptr(), sc.data_ptr(), lab.data_ptr(), off.data_ptr(), 1, thr.data_ptr(),
                            len(names), keep.data_ptr(), _st()), "cm3d_circle_nms")
    return np.flatnonzero(keep.cpu().numpy()).tolist()


def rotated_nms(rec, score, group, frame_off, thr, measure="iou", class_agnostic=False):
    """The opt-in rotated-box NMS on records (cm3d_rotated_nms; nms.rotated_nms_host states it): rec (n, 6) cx, cy, length, width,
    c, s; score (n,); group (n,) NMS group of each box; frame_off (F + 1,); thr: one float or one per group.  Returns keep (n,) int32."""
    from . import nms as nmsmod
    L = _lib.lib()
    rec = np.asarray(rec, np.float64).reshape(-1, 6)
    n = rec.shape[0]
    off = np.asarray(frame_off, np.int32).reshape(-1)
    thr = np.atleast_1d(np.asarray(thr, np.float64))
    if n == 0 or off.size < 2:
        return np.zeros(n, np.int32)
    d_rec, d_sc, d_grp = _t(rec), _t(np.asarray(score, np.float64).reshape(n)), _t(np.asarray(group, np.int32).reshape(n))
    d_off, d_thr = _t(off), _t(thr)
    keep = _e(n)
    check(L.cm3d_rotated_nms(d_rec.data_ptr(), d_sc.data_ptr(), d_grp.data_ptr(), d_off.data_ptr(), off.size - 1, d_thr.data_ptr(),
                             thr.size, nmsmod.measure_code(measure), int(bool(class_agnostic)), keep.data_ptr(), _st()), "cm3d_rotated_nms")
    return keep.cpu().numpy()


def box_velocity(box, flags, mask_off, class_id, frame_next, frame_time, track_group, max_speed, max_dt=1.5, out=None):
    """The opt-in velocity stage on arrays (cm3d_box_velocity; velocity.track_velocity_host states it): box (M, BOX_STRIDE) float64 and
    flags (M,) as a pass left them, mask_off (F + 1,), class_id (M,), frame_next (F,), frame_time (F,) seconds, track_group per class,
    max_speed per group.  out: optional dict of device tensors next_match, prev_match, vel_src (M,) int32 and vel (M, 2) float64 to
    write into (else allocated).  Returns a dict of numpy arrays next_match, prev_match, vel, vel_src and `status` (int; the bits of the
    header, not raised: a caller decides)."""
    from . import velocity as velmod
    L = _lib.lib()
    box = np.asarray(box, np.float64).reshape(-1, _lib.BOX_STRIDE)
    M = box.shape[0]
    off = np.asarray(mask_off, np.int32).reshape(-1)
    F = off.size - 1
    nxt, tim = np.asarray(frame_next, np.int32).reshape(F), np.asarray(frame_time, np.float64).reshape(F)
    grp, spd = np.asarray(track_group, np.int32).reshape(-1), np.asarray(max_speed, np.float64).reshape(-1)
    pair_off = velmod.link_table(off, nxt, tim, float(max_dt), M)[2]
    total = int(pair_off[-1])
    d_box, d_flags = _t(box if M else np.zeros((1, _lib.BOX_STRIDE))), _t(np.asarray(flags, np.int32).reshape(M) if M else np.zeros(1, np.int32))
    d_cls = _t(np.asarray(class_id, np.int32).reshape(M) if M else np.zeros(1, np.int32))
    d_off, d_nxt, d_tim, d_grp, d_spd, d_pair = _t(off), _t(nxt), _t(tim), _t(grp), _t(spd), _t(pair_off)
    o = out or {}
    nm, pm, src = (o[k] if k in o else _e(max(M, 1)) for k in ("next_match", "prev_match", "vel_src"))
    vel = o["vel"] if "vel" in o else _e(max(M, 1), 2, dtype=torch.float64)
    status = torch.zeros(1, dtype=torch.int32, device=_dev())
    ws = _ws(L.cm3d_box_velocity_workspace_bytes(total, M))
    check(L.cm3d_box_velocity(d_box.data_ptr(), d_flags.data_ptr(), d_off.data_ptr(), F, M, d_cls.data_ptr(), d_grp.data_ptr(),
                              d_spd.data_ptr(), grp.size, spd.size, d_nxt.data_ptr(), d_tim.data_ptr(), float(max_dt), d_pair.data_ptr(), F,
                              total, nm.data_ptr(), pm.data_ptr(), vel.data_ptr(), src.data_ptr(), status.data_ptr(), ws.data_ptr(),
                              ws.numel(), _st()), "cm3d_box_velocity")
    return dict(next_match=nm.cpu().numpy()[:M], prev_match=pm.cpu().numpy()[:M], vel=vel.cpu().numpy().reshape(-1, 2)[:M], vel_src=src.cpu().numpy()[:M],
                status=int(status.item()))


def box_tracks(box, flags, mask_frame, next_match, prev_match, frame_time, min_length=1, score="own", smooth_window=0, out=None):
    """The opt-in track stage on arrays (cm3d_box_tracks; tracks.box_tracks_host states it): box (M, BOX_STRIDE) float64 and flags (M,)
    as a pass left them, mask_frame (M,), next_match / prev_match (M,) as box_velocity left them, frame_time (F,) seconds.  out: optional
    dict of device tensors track_id, track_pos, track_len (M,) int32, track_stat (M, 4), vel_smooth (M, 2) float64, and box (M, BOX_STRIDE)
    float64, flags (M,) int32 to work in (else allocated; box and flags are filled from the arguments either way).  Returns a dict of
    numpy arrays: the five outputs (vel_smooth only for smooth_window > 0), the new `box` and `flags`, and `status` (int; the bits of
    the header, not raised: a caller decides)."""
    from . import tracks as trmod
    L = _lib.lib()
    box = np.asarray(box, np.float64).reshape(-1, _lib.BOX_STRIDE)
    M = box.shape[0]
    tim = np.asarray(frame_time, np.float64).reshape(-1)
    W = int(smooth_window)
    o = out or {}
    n = max(M, 1)
    i32 = lambda a: np.asarray(a, np.int32).reshape(M) if M else np.zeros(1, np.int32)
    if "box" in o:
        d_box, d_flags = o["box"], o["flags"]
        if M:
            d_box.view(-1)[:M * _lib.BOX_STRIDE].copy_(_t(box).view(-1)); d_flags.view(-1)[:M].copy_(_t(i32(flags)))
    else:
        d_box, d_flags = _t(box if M else np.zeros((1, _lib.BOX_STRIDE))), _t(i32(flags))
    d_frm, d_nm, d_pm, d_tim = _t(i32(mask_frame)), _t(i32(next_match)), _t(i32(prev_match)), _t(tim if tim.size else np.zeros(1))
    tid, pos, ln = (o[k] if k in o else _e(n) for k in ("track_id", "track_pos", "track_len"))
    stat = o["track_stat"] if "track_stat" in o else _e(n, 4, dtype=torch.float64)
    vs = (o["vel_smooth"] if "vel_smooth" in o else _e(n, 2, dtype=torch.float64)) if W > 0 else None
    status = torch.zeros(1, dtype=torch.int32, device=_dev())
    ws = _ws(L.cm3d_box_tracks_workspace_bytes(M))
    check(L.cm3d_box_tracks(d_box.data_ptr(), d_flags.data_ptr(), d_frm.data_ptr(), d_nm.data_ptr(), d_pm.data_ptr(), d_tim.data_ptr(), M,
                            tim.size, int(min_length), trmod.score_code(score), W, tid.data_ptr(), pos.data_ptr(), ln.data_ptr(),
                            stat.data_ptr(), vs.data_ptr() if vs is not None else None, status.data_ptr(), ws.data_ptr(), ws.numel(), _st()),
          "cm3d_box_tracks")
    res = dict(track_id=tid.cpu().numpy().reshape(-1)[:M], track_pos=pos.cpu().numpy().reshape(-1)[:M], track_len=ln.cpu().numpy().reshape(-1)[:M],
               track_stat=stat.cpu().numpy().reshape(-1, 4)[:M], box=d_box.cpu().numpy().reshape(-1, _lib.BOX_STRIDE)[:M],
               flags=d_flags.cpu().numpy().reshape(-1)[:M], status=int(status.item()))
    if vs is not None:
        res["vel_smooth"] = vs.cpu().numpy().reshape(-1, 2)[:M]
    return res


def box_size(box, flags, mask_frame, fit_rect, place_src, prior_wlh, ego_xyz, next_match, prev_match, track_id, track_pos, track_len,
             frame_time, thin=0.5, max_dt=1.5, smooth_window=0, q=0.75, min_obs=2, lo=0.6, hi=1.5):
    """The opt-in size stage on arrays (cm3d_box_size; boxsize.box_size_host states it and takes the same arguments): box, flags as the
    placed pass and the track stage left them, fit_rect (M, 6), place_src (M,), prior_wlh (C, 3), ego_xyz (F, 3) or None (Waymo), the
    match arrays of box_velocity, the track arrays of box_tracks, frame_time (F,).  Returns a dict of numpy arrays: size_wlh (M, 3),
    size_src (M,), size_ratio (M, 2), size_obs (M, 2), size_placed (M, 2), size_vel (M, 2), the new `box`, `flags`, and `status` (int;
    the bits of the header, not raised: a caller decides).  The four parameters' defaults are untuned."""
    L = _lib.lib()
    box = np.asarray(box, np.float64).reshape(-1, _lib.BOX_STRIDE)
    M = box.shape[0]
    tim = np.asarray(frame_time, np.float64).reshape(-1)
    prior = np.asarray(prior_wlh, np.float64).reshape(-1, 3)
    n = max(M, 1)
    i32 = lambda a: _t(np.asarray(a, np.int32).reshape(M) if M else np.zeros(1, np.int32))
    d_box, d_flags = _t(box if M else np.zeros((1, _lib.BOX_STRIDE))), i32(flags)
    d_rect = _t(np.asarray(fit_rect, np.float64).reshape(M, _lib.MATCH_BOX_STRIDE) if M else np.zeros((1, _lib.MATCH_BOX_STRIDE)))
    d_int = [i32(a) for a in (mask_frame, place_src, next_match, prev_match, track_id, track_pos, track_len)]
    d_frm, d_src, d_nm, d_pm, d_tid, d_pos, d_len = d_int
    d_prior, d_tim = _t(prior), _t(tim if tim.size else np.zeros(1))
    d_ego = None if ego_xyz is None else _t(np.asarray(ego_xyz, np.float64).reshape(-1, 3))
    wlh, ratio, placed, vel = (_e(n, w, dtype=torch.float64) for w in (3, 2, 2, 2))
    src, obs = _e(n), _e(n, 2)
    status = torch.zeros(1, dtype=torch.int32, device=_dev())
    ws = _ws(L.cm3d_box_size_workspace_bytes(M))
    check(L.cm3d_box_size(d_box.data_ptr(), d_flags.data_ptr(), d_frm.data_ptr(), d_rect.data_ptr(), d_src.data_ptr(), d_prior.data_ptr(),
                          prior.shape[0], d_ego.data_ptr() if d_ego is not None else None, int(d_ego is None), float(thin), d_nm.data_ptr(),
                          d_pm.data_ptr(), d_tid.data_ptr(), d_pos.data_ptr(), d_len.data_ptr(), d_tim.data_ptr(), M, tim.size, float(max_dt),
                          int(smooth_window), float(q), int(min_obs), float(lo), float(hi), wlh.data_ptr(), src.data_ptr(), ratio.data_ptr(),
                          obs.data_ptr(), placed.data_ptr(), vel.data_ptr(), status.data_ptr(), ws.data_ptr(), ws.numel(), _st()),
          "cm3d_box_size")
    f64 = lambda a, w: a.cpu().numpy().reshape(-1, w)[:M]
    return dict(size_wlh=f64(wlh, 3), size_src=src.cpu().numpy().reshape(-1)[:M], size_ratio=f64(ratio, 2),
                size_obs=obs.cpu().numpy().reshape(-1, 2)[:M], size_placed=f64(placed, 2), size_vel=f64(vel, 2),
                box=f64(d_box, _lib.BOX_STRIDE), flags=d_flags.cpu().numpy().reshape(-1)[:M], status=int(status.item()))


def box_vertical(xyz, off, box, flags, prior_wlh, q_bot=0.02, q_top=0.98, min_points=5, lo=0.7, hi=1.3, idx_cap=None):
    """The opt-in vertical stage on arrays (cm3d_box_vertical; boxvertical.box_vertical_host states it): xyz (n, 4) float32, the points
    of all lists; off int32 (M + 1,); idx_cap: the capacity the call is told (default: the rows of xyz) -- offsets beyond it are
    clamped by the call, nothing at or beyond it is read; box (M, BOX_STRIDE), flags (M,), prior_wlh (C, 3).  Returns a dict of numpy
    arrays: vert_z (M, 2), vert_h (M,), vert_src (M,), vert_status (M,), vert_entry_z (M,) and the new `box`.  The defaults are untuned."""
    L = _lib.lib()
    p = np.asarray(xyz, np.float32).reshape(-1, 4)
    cap = int(p.shape[0] if idx_cap is None else idx_cap)
    P4 = np.zeros((max(p.shape[0], cap, 1), 4), np.float32)
    P4[:p.shape[0]] = p
    off = np.ascontiguousarray(off, np.int32).reshape(-1)
    M = off.size - 1
    box = np.asarray(box, np.float64).reshape(-1, _lib.BOX_STRIDE)
    prior = np.asarray(prior_wlh, np.float64).reshape(-1, 3)
    if box.shape[0] != M:
        raise ValueError("one offset more than boxes")
    n = max(M, 1)
    d_xyz, d_off, d_prior = _t(P4), _t(off), _t(prior if prior.size else np.zeros((1, 3)))
    d_box = _t(box if M else np.zeros((1, _lib.BOX_STRIDE)))
    d_flags = _t(np.asarray(flags, np.int32).reshape(M) if M else np.zeros(1, np.int32))
    vz, vh, ez = _e(n, 2, dtype=torch.float64), _e(n, dtype=torch.float64), _e(n, dtype=torch.float64)
    src, status = _e(n), _e(n)
    check(L.cm3d_box_vertical(d_xyz.data_ptr(), d_off.data_ptr(), M, cap, d_box.data_ptr(), d_flags.data_ptr(), d_prior.data_ptr(),
                              prior.shape[0], float(q_bot), float(q_top), int(min_points), float(lo), float(hi), vz.data_ptr(), vh.data_ptr(),
                              src.data_ptr(), status.data_ptr(), ez.data_ptr(), _st()), "cm3d_box_vertical")
    return dict(vert_z=vz.cpu().numpy()[:M], vert_h=vh.cpu().numpy()[:M], vert_src=src.cpu().numpy()[:M],
                vert_status=status.cpu().numpy()[:M], vert_entry_z=ez.cpu().numpy()[:M], box=d_box.cpu().numpy()[:M])


def _filled(fill, *shape, dtype=torch.int32):
    """An output buffer: uninitialised, or every byte `fill` (the tests' poison)."""
    t = _e(*shape, dtype=dtype)
    if fill is not None:
        t.view(torch.uint8).fill_(int(fill))
    return t


def hit_project(xyz, off, mask_frame, mask_cam, cams, idx_cap=None, fill=None):
    """Step 1 of the virtual-point stage on arrays (cm3d_hit_project): xyz (n, 4) float32, the points of all lists; off int32 (M + 1,);
    mask_frame, mask_cam (M,); cams (F, n_cams, CAM_STRIDE) float32; idx_cap: the capacity the call is told (default: the rows of xyz).
    Returns hit_uvd (max(n, idx_cap), 4) float32: (u, v, depth, 0) of every list position below idx_cap; the other rows keep what the
    buffer held (`fill`: that byte everywhere before the call)."""
    L = _lib.lib()
    p = np.asarray(xyz, np.float32).reshape(-1, 4)
    cap = int(p.shape[0] if idx_cap is None else idx_cap)
    rows = max(p.shape[0], cap, 1)
    P4 = np.zeros((rows, 4), np.float32)
    P4[:p.shape[0]] = p
    off = np.ascontiguousarray(off, np.int32).reshape(-1)
    M = off.size - 1
    cams = np.ascontiguousarray(cams, np.float32).reshape(-1, np.shape(cams)[-2], _lib.CAM_STRIDE)
    F, n_cams = cams.shape[0], cams.shape[1]
    d_frame = _t(np.asarray(mask_frame, np.int32).reshape(M) if M else np.zeros(1, np.int32))
    d_cam = _t(np.asarray(mask_cam, np.int32).reshape(M) if M else np.zeros(1, np.int32))
    d_xyz, d_off, d_cams = _t(P4), _t(off), _t(cams)
    uvd = _filled(fill, rows, 4, dtype=torch.float32)
    check(L.cm3d_hit_project(d_xyz.data_ptr(), d_off.data_ptr(), d_frame.data_ptr(), d_cam.data_ptr(), d_cams.data_ptr(), n_cams, F, M, cap,
                             uvd.data_ptr(), _st()), "cm3d_hit_project")
    return uvd.cpu().numpy()


def virtual_points(packed, bbox, W, H, cams, mask_off, mask_frame, mask_cam, flags, hit_uvd, off, per_mask=50, seed=0, max_px=0.0,
                   kept_only=True, frame_seed=None, idx_cap=None, fill=None):
    """The virtual-point stage on arrays (cm3d_virtual_points; virtualpoints.virtual_points_host states it): packed, M slots of H * Wp
    words, and bbox (M, BBOX_STRIDE) as the mask kernels leave them; cams (F, n_cams, CAM_STRIDE) float32; mask_off (F + 1,); mask_frame,
    mask_cam, flags (M,; flags may be None without kept_only); hit_uvd (n, 4) float32 (hit_project); off int32 (M + 1,); frame_seed (F,)
    uint32, None: arange(F); idx_cap: the capacity the call is told (default: the rows of hit_uvd).  Returns a dict of the seven whole
    output arrays: rows behind a mask's count keep what the buffers held (`fill`: that byte everywhere before the call).  The defaults
    are untuned."""
    L = _lib.lib()
    W, H, K = int(W), int(H), int(per_mask)
    Wp = (W + 31) // 32
    bbox = np.ascontiguousarray(bbox, np.int32).reshape(-1, _lib.BBOX_STRIDE)
    M = bbox.shape[0]
    uvd = np.asarray(hit_uvd, np.float32).reshape(-1, 4)
    cap = int(uvd.shape[0] if idx_cap is None else idx_cap)
    U4 = np.zeros((max(uvd.shape[0], cap, 1), 4), np.float32)
    U4[:uvd.shape[0]] = uvd
    cams = np.ascontiguousarray(cams, np.float32).reshape(-1, np.shape(cams)[-2], _lib.CAM_STRIDE)
    F, n_cams = cams.shape[0], cams.shape[1]
    words = np.ascontiguousarray(packed).view(np.int32).reshape(-1)
    if words.size != M * H * Wp:
        raise ValueError("packed: one slot of H * Wp words per mask")
    fs = np.arange(F, dtype=np.uint32) if frame_seed is None else np.asarray(frame_seed).astype(np.uint32).reshape(F)
    one = np.zeros(1, np.int32)
    d_packed, d_bbox = _t(words if M else one), _t(bbox if M else np.zeros((1, _lib.BBOX_STRIDE), np.int32))
    d_cams, d_moff, d_fs = _t(cams), _t(np.asarray(mask_off, np.int32).reshape(-1)), _t(fs.view(np.int32) if F else one)
    d_frame = _t(np.asarray(mask_frame, np.int32).reshape(M) if M else one)
    d_cam = _t(np.asarray(mask_cam, np.int32).reshape(M) if M else one)
    d_flags = None if flags is None else _t(np.asarray(flags, np.int32).reshape(M) if M else one)
    d_uvd, d_off = _t(U4), _t(np.ascontiguousarray(off, np.int32).reshape(-1))
    n, nk = max(M, 1), max(M * max(K, 1), 1)
    count, status = _filled(fill, n), _filled(fill, n)
    xyz, pix, src = _filled(fill, nk, 3, dtype=torch.float64), _filled(fill, nk, 2), _filled(fill, nk)
    depth, d2 = _filled(fill, nk, dtype=torch.float32), _filled(fill, nk, dtype=torch.float32)
    check(L.cm3d_virtual_points(d_packed.data_ptr(), d_bbox.data_ptr(), W, H, d_cams.data_ptr(), n_cams, d_moff.data_ptr(), d_frame.data_ptr(),
                                d_cam.data_ptr(), None if d_flags is None else d_flags.data_ptr(), F, M, d_uvd.data_ptr(), d_off.data_ptr(), cap,
                                K, int(seed) & 0xFFFFFFFF, float(max_px), int(bool(kept_only)), d_fs.data_ptr(), count.data_ptr(),
                                status.data_ptr(), xyz.data_ptr(), pix.data_ptr(), src.data_ptr(), depth.data_ptr(), d2.data_ptr(), _st()),
          "cm3d_virtual_points")
    return dict(vp_count=count.cpu().numpy(), vp_status=status.cpu().numpy(), vp_xyz=xyz.cpu().numpy(), vp_pix=pix.cpu().numpy(),
                vp_src=src.cpu().numpy(), vp_depth=depth.cpu().numpy(), vp_d2=d2.cpu().numpy())


def box_ground(box, flags, prior_wlh, mask_off, points=None, pt_off=None, raw=None, raw_stride=4, sweep_xf=None, sweep_row_off=None,
               frame_sweep_off=None, halfw=0.0, zref=None, vert=None, zref_aliases=False, radius=3.0, quantile=0.1, min_points=20, down=5.0,
               up=0.5, lo=0.7, hi=1.3):
    """The opt-in ground stage on arrays (cm3d_box_ground; boxground.box_ground_host states it).  The cloud is either points (n, 4)
    float32 with pt_off (F + 1,), or the raw rows as cm3d_sweep_prep takes them: raw (flat float32), raw_stride (4 and up, or
    _lib.RAW_QUADS), sweep_xf (S, 24), sweep_row_off (S + 1,), frame_sweep_off (F + 1,), halfw.  box (M, BOX_STRIDE), flags (M,),
    prior_wlh (C, 3), mask_off (F + 1,); zref (M,) or None (column 2 of box); vert: None or the vertical stage's outputs (vert_status,
    vert_z, vert_h).  zref_aliases: hand zref in the very array ground_zref is written to.  Returns a dict of numpy arrays: the six
    boxground.RESULTS and the new `box`.  The defaults are untuned."""
    L = _lib.lib()
    box = np.asarray(box, np.float64).reshape(-1, _lib.BOX_STRIDE)
    M = box.shape[0]
    prior = np.asarray(prior_wlh, np.float64).reshape(-1, 3)
    mask_off = np.ascontiguousarray(mask_off, np.int32).reshape(-1)
    F = mask_off.size - 1
    n = max(M, 1)
    d_box = _t(box if M else np.zeros((1, _lib.BOX_STRIDE)))
    d_flags = _t(np.asarray(flags, np.int32).reshape(M) if M else np.zeros(1, np.int32))
    d_prior, d_moff = _t(prior if prior.size else np.zeros((1, 3))), _t(mask_off)
    null = lambda a: None if a is None else a.data_ptr()
    d_pts = d_poff = d_raw = d_xf = d_roff = d_soff = None
    n_sweeps = 0
    if points is not None:
        p = np.asarray(points, np.float32).reshape(-1, 4)
        n_rows = p.shape[0]
        d_pts, d_poff = _t(p if n_rows else np.zeros((1, 4), np.float32)), _t(np.asarray(pt_off, np.int32).reshape(F + 1))
    else:
        sweep_row_off = np.ascontiguousarray(sweep_row_off, np.int32).reshape(-1)
        n_sweeps, n_rows = sweep_row_off.size - 1, int(sweep_row_off[-1])
        r = np.asarray(raw, np.float32).reshape(-1)
        need = (n_rows + 3) // 4 * 12 if raw_stride == _lib.RAW_QUADS else n_rows * int(raw_stride)
        if r.size < need:
            raise ValueError(f"raw: {r.size} floats for {n_rows} rows")
        d_raw, d_xf = _t(r if r.size else np.zeros(12, np.float32)), _t(np.asarray(sweep_xf, np.float32).reshape(max(n_sweeps, 0), 24))
        d_roff, d_soff = _t(sweep_row_off), _t(np.asarray(frame_sweep_off, np.int32).reshape(F + 1))
    gz, gh, gr = (_e(n, dtype=torch.float64) for _ in range(3))
    gn, src, status = _e(n), _e(n), _e(n)
    d_zref = None
    if zref is not None:
        d_zref = _t(np.asarray(zref, np.float64).reshape(M) if M else np.zeros(1))
        if zref_aliases:
            gr = d_zref
    d_vs = d_vz = d_vh = None
    if vert is not None:
        d_vs = _t(np.asarray(vert["vert_status"], np.int32).reshape(M) if M else np.zeros(1, np.int32))
        d_vz = _t(np.asarray(vert["vert_z"], np.float64).reshape(M, 2) if M else np.zeros((1, 2)))
        d_vh = _t(np.asarray(vert["vert_h"], np.float64).reshape(M) if M else np.zeros(1))
    nm_max = int(np.diff(mask_off).max()) if F > 0 else 0
    check(L.cm3d_box_ground(null(d_pts), null(d_poff), null(d_raw), int(raw_stride), null(d_xf), null(d_roff), null(d_soff), n_sweeps,
                            float(halfw), n_rows, d_moff.data_ptr(), F, M, max(nm_max, 0), d_box.data_ptr(), d_flags.data_ptr(),
                            d_prior.data_ptr(), prior.shape[0], null(d_zref), null(d_vs), null(d_vz), null(d_vh), float(radius),
                            float(quantile), int(min_points), float(down), float(up), float(lo), float(hi), gz.data_ptr(), gn.data_ptr(),
                            gh.data_ptr(), src.data_ptr(), status.data_ptr(), gr.data_ptr(), _st()), "cm3d_box_ground")
    return dict(ground_z=gz.cpu().numpy()[:M], ground_n=gn.cpu().numpy()[:M], ground_h=gh.cpu().numpy()[:M],
                ground_src=src.cpu().numpy()[:M], ground_status=status.cpu().numpy()[:M], ground_zref=gr.cpu().numpy()[:M],
                box=d_box.cpu().numpy()[:M])


# ----------------------------------------------------------------------------- ground strip (opt-in)
def ground_grid(origin, points=None, pt_off=None, raw=None, raw_stride=4, sweep_xf=None, sweep_row_off=None, frame_sweep_off=None, halfw=0.0,
                cell=2.0, down=4.0, up=4.0, quantile=0.1, min_points=8):
    """The per-frame ground grid on arrays (cm3d_ground_grid; groundstrip.ground_grid_host states it).  origin (F, 3) float64; the cloud
    is either points (n, 4) float32 with pt_off (F + 1,), or the raw rows as box_ground takes them.  Returns (grid_z (F, 4096) float64,
    grid_n (F, 4096) int32).  The defaults are untuned."""
    from .groundstrip import N_CELLS
    L = _lib.lib()
    org = np.ascontiguousarray(origin, np.float64).reshape(-1, 3)
    F = org.shape[0]
    null = lambda a: None if a is None else a.data_ptr()
    d_pts = d_poff = d_raw = d_xf = d_roff = d_soff = None
    n_sweeps = 0
    if points is not None:
        p = np.asarray(points, np.float32).reshape(-1, 4)
        n_rows = p.shape[0]
        d_pts, d_poff = _t(p if n_rows else np.zeros((1, 4), np.float32)), _t(np.asarray(pt_off, np.int32).reshape(F + 1))
    else:
        sweep_row_off = np.ascontiguousarray(sweep_row_off, np.int32).reshape(-1)
        n_sweeps, n_rows = sweep_row_off.size - 1, int(sweep_row_off[-1])
        r = np.asarray(raw, np.float32).reshape(-1)
        need = (n_rows + 3) // 4 * 12 if raw_stride == _lib.RAW_QUADS else n_rows * int(raw_stride)
        if r.size < need:
            raise ValueError(f"raw: {r.size} floats for {n_rows} rows")
        d_raw, d_xf = _t(r if r.size else np.zeros(12, np.float32)), _t(np.asarray(sweep_xf, np.float32).reshape(max(n_sweeps, 0), 24))
        d_roff, d_soff = _t(sweep_row_off), _t(np.asarray(frame_sweep_off, np.int32).reshape(F + 1))
    gz, gn = _e(max(F, 1), N_CELLS, dtype=torch.float64), _e(max(F, 1), N_CELLS)
    check(L.cm3d_ground_grid(null(d_pts), null(d_poff), null(d_raw), int(raw_stride), null(d_xf), null(d_roff), null(d_soff), n_sweeps,
                             float(halfw), n_rows, _t(org if F else np.zeros((1, 3))).data_ptr(), F, float(cell), float(down), float(up),
                             float(quantile), int(min_points), gz.data_ptr(), gn.data_ptr(), _st()), "cm3d_ground_grid")
    return gz.cpu().numpy()[:F], gn.cpu().numpy()[:F]


def ground_strip(hit_xyz, hit_off, mask_frame, origin, grid_z, hit_idx=None, cell=2.0, margin=0.3, min_keep=5, idx_cap=None):
    """The strip of the in-mask lists on arrays (cm3d_ground_strip; groundstrip.ground_strip_host states it).  hit_xyz (n, 3 or 4)
    float32, hit_off (M + 1,), mask_frame (M,), origin (F, 3), grid_z (F, 4096) as ground_grid returns it; hit_idx (n,) or None: the call
    without hit_idx / gs_idx.  idx_cap: the capacity the call is told (default: the number of positions).  Returns a dict of numpy
    arrays: gs_off, gs_tile_off, gs_status, gs_dropped, gs_xyz (gs_off[-1], 4), gs_idx (or None).  The defaults are untuned."""
    from .groundstrip import N_CELLS
    L = _lib.lib()
    p = np.asarray(hit_xyz, np.float32)
    p = p.reshape(-1, p.shape[-1] if p.ndim > 1 else 4)
    tot = p.shape[0]
    cap = max(tot, 1) if idx_cap is None else int(idx_cap)
    P4 = np.zeros((max(tot, cap, 1), 4), np.float32)
    P4[:tot, :min(p.shape[1], 4)] = p[:, :4]
    hit_off = np.ascontiguousarray(hit_off, np.int32).reshape(-1)
    M = hit_off.size - 1
    org, gz = np.ascontiguousarray(origin, np.float64).reshape(-1, 3), np.ascontiguousarray(grid_z, np.float64).reshape(-1, N_CELLS)
    F = org.shape[0]
    idx = None
    if hit_idx is not None:
        idx = np.zeros(P4.shape[0], np.int32)
        idx[:tot] = np.asarray(hit_idx, np.int32)
    n = max(M, 1)
    d_xyz, d_idx, d_off = _t(P4), None if idx is None else _t(idx), _t(hit_off)
    d_mf = _t(np.asarray(mask_frame, np.int32).reshape(M) if M else np.zeros(1, np.int32))
    d_org, d_gz = _t(org if F else np.zeros((1, 3))), _t(gz if F else np.zeros((1, N_CELLS)))
    gs_off, gs_tile, gs_st, gs_dr = _e(n + 1), _e(n + 1), _e(n), _e(n)
    gs_idx, gs_xyz = (None if idx is None else _e(P4.shape[0])), _e(P4.shape[0], 4, dtype=torch.float32)
    ws = _ws(L.cm3d_ground_strip_workspace_bytes(M, cap))
    check(L.cm3d_ground_strip(d_xyz.data_ptr(), None if d_idx is None else d_idx.data_ptr(), d_off.data_ptr(), d_mf.data_ptr(), M, cap,
                              d_org.data_ptr(), d_gz.data_ptr(), F, float(cell), float(margin), int(min_keep), gs_off.data_ptr(),
                              gs_tile.data_ptr(), None if gs_idx is None else gs_idx.data_ptr(), gs_xyz.data_ptr(), gs_st.data_ptr(),
                              gs_dr.data_ptr(), ws.data_ptr(), ws.numel(), _st()), "cm3d_ground_strip")
    if M == 0:
        return dict(gs_off=np.zeros(1, np.int32), gs_tile_off=np.zeros(1, np.int32), gs_status=np.zeros(0, np.int32),
                    gs_dropped=np.zeros(0, np.int32), gs_xyz=np.zeros((0, 4), np.float32), gs_idx=None if idx is None else np.zeros(0, np.int32))
    off = gs_off.cpu().numpy()
    k = int(off[-1])
    return dict(gs_off=off, gs_tile_off=gs_tile.cpu().numpy(), gs_status=gs_st.cpu().numpy(), gs_dropped=gs_dr.cpu().numpy(),
                gs_xyz=gs_xyz.cpu().numpy()[:k], gs_idx=None if gs_idx is None else gs_idx.cpu().numpy()[:k])


def point_owner(hit_xyz, hit_idx, hit_off, mask_off, score, max_pts_per_frame, rule="score", min_keep=5, idx_cap=None):
    """One owner per contested point on arrays (cm3d_point_owner; pointowner.point_owner_host states it).  hit_xyz (n, 3 or 4) float32,
    hit_idx (n,), hit_off (M + 1,), mask_off (F + 1,), score (M,); rule "score" / "smallest" (or 0 / 1).  idx_cap: the capacity the
    call is told (default: the number of positions).  Returns a dict of numpy arrays: ow_owner (the clamped end of the last list,),
    ow_off, ow_tile_off, ow_status, ow_lost, ow_xyz (ow_off[-1], 4), ow_idx.  The defaults are untuned."""
    from .pointowner import rule_code
    L = _lib.lib()
    p = np.asarray(hit_xyz, np.float32)
    p = p.reshape(-1, p.shape[-1] if p.ndim > 1 else 4)
    tot = p.shape[0]
    cap = max(tot, 1) if idx_cap is None else int(idx_cap)
    P4 = np.zeros((max(tot, cap, 1), 4), np.float32)
    P4[:tot, :min(p.shape[1], 4)] = p[:, :4]
    hit_off = np.ascontiguousarray(hit_off, np.int32).reshape(-1)
    mask_off = np.ascontiguousarray(mask_off, np.int32).reshape(-1)
    M, F, P = hit_off.size - 1, mask_off.size - 1, int(max_pts_per_frame)
    idx = np.zeros(P4.shape[0], np.int32)
    idx[:tot] = np.asarray(hit_idx, np.int32)
    n = max(M, 1)
    d_xyz, d_idx, d_off, d_mo = _t(P4), _t(idx), _t(hit_off), _t(mask_off)
    d_sc = _t(np.asarray(score, np.float64).reshape(M) if M else np.zeros(1))
    ow_owner, ow_off, ow_tile, ow_st, ow_lost = _e(P4.shape[0]), _e(n + 1), _e(n + 1), _e(n), _e(n)
    ow_idx, ow_xyz = _e(P4.shape[0]), _e(P4.shape[0], 4, dtype=torch.float32)
    ws = _ws(L.cm3d_point_owner_workspace_bytes(F, P, M, cap))
    check(L.cm3d_point_owner(d_xyz.data_ptr(), d_idx.data_ptr(), d_off.data_ptr(), d_mo.data_ptr(), F, M, cap, P, d_sc.data_ptr(),
                             rule_code(rule), int(min_keep), ow_owner.data_ptr(), ow_off.data_ptr(), ow_tile.data_ptr(), ow_idx.data_ptr(),
                             ow_xyz.data_ptr(), ow_st.data_ptr(), ow_lost.data_ptr(), ws.data_ptr(), ws.numel(), _st()), "cm3d_point_owner")
    if M == 0:
        return dict(ow_owner=np.zeros(0, np.int32), ow_off=np.zeros(1, np.int32), ow_tile_off=np.zeros(1, np.int32),
                    ow_status=np.zeros(0, np.int32), ow_lost=np.zeros(0, np.int32), ow_xyz=np.zeros((0, 4), np.float32),
                    ow_idx=np.zeros(0, np.int32))
    off = ow_off.cpu().numpy()
    k, end = int(off[-1]), min(max(int(hit_off[-1]), 0), cap)
    return dict(ow_owner=ow_owner.cpu().numpy()[:end], ow_off=off, ow_tile_off=ow_tile.cpu().numpy(), ow_status=ow_st.cpu().numpy(),
                ow_lost=ow_lost.cpu().numpy(), ow_xyz=ow_xyz.cpu().numpy()[:k], ow_idx=ow_idx.cpu().numpy()[:k])


# ----------------------------------------------------------------------------- f4: SAM3D fusion matching
def match_records(boxes7):
    """(n,7) [center_x, center_y, bottom_z, length, width, height, heading] -> (n,6) float64 records of
    cm3d_bev_match.  The values pass through float32 like `tf.convert_to_tensor(boxes, dtype=float)`
    (linear_matching.py:248-249); cos/sin of the float32 heading are taken in float64 on the host."""
    b = np.asarray(boxes7, np.float64).reshape(-1, 7).astype(np.float32).astype(np.float64)
    return np.stack([b[:, 0], b[:, 1], b[:, 3], b[:, 4], np.cos(b[:, 6]), np.sin(b[:, 6])], axis=1)


def bev_match(pred_boxes, gt_boxes, iou=0.2):
    """`match(pred_boxes, sam3d_boxes, iou, Type.TYPE_2D)` (linear_matching.py:53-104) for a list of samples in one
    GPU call.  pred_boxes / gt_boxes: lists (one entry per sample) of (n,7) arrays.  Returns one
    (prediction_ids, groundtruth_ids, ious) triple per sample, matches in ascending prediction order."""
    return bev_match_records([match_records(b) for b in pred_boxes], [match_records(b) for b in gt_boxes], iou)


def bev_match_records(pr, gr, iou=0.2):
    """bev_match on float64 records as cm3d_bev_match takes them: lists (one entry per sample) of (n,6) arrays
    cx, cy, length, width, cos(heading), sin(heading), passed on unrounded."""
    L = _lib.lib()
    F = len(pr)
    if F == 0:
        return []
    if len(gr) != F:
        raise ValueError("bev_match: one gt entry per sample")
    pr = [np.asarray(r, np.float64).reshape(-1, 6) for r in pr]
    gr = [np.asarray(r, np.float64).reshape(-1, 6) for r in gr]
    np_, ng = np.array([r.shape[0] for r in pr], np.int64), np.array([r.shape[0] for r in gr], np.int64)
    if max(np_.max(), ng.max()) > _lib.MAX_MATCH_BOXES:
        raise _lib.Cm3dError(f"bev_match: more than {_lib.MAX_MATCH_BOXES} boxes in a sample")
    p_off = np.concatenate([[0], np.cumsum(np_)]).astype(np.int32)
    g_off = np.concatenate([[0], np.cumsum(ng)]).astype(np.int32)
    pair_off = np.concatenate([[0], np.cumsum(np_ * ng)]).astype(np.int64)
    n_pred, n_gt, total = int(p_off[-1]), int(g_off[-1]), int(pair_off[-1])
    d_p = _t(np.concatenate(pr).reshape(-1, 6) if n_pred else np.zeros((1, 6)), np.float64)
    d_g = _t(np.concatenate(gr).reshape(-1, 6) if n_gt else np.zeros((1, 6)), np.float64)
    d_po, d_go, d_pair = _t(p_off), _t(g_off), _t(pair_off)
    pm, gm = _e(max(n_pred, 1)), _e(max(n_gt, 1))
    miou = _e(max(n_pred, 1), dtype=torch.float64)
    status = torch.zeros(1, dtype=torch.int32, device=_dev())
    ws = _ws(L.cm3d_bev_match_workspace_bytes(total))
    check(L.cm3d_bev_match(d_p.data_ptr(), d_po.data_ptr(), n_pred, d_g.data_ptr(), d_go.data_ptr(), n_gt, d_pair.data_ptr(), F,
                           total, float(iou), pm.data_ptr(), gm.data_ptr(), miou.data_ptr(), status.data_ptr(), ws.data_ptr(),
                           ws.numel(), _st()), "cm3d_bev_match")
    pm, miou = pm.cpu().numpy()[:n_pred], miou.cpu().numpy()[:n_pred]
    if int(status.item()) != 0:
        raise _lib.Cm3dError("cm3d_bev_match: a sample exceeded the box capacity")
    out = []
    for f in range(F):
        m = pm[p_off[f]:p_off[f + 1]]
        ids = np.flatnonzero(m >= 0)
        out.append((ids.astype(np.int64), m[ids].astype(np.int64), miou[p_off[f]:p_off[f + 1]][ids]))
    return out


def waymo_metrics(packed, per_cutoff=False):
    """Counts of the Waymo detection metrics for a packed file pair (waymo_eval.pack) in ONE cm3d_waymo_metrics call.
    Returns (counts int64[16][101][4]: TP, FP, FN L1, FN L2; heading_sum int64[16][101] in 2^-32 units)."""
    L = _lib.lib()
    po, go = np.asarray(packed["pred_off"], np.int64), np.asarray(packed["gt_off"], np.int64)
    n_groups = int(po.size - 1)
    pair_off = np.concatenate([[0], np.cumsum(np.diff(po) * np.diff(go))]).astype(np.int64)
    total = int(pair_off[-1])
    counts = _e(_lib.WM_BREAKDOWNS, _lib.WM_CUTOFFS, 4, dtype=torch.int64)
    hsum = _e(_lib.WM_BREAKDOWNS, _lib.WM_CUTOFFS, dtype=torch.int64)
    status = torch.zeros(1, dtype=torch.int32, device=_dev())
    if n_groups == 0:
        return np.zeros((_lib.WM_BREAKDOWNS, _lib.WM_CUTOFFS, 4), np.int64), np.zeros((_lib.WM_BREAKDOWNS, _lib.WM_CUTOFFS), np.int64)

    def dev(a, dtype):
        a = np.ascontiguousarray(a, dtype)
        if a.shape[0] == 0:
            a = np.zeros((1,) + a.shape[1:], dtype)
        return _t(a)
    d_pb, d_ph, d_ps = dev(packed["pred_box"], np.float64), dev(packed["pred_head"], np.float32), dev(packed["pred_score"], np.float32)
    d_gb, d_gh, d_gl = dev(packed["gt_box"], np.float64), dev(packed["gt_head"], np.float32), dev(packed["gt_level"], np.int32)
    d_po, d_go = _t(po.astype(np.int32)), _t(go.astype(np.int32))
    d_bd, d_pair = _t(np.asarray(packed["group_bd"], np.int32)), _t(pair_off)
    ws = _ws(L.cm3d_waymo_metrics_workspace_bytes(total))
    check(L.cm3d_waymo_metrics(d_pb.data_ptr(), d_ph.data_ptr(), d_ps.data_ptr(), d_po.data_ptr(), d_gb.data_ptr(), d_gh.data_ptr(),
                               d_gl.data_ptr(), d_go.data_ptr(), d_bd.data_ptr(), d_pair.data_ptr(), n_groups, total, int(bool(per_cutoff)),
                               counts.data_ptr(), hsum.data_ptr(), status.data_ptr(), ws.data_ptr(), ws.numel(), _st()),
          "cm3d_waymo_metrics")
    st = int(status.item())
    if st:
        raise _lib.Cm3dError(f"cm3d_waymo_metrics: status {st} (bit0: more than {_lib.MAX_MATCH_BOXES} boxes of one type in a "
                             "frame, bit1: unknown breakdown)")
    return counts.cpu().numpy(), hsum.cpu().numpy()


SWEEP_ALPHA_CHUNK = 256      # alphas per cm3d_waymo_metrics_sweep call: bounds the output (64 KiB an alpha)


def waymo_metrics_sweep(packed_candidates, alphas, device_ms=None):
    """Counts of the Waymo detection metrics for every alpha of the SAM3D fusion grid search (waymo_eval.pack_candidates),
    SWEEP_ALPHA_CHUNK alphas per cm3d_waymo_metrics_sweep call.  Returns (counts int64[A][16][101][4], heading_sum
    int64[A][16][101]).  Raises Cm3dError (its `status` attribute holds the status word) when a group is over capacity.
    device_ms: a list that receives every call's device time in ms, measured with events (tools/waymo_sweep_rate.py)."""
    L = _lib.lib()
    pc = packed_candidates
    alphas = np.ascontiguousarray(alphas, np.float64).reshape(-1)
    A = int(alphas.size)
    co, go = np.asarray(pc["cand_off"], np.int64), np.asarray(pc["gt_off"], np.int64)
    n_groups = int(co.size - 1)
    out_c = np.zeros((A, _lib.WM_BREAKDOWNS, _lib.WM_CUTOFFS, 4), np.int64)
    out_h = np.zeros((A, _lib.WM_BREAKDOWNS, _lib.WM_CUTOFFS), np.int64)
    if n_groups == 0 or A == 0:
        return out_c, out_h
    pair_off = np.concatenate([[0], np.cumsum(np.diff(co) * np.diff(go))]).astype(np.int64)
    total = int(pair_off[-1])

    def dev(a, dtype):
        a = np.ascontiguousarray(a, dtype)
        if a.shape[0] == 0:
            a = np.zeros((1,) + a.shape[1:], dtype)
        return _t(a)
    d_cb, d_ch, d_ck = dev(pc["cand_box"], np.float64), dev(pc["cand_head"], np.float32), dev(pc["cand_kind"], np.int32)
    d_cp, d_cs = dev(pc["cand_p"], np.float64), dev(pc["cand_s"], np.float64)
    d_gb, d_gh, d_gl = dev(pc["gt_box"], np.float64), dev(pc["gt_head"], np.float32), dev(pc["gt_level"], np.int32)
    d_co, d_go = _t(co.astype(np.int32)), _t(go.astype(np.int32))
    d_bd, d_pair, d_static = _t(np.asarray(pc["group_bd"], np.int32)), _t(pair_off), _t(np.asarray(pc["group_static"], np.int32))
    ws = _ws(L.cm3d_waymo_metrics_sweep_workspace_bytes(total))
    status = torch.zeros(1, dtype=torch.int32, device=_dev())
    for lo in range(0, A, SWEEP_ALPHA_CHUNK):
        n = min(SWEEP_ALPHA_CHUNK, A - lo)
        d_al = _t(alphas[lo:lo + n])
        counts = _e(n, _lib.WM_BREAKDOWNS, _lib.WM_CUTOFFS, 4, dtype=torch.int64)
        hsum = _e(n, _lib.WM_BREAKDOWNS, _lib.WM_CUTOFFS, dtype=torch.int64)
        if device_ms is not None:
            ev = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            ev[0].record()
        check(L.cm3d_waymo_metrics_sweep(d_cb.data_ptr(), d_ch.data_ptr(), d_ck.data_ptr(), d_cp.data_ptr(), d_cs.data_ptr(),
                                         d_co.data_ptr(), d_gb.data_ptr(), d_gh.data_ptr(), d_gl.data_ptr(), d_go.data_ptr(),
                                         d_bd.data_ptr(), d_pair.data_ptr(), d_static.data_ptr(), n_groups, total, d_al.data_ptr(), n,
                                         counts.data_ptr(), hsum.data_ptr(), status.data_ptr(), ws.data_ptr(), ws.numel(), _st()),
              "cm3d_waymo_metrics_sweep")
        if device_ms is not None:
            ev[1].record()
            ev[1].synchronize()
            device_ms.append(ev[0].elapsed_time(ev[1]))
        st = int(status.item())
        if st:
            err = _lib.Cm3dError(f"cm3d_waymo_metrics_sweep: status {st} (bit0: more than {_lib.MAX_MATCH_BOXES} candidates or ground-truth "
                                 "boxes of one type in a frame, bit1: unknown breakdown)")
            err.status = st
            raise err
        out_c[lo:lo + n], out_h[lo:lo + n] = counts.cpu().numpy(), hsum.cpu().numpy()
    return out_c, out_h


NUSC_ALPHA_CHUNK = 256       # alphas per cm3d_nusc_match call: bounds the output (one byte per candidate and alpha, 4 T more with indices)


def nusc_match(packed, alphas, want_idx=False, device_ms=None):
    """The nuScenes greedy matching of every group of `packed` (nusc_eval.pack) at every alpha, NUSC_ALPHA_CHUNK alphas per
    cm3d_nusc_match call.  Returns (tp_bits uint8[A][C]: bit t = TP at dist_th[t], bit 7 = active; match_idx int32[A][C][T] with
    the group-local ground-truth index or -1 when want_idx, else None).  Raises Cm3dError (its `status` attribute holds the
    status word) when a group is over capacity.  device_ms: a list that receives every call's device time in ms (events)."""
    L = _lib.lib()
    alphas = np.ascontiguousarray(alphas, np.float64).reshape(-1)
    A = int(alphas.size)
    co, go = np.asarray(packed["cand_off"], np.int64), np.asarray(packed["gt_off"], np.int64)
    th = np.ascontiguousarray(packed["dist_th"], np.float64).reshape(-1)
    n_groups, C, T = int(co.size - 1), int(co[-1]), int(th.size)
    tp_bits = np.zeros((A, C), np.uint8)
    match_idx = np.full((A, C, T), -1, np.int32) if want_idx else None
    if n_groups == 0 or C == 0 or A == 0:
        return tp_bits, match_idx
    if C >= 2 ** 31 or int(go[-1]) >= 2 ** 31:
        raise _lib.Cm3dError("cm3d_nusc_match: offsets are 32-bit")

    def dev(a, dtype):
        a = np.ascontiguousarray(a, dtype)
        if a.shape[0] == 0:
            a = np.zeros((1,) + a.shape[1:], dtype)
        return _t(a)
    d_xy, d_kind = dev(packed["cand_xy"], np.float64), dev(packed["cand_kind"], np.int32)
    d_p, d_s, d_gxy = dev(packed["cand_p"], np.float64), dev(packed["cand_s"], np.float64), dev(packed["gt_xy"], np.float64)
    d_co, d_go, d_th = _t(co.astype(np.int32)), _t(go.astype(np.int32)), _t(th)
    status = torch.zeros(1, dtype=torch.int32, device=_dev())
    for lo in range(0, A, NUSC_ALPHA_CHUNK):
        n = min(NUSC_ALPHA_CHUNK, A - lo)
        d_al = _t(alphas[lo:lo + n])
        bits = _e(n, C, dtype=torch.uint8)
        idx = _e(n, C, T) if want_idx else None
        ws = _ws(L.cm3d_nusc_match_workspace_bytes(n_groups, C, n))
        if device_ms is not None:
            ev = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            ev[0].record()
        check(L.cm3d_nusc_match(d_xy.data_ptr(), d_kind.data_ptr(), d_p.data_ptr(), d_s.data_ptr(), d_co.data_ptr(), d_gxy.data_ptr(),
                                d_go.data_ptr(), n_groups, C, d_al.data_ptr(), n, d_th.data_ptr(), T, bits.data_ptr(),
                                idx.data_ptr() if want_idx else 0, status.data_ptr(), ws.data_ptr(), ws.numel(), _st()), "cm3d_nusc_match")
        if device_ms is not None:
            ev[1].record()
            ev[1].synchronize()
            device_ms.append(ev[0].elapsed_time(ev[1]))
        st = int(status.item())
        if st:
            err = _lib.Cm3dError(f"cm3d_nusc_match: status {st} (bit0: a group with more than {_lib.NUSC_MAX_CAND} candidates or more than "
                                 f"{_lib.NUSC_MAX_GT} ground-truth boxes)")
            err.status = st
            raise err
        tp_bits[lo:lo + n] = bits.cpu().numpy()
        if want_idx:
            match_idx[lo:lo + n] = idx.cpu().numpy()
    return tp_bits, match_idx
