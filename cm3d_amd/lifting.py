"""Host-side driver of the lifting path: packs frames into a lift batch, keeps
the device buffers (PyTorch-ROCm tensors are used for device memory and streams
only) and calls the HIP kernels through the C-ABI of include/cm3d_hip.h.

Mirrors the stages of the reference's src/nuscenes/2d_to_3d.py main loop
(:415-694 stage 1, :699-827 stage 2, :844-924 NMS) for a whole batch of frames
at once; names follow the reference (`get_detection_name`, `ATTRIBUTE_NAMES`,
`threshs_by_label`, ...).
"""
from contextlib import contextmanager
from dataclasses import dataclass, field
from typing import List, Optional, Sequence

import ctypes
import os
import zlib

import numpy as np
import torch

from . import _lib
from . import drivable
from . import rle as rlemod
from ._lib import Cm3dError, check
from .drivable import Stage2Filters  # noqa: F401  (LiftEngine(filters=Stage2Filters(...)))
from .cluster import DepthCluster  # noqa: F401  (LiftEngine(cluster=DepthCluster(...)))
from .bevfit import YawFit, angle_table  # noqa: F401  (LiftEngine(yaw=YawFit(...)))
from .boxplace import BoxPlace  # noqa: F401  (LiftEngine(yaw=YawFit(...), place=BoxPlace(...)))
from .nms import RotatedNms  # noqa: F401  (LiftEngine(nms=RotatedNms(...)))
from .velocity import Velocity, link_table  # noqa: F401  (LiftEngine(velocity=Velocity(...)))
from .tracks import Tracks  # noqa: F401  (LiftEngine(velocity=Velocity(...), tracks=Tracks(...)))
from .boxsize import BoxSize  # noqa: F401  (LiftEngine(yaw=..., place=..., velocity=..., size=BoxSize(...)))
from .boxvertical import BoxVertical, RESULTS as VERTICAL_RESULTS  # noqa: F401  (LiftEngine(vertical=BoxVertical(...)))
from .virtualpoints import VirtualPoints, RESULTS as VIRTUAL_RESULTS  # noqa: F401  (LiftEngine(virtual=VirtualPoints(...)))
from .boxground import BoxGround, RESULTS as GROUND_RESULTS  # noqa: F401  (LiftEngine(ground=BoxGround(...)))
from .groundstrip import GroundStrip, N_CELLS as GRID_CELLS  # noqa: F401  (LiftEngine(strip=GroundStrip(...)))
from .pointowner import PointOwner  # noqa: F401  (LiftEngine(owner=PointOwner(...)))

# ---- tables of the reference --------------------------------------------------
CAM_LIST = ["CAM_FRONT", "CAM_FRONT_RIGHT", "CAM_BACK_RIGHT", "CAM_BACK", "CAM_BACK_LEFT", "CAM_FRONT_LEFT"]  # :62-69
ATTRIBUTE_NAMES = {  # :70-81
    "barrier": "", "traffic_cone": "", "bicycle": "cycle.without_rider", "motorcycle": "cycle.without_rider",
    "pedestrian": "pedestrian.standing", "car": "vehicle.stopped", "bus": "vehicle.stopped",
    "construction_vehicle": "vehicle.stopped", "trailer": "vehicle.stopped", "truck": "vehicle.stopped",
}
SHAPE_PRIORS_CHATGPT = {  # cfg/shape_priors_chatgpt.json:1-12, [w, l, h]
    "car": [1.8, 4.5, 1.4], "truck": [2.6, 8.0, 3.6], "bus": [2.5, 12.0, 4.0], "trailer": [2.6, 12.0, 3.6],
    "construction_vehicle": [2.0, 4.5, 2.5], "pedestrian": [0.4, 0.7, 1.7], "motorcycle": [0.8, 2.1, 1.7],
    "bicycle": [0.6, 1.8, 1.4], "traffic_cone": [0.3, 0.3, 0.7], "barrier": [0.5, 1.2, 0.9],
}
THRESHS_BY_LABEL = {  # :850-861 (squared metres)
    "barrier": 1, "traffic_cone": 0.175, "bicycle": 0.85, "motorcycle": 0.85, "pedestrian": 0.175, "car": 4,
    "bus": 10, "construction_vehicle": 12, "trailer": 10, "truck": 12,
}
PUSHED_CLASSES = ["car", "truck", "bus", "construction_vehicle", "trailer", "barrier"]  # :763
MIN_DIST = 2.3            # :348
N_SWEEPS = 3              # :437
# the opt-in stages of a pass that have an event pair, in the order LiftEngine.run appends their events (`b.timed`)
TIMED_ORDER = ("filter", "owner", "strip", "cluster", "yaw", "place")


def get_detection_name(name):
    """reference :122-132"""
    return {"trafficcone": "traffic_cone", "constructionvehicle": "construction_vehicle", "human": "pedestrian"}.get(name, name)


def get_shape_prior(shape_priors, name, chatgpt=True):
    """reference :134-161 (only the chatgpt table is ever loaded, :384-385)"""
    if not chatgpt:
        raise NotImplementedError("the reference only ships the chatgpt priors on this path")
    return shape_priors[name]


@dataclass
class ClassTable:
    names: List[str]
    prior_wlh: np.ndarray      # (n,3) float64
    is_vehicle: np.ndarray     # (n,) int32
    nms_thr: np.ndarray        # (g,) float64, squared-distance threshold per NMS label
    nms_group: Optional[np.ndarray] = None   # (n,) int32 NMS label of each class (default: the class itself)
    out_names: Optional[List[str]] = None    # what the writer calls each class (Waymo: the Waymo type)
    needs_road: Optional[np.ndarray] = None  # (n,) int32 classes the opt-in drivable filter tests (default: car, truck, bus; :775)

    def __post_init__(self):
        if self.nms_group is None:
            self.nms_group = np.arange(len(self.names), dtype=np.int32)
        if self.needs_road is None:
            self.needs_road = drivable.needs_road(self.names)

    @staticmethod
    def nuscenes(shape_priors=None):
        pri = shape_priors or SHAPE_PRIORS_CHATGPT
        names = list(pri.keys())
        return ClassTable(names=names,
                          prior_wlh=np.array([pri[n] for n in names], np.float64),
                          is_vehicle=np.array([n in PUSHED_CLASSES for n in names], np.int32),
                          nms_thr=np.array([THRESHS_BY_LABEL[n] for n in names], np.float64))

    @staticmethod
    def waymo(shape_priors=None):
        """Reference src/waymo: same priors and pushed classes, classes renamed through NUSC_TO_WAYMO
        (cfg/prompt_cfg.py:286-297), NMS per Waymo type with the thresholds of 2d_to_3d.py:1147-1158."""
        from . import waymo as wm
        base = ClassTable.nuscenes(shape_priors)
        types = [wm.WAYMO_TYPE.get(wm.NUSC_TO_WAYMO[n], -1) for n in base.names]
        thr = np.zeros(5, np.float64)
        for t, v in wm.THRESHS_BY_TYPE.items():
            thr[t] = v
        return ClassTable(names=base.names, prior_wlh=base.prior_wlh, is_vehicle=base.is_vehicle, nms_thr=thr,
                          nms_group=np.array([max(t, 0) for t in types], np.int32),
                          out_names=[wm.NUSC_TO_WAYMO[n] for n in base.names])

    def index(self, detection_name):
        return self.names.index(detection_name)   # ValueError for an unknown class, like the reference's KeyError


# ---- batch packing ------------------------------------------------------------
@dataclass
class HostBatch:
    """numpy view of one lift batch (see include/cm3d_hip.h for the layout).  Built by assemble_batch and nowhere else."""
    raw: Optional[np.ndarray]                 # None while the sweeps wait in shared memory (raw_shm) and once they have been uploaded
    raw_stride: int
    sweep_row_off: np.ndarray
    sweep_xf: np.ndarray
    frame_sweep_off: np.ndarray
    max_rows_per_sweep: int
    cams: np.ndarray
    n_cams: int
    mask_off: np.ndarray
    mask_cam: np.ndarray
    mask_frame: np.ndarray
    rle_counts: np.ndarray
    rle_off: np.ndarray
    class_id: np.ndarray
    score: np.ndarray
    lane: np.ndarray
    lane_off: np.ndarray
    frame_lane: np.ndarray
    ego_xyz: np.ndarray
    width: int
    height: int
    tokens: Optional[List[str]] = None        # None on the route through reader.Manifest: its frames are rows of sample.json, not tokens
    labels: Optional[List[List[str]]] = None  # None on that route too: the labels arrive as class ids
    intensity: Optional[np.ndarray] = None    # quad layout only: (rows,) float32, the rows' fourth column (None: not uploaded)
    frame_rows: Optional[np.ndarray] = None   # quad layout only: (F,) rows of each frame without its padding rows
    pose_rt: Optional[np.ndarray] = None      # (F,12) float32, Waymo: vehicle -> global rotate/translate
    pose_inv: Optional[np.ndarray] = None     # (F,16) float32, Waymo: inverse of the float32 frame pose
    ego_box: bool = True                      # nuScenes drops the ego-box points (:442-445); Waymo does not
    mask_wh: Optional[np.ndarray] = None      # (n_masks, 2) int32 own (w, h) of every mask when they differ (Waymo's side cameras,
                                              # src/waymo/2d_to_3d.py:520-521); None: every mask has the canvas size (width, height)
    lane_key: Optional[tuple] = None          # which lane tables these are, from a caller that knows (pipeline_nuscenes: the map locations)
    raw_shm: Optional[tuple] = None           # (segment name, shape): the sweeps a reader process left in shared memory instead of `raw`
    polygons: Optional[list] = None           # drivable-area polygon tables, one per lane table (eval_detection.load_drivable_polygons); only
                                              # an engine with Stage2Filters(drivable=True) reads them
    polygon_key: Optional[tuple] = None       # which polygon tables these are, from a caller that knows (else a checksum: polygon_tables_key)
    frame_next: Optional[np.ndarray] = None   # (F,) int32 batch index of the same scene's following keyframe, -1 for none; with
    frame_time: Optional[np.ndarray] = None   # (F,) float64 seconds since the batch's first frame (velocity.frame_times): only an engine
                                              # with Velocity(...) reads them; None: that option cannot be enabled for this batch
    frame_seed: Optional[np.ndarray] = None   # (F,) uint32, one word per frame for the sampling of an engine with VirtualPoints(...): the
                                              # entry points set the frame's ordinal in the whole job; None: arange(F)
    _lane_crc: Optional[tuple] = field(default=None, init=False, repr=False, compare=False)

    def lane_tables_key(self):
        """What LiftEngine keys its cache of lane tables and their spatial index by: lane_key, else a checksum of the tables (kept)."""
        if self.lane_key is not None:
            return self.lane_key
        if self._lane_crc is None:
            self._lane_crc = (self.lane.shape, self.lane_off.tobytes(), zlib.crc32(np.ascontiguousarray(self.lane).view(np.uint8)))
        return self._lane_crc

    def polygon_tables_key(self):
        """What LiftEngine keys its cache of polygon indices by."""
        if self.polygon_key is None:
            self.polygon_key = drivable.tables_key(self.polygons)
        return ("polygons",) + tuple(self.polygon_key)

    @property
    def n_frames(self):
        return len(self.mask_off) - 1

    @property
    def n_masks(self):
        return int(self.mask_off[-1])

    @property
    def n_raw_rows(self):
        return int(self.sweep_row_off[-1])

    @property
    def quads(self):
        return self.raw_stride == _lib.RAW_QUADS

    @property
    def n_real_rows(self):
        """Rows the files held (the quad layout's padding rows left out)."""
        return self.n_raw_rows if self.frame_rows is None else int(np.sum(self.frame_rows))

    @property
    def bytes_per_row(self):
        """Bytes of a raw row that cross HBM in the projection launch."""
        return 12 if self.quads else 4 * self.raw_stride


def rows_to_quads(raw, sweep_row_off, frame_sweep_off, keep_intensity=True):
    """Row-major sweeps (rows, >= 4 columns) -> the quad layout of include/cm3d_hip.h (cm3d_sweep_prep): every frame padded to a
    multiple of 4 rows with NaN rows that belong to its last sweep, rows 4q..4q+3 stored as x0..3 y0..3 z0..3.
    Returns (quads (R/4, 3, 4) float32, intensity (R,) float32 or None, sweep_row_off' (S+1,), frame_rows (F,)).
    What the native reader does while it fills the page-locked batch (cm3d_amd.reader); this is the numpy form for
    batches packed from arrays."""
    raw = np.asarray(raw, np.float32)
    sro = np.asarray(sweep_row_off, np.int64)
    fso = np.asarray(frame_sweep_off, np.int64)
    F = len(fso) - 1
    frame_rows = (sro[fso[1:]] - sro[fso[:-1]]).astype(np.int32)
    padded = (frame_rows.astype(np.int64) + 3) // 4 * 4
    new_start = np.concatenate([[0], np.cumsum(padded)])
    R = int(new_start[-1])
    xyz = np.full((R, 3), np.nan, np.float32)
    inten = np.zeros(R, np.float32) if keep_intensity else None
    new_sro = np.zeros(len(sro), np.int64)
    for f in range(F):
        a, b = int(sro[fso[f]]), int(sro[fso[f + 1]])
        d = int(new_start[f]) - a
        xyz[a + d:b + d] = raw[a:b, :3]
        if keep_intensity:
            inten[a + d:b + d] = raw[a:b, 3]
        new_sro[fso[f]:fso[f + 1]] = sro[fso[f]:fso[f + 1]] + d
    new_sro[fso[-1]:] = R                      # the end of the last sweep = the padded end of the batch
    # sweeps of a frame stay back to back; a frame's padding rows sit behind its last sweep, in front of the next frame's first
    quads = np.ascontiguousarray(xyz.reshape(R // 4, 4, 3).transpose(0, 2, 1))
    return quads, inten, new_sro.astype(np.int32), frame_rows


def default_layout():
    """Layout of the raw rows in a packed batch: "quads" (12 bytes per row cross HBM; include/cm3d_hip.h) unless
    CM3D_RAW_LAYOUT=rows asks for the files' own rows."""
    return os.environ.get("CM3D_RAW_LAYOUT", "quads")


class BatchDeclined(Exception):
    """The native reader does not take this batch -- a pickle its parser does not know, masks of different image sizes, (Manifest route
    only) frames without masks to be dropped --; the caller hands the batch to the Python reader.  Nothing else means "fall back"."""


@contextmanager
def declining_unknown_formats():
    """The one place where a file the native parser does not know (reader.ReaderError with ERR_FORMAT) becomes BatchDeclined."""
    from .reader import ERR_FORMAT, ReaderError
    try:
        yield
    except ReaderError as exc:
        if exc.code != ERR_FORMAT:
            raise
        raise BatchDeclined(str(exc)) from exc


def _as(a, dtype):
    """`a` itself when it already is an array of that type (a page-locked staging buffer stays the object it is)."""
    return a if isinstance(a, np.ndarray) and a.dtype == dtype else np.asarray(a, dtype)


def assemble_batch(*, raw, raw_stride, sweep_row_off, sweep_xf, frame_sweep_off, cams, mask_off, mask_cam, rle_counts, rle_off, class_id, score,
                   detections_per_frame, lane_tables, frame_lane, ego_xyz, width, height, mask_wh=None, **optional) -> HostBatch:
    """The primary arrays of a batch -> HostBatch: the one place that coerces types, derives what can be derived (n_cams,
    max_rows_per_sweep, mask_frame, lane, lane_off, whether mask_wh says anything) and checks the fields against each other.
    cams: one (n_cams, 64) record array per frame, or all of them stacked.  detections_per_frame: for every list that names a frame's
    detections beside the masks themselves (labels, scores, cam_nums), its length per frame.  optional: the remaining HostBatch fields."""
    i32 = lambda a: _as(a, np.int32)
    if not isinstance(cams, np.ndarray):
        if len({np.shape(c)[0] for c in cams}) > 1:
            raise ValueError("all frames of a batch must share the camera count")
        cams = np.stack([np.asarray(c, np.float32) for c in cams])
    mask_off, mask_cam, class_id, score = i32(mask_off), i32(mask_cam), i32(class_id), _as(score, np.float64)
    n_per = np.diff(mask_off)
    if not (all(np.array_equal(n, n_per) for n in detections_per_frame) and mask_cam.size == class_id.size == score.size == int(mask_off[-1])):
        raise ValueError("labels / detection_scores / cam_nums / masks differ in length")
    sweep_row_off = i32(sweep_row_off)
    if mask_wh is not None:
        mask_wh = i32(mask_wh).reshape(-1, 2)
        if bool(np.all(mask_wh == np.array([width, height], np.int32))):
            mask_wh = None
    # torch.Tensor(...) at :278: through float64 to float32; a table that already is float32 is taken as it is (the identity)
    lane32 = [(t if isinstance(t, np.ndarray) and t.dtype == np.float32 else np.asarray(t, np.float64).astype(np.float32)).reshape(-1, 3)
              for t in lane_tables]
    return HostBatch(
        raw=raw, raw_stride=raw_stride, sweep_row_off=sweep_row_off, sweep_xf=sweep_xf, frame_sweep_off=i32(frame_sweep_off),
        max_rows_per_sweep=max(1, int(np.diff(sweep_row_off).max())) if len(sweep_row_off) > 1 else 1, cams=cams, n_cams=cams.shape[1],
        mask_off=mask_off, mask_cam=mask_cam, mask_frame=np.repeat(np.arange(len(n_per), dtype=np.int32), n_per),
        rle_counts=_as(rle_counts, np.uint32), rle_off=i32(rle_off), class_id=class_id, score=score,
        lane=np.concatenate(lane32, 0), lane_off=np.concatenate([[0], np.cumsum([t.shape[0] for t in lane32])]).astype(np.int32),
        frame_lane=i32(frame_lane), ego_xyz=_as(ego_xyz, np.float64), width=width, height=height, mask_wh=mask_wh, **optional)


def frame_detections(frames, classes: ClassTable):
    """labels, scores and cam_nums of frames (or frame manifests) -> what assemble_batch takes of them: (class_id, score, mask_cam,
    labels per frame, detections_per_frame)."""
    class_id, score, mask_cam = [], [], []
    for fr in frames:
        for l in fr.labels:
            ci = classes.index(get_detection_name(l))
            if classes.out_names is not None and classes.out_names[ci] == "":
                raise ValueError(f"label {l!r} has no output type")     # the reference raises ValueError (src/waymo/2d_to_3d.py:1054-1062)
            class_id.append(ci)
        score.extend(float(s) for s in fr.scores)
        mask_cam.extend(int(c) for c in fr.cam_nums)
    per_frame = [[len(getattr(fr, k)) for fr in frames] for k in ("labels", "scores", "cam_nums")]
    return class_id, score, mask_cam, [list(fr.labels) for fr in frames], per_frame


def frame_links(frames):
    """(frame_next, frame_time) of frames that carry the sample table's `timestamp` (integer microseconds) and `next_token`
    (nusc_io.scene_manifest, frames_of_scene): the batch index of every frame's follower -- -1 when it is not in the batch -- and the
    seconds since the batch's first frame (velocity.frame_next_of, frame_times).  (None, None) for frames without them."""
    from .velocity import frame_next_of, frame_times
    stamps = [getattr(f, "timestamp", None) for f in frames]
    if not stamps or any(t is None for t in stamps):
        return None, None
    return frame_next_of([f.token for f in frames], [getattr(f, "next_token", "") or "" for f in frames]), frame_times(stamps)


def pack_frames(frames: Sequence, lane_tables: Sequence[np.ndarray], frame_lane: Sequence[int],
                classes: Optional[ClassTable] = None, layout: Optional[str] = None, keep_intensity: bool = True,
                frame_next=None, frame_time=None) -> HostBatch:
    """frames: objects with the attributes of cm3d_amd.synthetic.Frame.  layout: "rows" (the sweeps as they are) or
    "quads" (rows_to_quads); None = default_layout().  frame_next, frame_time: HostBatch's fields of those names (the velocity stage);
    None: frame_links(frames).
    The masks of a batch may have different image sizes (Waymo's front and side cameras inside one frame, KITTI's frames among each
    other): the batch's `width`, `height` are the CANVAS -- the elementwise maximum over the frames' and the masks' sizes --, every run
    list stays as the producer wrote it, and `mask_wh` lists the masks' own sizes (None when they all have the canvas size)."""
    classes = classes or ClassTable.nuscenes()
    layout = layout or default_layout()
    if layout not in ("rows", "quads"):
        raise ValueError(layout)
    if frame_next is None and frame_time is None:
        frame_next, frame_time = frame_links(frames)
    W = max([int(fr.width) for fr in frames] + [int(rl["size"][0]) for fr in frames for rl in fr.rles])
    H = max([int(fr.height) for fr in frames] + [int(rl["size"][1]) for fr in frames for rl in fr.rles])
    if W > 4096:
        raise ValueError(f"masks of {W} columns: the mask kernels hold rows of up to 4096 pixels")
    raws, xfs, row_off, fso = [], [], [0], [0]
    mask_wh, mask_off, cnts, rle_off = [], [0], [], [0]
    pose_rt, pose_inv = [], []
    stride = frames[0].sweeps_raw[0].shape[1]
    for fr in frames:
        for r in fr.sweeps_raw:
            r = np.ascontiguousarray(r, np.float32)
            if r.shape[1] != stride:
                raise ValueError("mixed sweep strides")
            raws.append(r)
            row_off.append(row_off[-1] + r.shape[0])
        xfs.append(np.asarray(fr.sweep_xf, np.float32).reshape(-1, _lib.SWEEP_XF_STRIDE))
        fso.append(fso[-1] + len(fr.sweeps_raw))
        for rl in fr.rles:
            w, h = (int(v) for v in rl["size"])
            if w < 1 or h < 1:
                raise ValueError(f"mask size {rl['size']}")
            c = rlemod.string_to_counts(rl["counts"]) if isinstance(rl["counts"], (bytes, bytearray)) else np.asarray(rl["counts"], np.uint32)
            if int(c.astype(np.int64).sum()) != w * h:
                raise ValueError("RLE run lengths do not cover the mask")
            mask_wh.append((w, h))
            cnts.append(c)
            rle_off.append(rle_off[-1] + c.size)
        mask_off.append(mask_off[-1] + len(fr.rles))
        if getattr(fr, "pose", None) is not None:
            from . import waymo as wm
            rt, inv = wm.pose_records(fr.pose)
            pose_rt.append(rt)
            pose_inv.append(inv)
    class_id, score, mask_cam, labels, per_frame = frame_detections(frames, classes)
    raw = np.concatenate(raws, 0) if raws else np.zeros((0, stride), np.float32)
    intensity = frame_rows = None
    if layout == "quads":
        raw, intensity, row_off, frame_rows = rows_to_quads(raw, np.asarray(row_off, np.int32), fso, keep_intensity)
        stride = _lib.RAW_QUADS
    posed = len(pose_rt) == len(frames) and len(frames) > 0
    return assemble_batch(
        raw=raw, raw_stride=stride, intensity=intensity, frame_rows=frame_rows, sweep_row_off=row_off, sweep_xf=np.concatenate(xfs, 0),
        frame_sweep_off=fso, cams=[fr.cams for fr in frames], mask_off=mask_off, mask_cam=mask_cam, mask_wh=mask_wh,
        rle_counts=np.concatenate(cnts).astype(np.uint32) if cnts else np.zeros(0, np.uint32), rle_off=rle_off,
        class_id=class_id, score=score, detections_per_frame=per_frame, lane_tables=lane_tables, frame_lane=frame_lane,
        ego_xyz=[np.asarray(fr.ego_xyz, np.float64) for fr in frames], width=W, height=H, tokens=[fr.token for fr in frames], labels=labels,
        pose_rt=np.stack(pose_rt).astype(np.float32) if posed else None, pose_inv=np.stack(pose_inv).astype(np.float32) if posed else None,
        ego_box=not (posed or all(getattr(f, "no_ego_box", False) for f in frames)),
        frame_next=None if frame_next is None else np.asarray(frame_next, np.int32),
        frame_time=None if frame_time is None else np.asarray(frame_time, np.float64))


def require_one_mask_size(hb: HostBatch):
    """The dense-mask route (decode_masks_dense, cm3d_erode_pack, `--masks dense`) takes one image size per batch."""
    if hb.mask_wh is not None:
        raise ValueError(f"masks of different image sizes in one batch (canvas {hb.width}x{hb.height}): the dense-mask route takes one size "
                         "per batch; use masks=\"rle\"")


def pack_manifest(man, lane_tables, frame_lane, classes: Optional[ClassTable], rd, stride=5, alloc=None):
    """Frame manifests (nusc_io.scene_manifest) -> HostBatch, with the bulk data read by the native loader `rd`
    (cm3d_amd.reader.Reader): all sweeps of the batch land in one (page-locked) `raw` buffer, all RLE strings are parsed
    to run lengths by its thread pool.  Frames without masks are left out, like pack_frames' callers do.
    Returns (HostBatch or None when no frame has a mask, indices of the frames it holds); BatchDeclined for a batch that
    needs the Python reader."""
    classes = classes or ClassTable.nuscenes()
    with declining_unknown_formats():
        counts, rle_off, fmo, wh = rd.load_masks([m.mask_path for m in man])
        n_per = np.diff(fmo)
        live = [i for i in range(len(man)) if n_per[i] > 0]
        if not live:
            return None, []
        if len(live) != len(man):                       # rare: repack the frames that have masks
            hb, sub = pack_manifest([man[i] for i in live], lane_tables, [frame_lane[i] for i in live], classes, rd, stride, alloc)
            return hb, [live[k] for k in sub]
        if np.any(wh != wh[0]):
            raise BatchDeclined("masks of different image sizes in one batch")
        fso = np.concatenate([[0], np.cumsum([len(m.sweep_paths) for m in man])]).astype(np.int32)
        intensity = frame_rows = None
        if default_layout() == "quads":     # the files' rows go straight into the quad layout (no intensity plane: no output holds it)
            raw, intensity, row_off, frame_rows = rd.load_sweeps_quads([p for m in man for p in m.sweep_paths], fso, stride, False, alloc)
            stride = _lib.RAW_QUADS
        else:
            raw, row_off = rd.load_sweeps([p for m in man for p in m.sweep_paths], stride, alloc)
    class_id, score, mask_cam, labels, per_frame = frame_detections(man, classes)
    frame_next, frame_time = frame_links(man)
    hb = assemble_batch(
        raw=raw, raw_stride=stride, intensity=intensity, frame_rows=frame_rows, sweep_row_off=row_off,
        sweep_xf=np.concatenate([np.asarray(m.sweep_xf, np.float32).reshape(-1, _lib.SWEEP_XF_STRIDE) for m in man], 0),
        frame_sweep_off=fso, cams=[m.cams for m in man], mask_off=fmo, mask_cam=mask_cam, mask_wh=wh, rle_counts=counts, rle_off=rle_off,
        class_id=class_id, score=score, detections_per_frame=per_frame, lane_tables=lane_tables, frame_lane=frame_lane,
        ego_xyz=[m.ego_xyz for m in man], width=int(wh[0, 0]), height=int(wh[0, 1]), tokens=[m.token for m in man], labels=labels,
        frame_next=frame_next, frame_time=frame_time)
    return hb, list(range(len(man)))


# ---- device side ----------------------------------------------------------------
def _ptr(t: Optional[torch.Tensor]):
    return 0 if t is None else t.data_ptr()


_MFMA_VERIFIED = {}


def _verify_matrix_pipe(lib, dev):
    """Once per process and device: the medoid's first pass over long lists runs on the matrix pipe, and the error bound of
    its second pass holds only while v_mfma_f32_32x32x2_f32 reproduces the reference's k-ordered fmaf chain bit for bit
    (csrc/medoid.hip).  cm3d_selftest_mfma checks exactly that on this device (2048 waves x 24 tiles, coordinates from
    vehicle-frame to 20x nuScenes' global magnitudes, ~0.1 ms); a device that fails it must not produce labels."""
    key = str(dev)
    if key in _MFMA_VERIFIED:
        return
    with torch.cuda.device(dev):
        bad = torch.zeros(1, dtype=torch.int64, device=dev)
        check(lib.cm3d_selftest_mfma(20240607, 24, bad.data_ptr(), torch.cuda.current_stream(dev).cuda_stream), "cm3d_selftest_mfma")
        n_bad = int(bad.item())
    if n_bad:
        raise Cm3dError(f"matrix-pipe self-test failed on {key}: {n_bad} of {2048 * 24 * 1024} squared distances differ from the "
                        "vector fma chain or an output clamp is not honoured; rebuild with -DMD_APPROX_MFMA=0 -DMD_SCALED_ROUTES=0")
    _MFMA_VERIFIED[key] = True


class LiftEngine:
    """Owns the device buffers of one lift batch and launches the kernels.
    All launches go to torch's current HIP stream and never synchronise."""

    def __init__(self, device="cuda:0", classes: Optional[ClassTable] = None, min_dist=MIN_DIST,
                 hits_per_point=4.0, keep_colsum=False, keep_cloud=None, lane_cache=None, obb=False, filters: Optional[Stage2Filters] = None,
                 cluster: Optional[DepthCluster] = None, nms: Optional[RotatedNms] = None, yaw: Optional[YawFit] = None,
                 velocity: Optional[Velocity] = None, tracks: Optional[Tracks] = None, place: Optional[BoxPlace] = None,
                 size: Optional[BoxSize] = None, vertical: Optional[BoxVertical] = None, ground: Optional[BoxGround] = None,
                 strip: Optional[GroundStrip] = None, virtual: Optional[VirtualPoints] = None, owner: Optional[PointOwner] = None):
        """keep_cloud: also materialise the transformed cloud (`points`, the reference's aggregated `pc`).  The path
        itself does not need it -- the in-mask points are re-derived from the raw rows (hit_xyz) -- so the default is
        off (CM3D_KEEP_CLOUD=1 turns it on); tests and callers that want the cloud back ask for it.
        obb: also fit KITTI's oriented box of every mask on the device (stage_obb, cm3d_obb: src/kitti/2d_to_3d.py:855-876, :1524);
        download() then returns `obb_yaw` and `obb_status`.  Off: no OBB buffer, no OBB launch.
        The four opt-in stages below are off when None (or inactive): then nothing changes, neither a buffer nor a launch.  With any of
        them on, `run` still makes one call, cm3d_lift_pass_composed; include/cm3d_hip.h states where each stage stands in the pass.
        filters: the stage-2 filters (drivable.Stage2Filters; the reference ships them commented out, :755-785).  download(full=True)
        adds `on_road` and `medoid_pos_kept`; `drivable` needs batches with polygon tables (HostBatch.polygons).
        cluster: the depth clustering of the in-mask lists (cluster.DepthCluster; the reference's clusters_hdbscan is dead code), with
        the batch's `ego_xyz` as the frames' origins.  `medoid_pos` is then a position in the clustered list (`cl_off`), and the OBB fit
        sees those lists too; download() adds `cl_off`, `cl_status` (full=True: `cl_idx`, `cl_xyz`), while `hit_off` / `hit_idx` /
        `hit_xyz` stay the raw lists.
        nms: the rotated-box NMS (nms.RotatedNms; the reference's rotated-rectangle nms is dead code): bit 1 of `flags` and column 9 of
        `box` are decided again by the bird's-eye-view overlap of the boxes the pass wrote, everything else stays what the pass wrote.
        yaw: the yaw fit (bevfit.YawFit; nuScenes and Waymo batches -- KITTI's yaw comes from cm3d_obb), on the clustered lists and the
        kept positions where the engine has those.  download() adds `yaw_src`, `fit_status`, `fit_k` and `fit_rect`, and column 5 of
        `box` holds the yaw that was used.
        place: the placement from the fitted rectangle (boxplace.BoxPlace; needs `yaw`): columns 0 and 1 of the boxes whose yaw was
        fitted come from the rectangle's sensor-side corner and faces instead of the view-ray push, and the circle NMS is decided again
        on the new centres (cm3d_box_place, enqueued by cm3d_lift_pass_composed in front of the rotated NMS).  download() adds `place_src`
        and `place_pushed`.  None: no buffer, no launch.
        velocity: the box velocity stage (velocity.Velocity; nuScenes batches, whose boxes are in the global frame): a call of its own
        behind the pass (cm3d_box_velocity) associates the kept boxes of consecutive frames.  It needs batches with `frame_next` and
        `frame_time`; download() adds `vel`, `vel_src`, `next_match` and `prev_match`.  None: no buffer, no call.
        tracks: the track stage (tracks.Tracks; needs `velocity`): one more call behind the velocity stage's (cm3d_box_tracks) follows
        the matches -- bit 1 of `flags`, columns 7 and 9 of `box` are what it leaves, download() adds `track_id`, `track_pos`,
        `track_len`, `track_stat` and, with a smoothing window, `vel_smooth`, which kept_box_velocities then returns.  None or at its
        defaults: no buffer, no call.
        size: the size stage (boxsize.BoxSize; needs `yaw`, `place` and `velocity`): one more call behind the track stage's
        (cm3d_box_size) pools the fitted extents over every track, hangs the pooled length and width on the rectangle by the
        placement's rule -- columns 0 and 1 of `box` are what it leaves -- and takes the velocity again on the new centres.  The track
        stage then runs even at its defaults (`tracks=None` means Tracks()).  download() adds `size_wlh`, `size_src`, `size_ratio`,
        `size_obs`, `size_placed` and `size_vel`; kept_box_sizes returns the rows of the kept boxes and kept_box_velocities those of
        `size_vel`.  None: no buffer, no call.  Its four parameters are untuned.
        vertical: the vertical stage (boxvertical.BoxVertical; nuScenes and Waymo batches, with any other option or none): one call
        directly behind the pass (cm3d_box_vertical), in front of the velocity stage's, takes two order statistics of every in-mask
        list's z -- the clustered lists when the engine clusters -- and rewrites column 2 of `box` where the seen extent agrees with
        the class's prior height or shows only the top.  download() adds `vert_z`, `vert_h`, `vert_src`, `vert_status` and
        `vert_entry_z`; column 2 of kept_box_sizes' rows is then `vert_h`.  None: no buffer, no call.  Its five parameters are untuned.
        ground: the ground stage (boxground.BoxGround; nuScenes and Waymo batches, with any other option or none): one call directly
        behind the vertical stage's, or behind the pass where there is none, and in front of the velocity stage's (cm3d_box_ground)
        streams every frame's sweep rows once more -- the raw rows, or the cloud where the engine has materialised it; it never makes the
        engine materialise it --, takes a low quantile of the heights around every box as its ground and rewrites column 2 of `box`
        where the box can be stood on it.  download() adds `ground_z`, `ground_n`, `ground_h`, `ground_src`, `ground_status` and
        `ground_zref`; column 2 of kept_box_sizes' rows is then `ground_h`.  None: no buffer, no call.  Its seven parameters are untuned.
        strip: the ground strip (groundstrip.GroundStrip; nuScenes and Waymo batches, with any other option or none): directly behind the
        compaction a grid of ground heights is taken from every frame's own sweep rows (cm3d_ground_grid; the raw rows, or the cloud where
        the engine has materialised it -- it never makes the engine materialise it) and every in-mask list loses its ground points
        (cm3d_ground_strip), both enqueued by cm3d_lift_pass_composed.  The clustering, the medoid, the yaw fit and the vertical stage then
        read the stripped lists: `medoid_pos` is a position in the lists the medoid saw -- the clustered ones (`cl_off`) when the engine
        clusters, else the stripped ones (`gs_off`) --, while `hit_off` / `hit_idx` / `hit_xyz` stay the raw lists.  download() adds
        `gs_off`, `gs_status`, `gs_dropped` (full=True: `gs_idx`, `gs_xyz`, `grid_z`, `grid_n`).  None: no buffer, no launch.  Its seven
        parameters are untuned.
        virtual: the virtual points (virtualpoints.VirtualPoints; any batch, KITTI's included, with any other option or none): one call of
        its own behind everything that writes `flags` -- behind the track stage where that runs, else the rotated NMS, else the pass --
        re-projects the lists the medoid saw through every mask's own camera (cm3d_hit_project) and lifts pixels sampled inside every
        eroded mask with the depth of the nearest return in the image (cm3d_virtual_points).  It writes no box, flag or record: every
        other downloaded array is what it is without it.  The sampling takes HostBatch.frame_seed (None: arange(F)).  download() adds
        `vp_count`, `vp_status`, `vp_xyz`, `vp_pix`, `vp_src`, `vp_depth`, `vp_d2` (mask m owns rows [m K, m K + vp_count[m])) and, with
        full=True, `hit_uvd`.  None: no buffer, no call.  Its parameters are untuned.
        owner: the point ownership (pointowner.PointOwner; nuScenes and Waymo batches, with any other option or none): directly behind the
        compaction, in front of the ground strip, every point that several masks of a frame list gets one owner and every list keeps
        the positions it owns (cm3d_point_owner, enqueued by cm3d_lift_pass_composed).  The strip, the clustering, the medoid, the yaw fit,
        the vertical stage and the virtual points then read the exclusive lists: `medoid_pos` is a position in the lists the medoid
        saw -- `cl_off`, else `gs_off`, else `ow_off` --, while `hit_off` / `hit_idx` / `hit_xyz` stay the raw lists.  download() adds
        `ow_off`, `ow_status`, `ow_lost` (full=True: `ow_owner`, `ow_idx`, `ow_xyz`).  None: no buffer, no launch.  Its two parameters
        (rule "score", min_keep 5) are untuned."""
        self.lib = _lib.lib()                      # raises when the extension is not built
        if not torch.cuda.is_available():
            raise Cm3dError("no HIP device: the lifting path only runs on the GPU (no CPU fallback)")
        self.dev = torch.device(device)
        self.classes = classes or ClassTable.nuscenes()
        self.min_dist = float(np.float32(min_dist))
        self.halfw = float(np.float32(np.sqrt(min_dist)))       # :443-444
        self.hits_per_point = hits_per_point
        self.keep_colsum = keep_colsum
        self.keep_cloud = (os.environ.get("CM3D_KEEP_CLOUD", "0") == "1") if keep_cloud is None else bool(keep_cloud)
        self.obb = bool(obb)
        self.filters = filters if filters is not None and filters.active else None
        self.cluster = cluster if cluster is not None and cluster.active else None
        self.nms = nms if nms is not None and nms.active else None
        self.yaw = yaw if yaw is not None and yaw.active else None
        self.velocity = velocity if velocity is not None and velocity.active else None
        self.size = size if size is not None and size.active else None
        self.vertical = vertical if vertical is not None and vertical.active else None
        self.ground = ground if ground is not None and ground.active else None
        self.strip = strip if strip is not None and strip.active else None
        self.virtual = virtual if virtual is not None and virtual.active else None
        self.owner = owner if owner is not None and owner.active else None
        if self.owner is not None and self.obb:
            raise ValueError("owner=PointOwner(...) is stated for nuScenes and Waymo batches; KITTI is out of its scope: it cannot be enabled "
                             "with obb=True")
        if self.strip is not None and self.obb:
            raise ValueError("strip=GroundStrip(...) is stated for nuScenes and Waymo lists (z up); KITTI's rect frame has y down: it cannot be "
                             "enabled with obb=True")
        if self.ground is not None and self.obb:
            raise ValueError("ground=BoxGround(...) is stated for nuScenes and Waymo boxes (z up); KITTI's rect frame has y down and "
                             "its own + h / 2: it cannot be enabled with obb=True")
        if self.vertical is not None and self.obb:
            raise ValueError("vertical=BoxVertical(...) is stated for nuScenes and Waymo boxes (z up); KITTI's rect frame has y down and "
                             "its own + h / 2: it cannot be enabled with obb=True")
        if self.size is not None:
            missing = [n for n, v in (("yaw=YawFit(...)", yaw), ("place=BoxPlace(...)", place), ("velocity=Velocity(...)", velocity))
                       if v is None or not v.active]
            if missing:
                raise ValueError(f"size=BoxSize(...) pools the fitted extents over the tracks and places the boxes again: it needs {', '.join(missing)}")
            self.tracks = tracks if tracks is not None else Tracks()        # the stage runs at its defaults too: the size stage reads its arrays
        else:
            self.tracks = tracks if tracks is not None and tracks.active else None
        if self.tracks is not None and self.velocity is None:
            raise ValueError("tracks=Tracks(...) follows the matches of the velocity stage: it needs velocity=Velocity(...)")
        self.place = place if place is not None and place.active else None
        if self.place is not None and self.yaw is None:
            raise ValueError("place=BoxPlace(...) places boxes from the rectangles of the yaw fit: it needs yaw=YawFit(...)")
        _verify_matrix_pipe(self.lib, self.dev)
        self.b = None
        self._lane = None                                    # the lane tables on the device and their spatial index (upload)
        self._lane_cache = lane_cache if lane_cache is not None else {}      # table set -> tables + index; a LiftPipeline hands its engines one
        d = self.dev
        self.side = torch.cuda.Stream(device=d)              # lane-grid build overlaps the point/mask stages
        self.fused_sweeps = os.environ.get("CM3D_FUSED_SWEEPS", "1") == "1"    # 0: separate sweep and projection launches
        # the medoid stage's feedback word (stage_medoid): starts at 1 = "expect long lists"
        self._md_hint = os.environ.get("CM3D_MD_HINT", "1") == "1"
        self._md_fb = torch.ones(4, dtype=torch.int32).pin_memory()
        self._md_fb_np = self._md_fb.numpy()
        self.graph_captured = False                          # capture_graph: a LiftPipeline then keeps every slot on its own stream
        self.prior_wlh = torch.from_numpy(self.classes.prior_wlh).to(d)
        self.is_vehicle = torch.from_numpy(self.classes.is_vehicle).to(d)
        self.nms_thr = torch.from_numpy(self.classes.nms_thr).to(d)
        self.nms_group = torch.from_numpy(np.ascontiguousarray(self.classes.nms_group, np.int32)).to(d)
        self.needs_road = torch.from_numpy(np.ascontiguousarray(self.classes.needs_road, np.int32)).to(d) if self.filters else None
        self.rot_thr = torch.from_numpy(self.nms.thr_by_group(self.classes)).to(d) if self.nms else None
        self.angle_cs = torch.from_numpy(angle_table(self.yaw.angles)).to(d) if self.yaw else None
        self.vel_speed = torch.from_numpy(self.velocity.speed_by_group(self.classes)).to(d) if self.velocity else None

    # -- upload + allocation
    def upload(self, hb: HostBatch, dense_masks: Optional[torch.Tensor] = None):
        d = self.dev
        def t(a):
            h = torch.from_numpy(np.ascontiguousarray(a))
            return h.to(d, non_blocking=h.is_pinned())        # page-locked staging buffers (cm3d_amd.reader) copy asynchronously
        F, M, S = hb.n_frames, hb.n_masks, len(hb.sweep_row_off) - 1
        if M <= 0 or F <= 0 or S <= 0 or hb.n_raw_rows <= 0:
            raise ValueError("empty batch")
        nm_max = int(np.diff(hb.mask_off).max())
        if hb.n_masks * hb.height * ((hb.width + 31) // 32) > 0x7FFFFFFF:
            raise ValueError(f"{hb.n_masks} masks of {hb.width}x{hb.height} in one batch: their bit-packed words no longer fit a 32-bit offset "
                             "(split the batch)")
        if nm_max > _lib.MAX_MASKS_PER_FRAME:
            raise ValueError(f"{nm_max} masks in one frame (limit {_lib.MAX_MASKS_PER_FRAME})")
        if hb.n_cams > _lib.MAX_CAMS or hb.mask_cam.min() < 0 or hb.mask_cam.max() >= hb.n_cams:
            raise ValueError("cam_nums out of range")
        W, H = hb.width, hb.height
        Wp = (W + 31) // 32
        b = type("DeviceBatch", (), {})()
        b.hb, b.F, b.M, b.S, b.W, b.H, b.Wp = hb, F, M, S, W, H, Wp
        b.sweep_row_off = t(hb.sweep_row_off); b.sweep_xf = t(hb.sweep_xf)
        b.frame_sweep_off = t(hb.frame_sweep_off)
        b.cams = t(hb.cams); b.mask_off = t(hb.mask_off); b.mask_cam = t(hb.mask_cam); b.mask_frame = t(hb.mask_frame)
        b.rle_off = t(hb.rle_off)
        # own (w, h) of every mask where they differ: set on every upload, so that a slot never carries the table of its last batch
        if hb.mask_wh is not None and np.asarray(hb.mask_wh).shape != (M, 2):
            raise ValueError("mask_wh: one (w, h) per mask")
        b.mask_wh = t(np.asarray(hb.mask_wh, np.int32)) if hb.mask_wh is not None else None
        if dense_masks is not None:
            require_one_mask_size(hb)
        b.class_id = t(hb.class_id); b.score = t(hb.score)
        b.pose_rt = t(hb.pose_rt) if hb.pose_rt is not None else None
        b.pose_inv = t(hb.pose_inv) if hb.pose_inv is not None else None
        b.halfw = self.halfw if hb.ego_box else 0.0
        b.frame_lane = t(hb.frame_lane); b.ego_xyz = t(hb.ego_xyz)
        b.pt_cap = hb.n_raw_rows
        b.max_pts = int(max(hb.sweep_row_off[hb.frame_sweep_off[1:]] - hb.sweep_row_off[hb.frame_sweep_off[:-1]]))
        b.planes = (nm_max + 31) // 32
        b.idx_cap = int(max(1024, self.hits_per_point * b.pt_cap))
        e = lambda *shape, dtype=torch.int32: torch.empty(*shape, dtype=dtype, device=d)
        # the transformed cloud exists only on request, or when the sweeps cannot be fused into the projection launch
        b.max_sweeps = int(np.max(np.diff(hb.frame_sweep_off))) if hb.frame_sweep_off.size > 1 else 0
        b.fused = self.fused_sweeps and 0 < b.max_sweeps <= _lib.MAX_FUSED_SWEEPS
        b.points = e(b.pt_cap, 4, dtype=torch.float32) if (self.keep_cloud or not b.fused) else None
        b.pt_off = e(F + 1)
        b.status = torch.zeros(_lib.STATUS_WORDS, dtype=torch.int32, device=d)
        b.packed = e(M, H, Wp)
        b.bbox = e(M, _lib.BBOX_STRIDE)        # [0..3] bounds of the eroded pixels, [4..7] the rectangle `packed` stores
        b.hit_words = e(b.planes, b.pt_cap)
        b.hit_count = e(M); b.hit_off = e(M + 1); b.tile_off = e(M + 1)
        b.hit_idx = e(b.idx_cap); b.hit_xyz = e(b.idx_cap, 4, dtype=torch.float32)
        b.removed_words = int(self.lib.cm3d_removed_words(b.pt_cap, F))
        b.removed_bits = e(b.removed_words)
        b.medoid_pos = e(M); b.centroid = e(M, 3, dtype=torch.float32)
        b.centroid_g = e(M, 3, dtype=torch.float32) if hb.pose_rt is not None else b.centroid
        b.colsum = e(b.idx_cap, dtype=torch.float32) if self.keep_colsum else None
        b.lane_idx = e(M); b.lane_dist = e(M, dtype=torch.float64)
        b.box = e(M, _lib.BOX_STRIDE, dtype=torch.float64); b.flags = e(M)
        L = self.lib
        b.tile_work = torch.empty(int(L.cm3d_tile_work_bytes(M, b.idx_cap)), dtype=torch.uint8, device=d)
        ws = max(L.cm3d_rle_workspace_bytes(max(1, hb.rle_counts.size)),
                 L.cm3d_medoid_workspace_bytes(M, b.idx_cap),
                 L.cm3d_lane_nn_workspace_bytes(M))
        b.ws_bytes = int(ws)
        b.ws = torch.empty(b.ws_bytes, dtype=torch.uint8, device=d)
        # per-(block, mask) hit counts: written by project_hits, consumed by compact_hits
        b.pg_ws_bytes = int(L.cm3d_project_workspace_bytes(F, b.max_pts, b.planes))
        b.pg_ws = torch.empty(max(b.pg_ws_bytes, 16), dtype=torch.uint8, device=d)
        # the RLE run ends stay alive across the whole pass, so they get their own buffer
        b.rle_ws_bytes = int(L.cm3d_rle_workspace_bytes(max(1, hb.rle_counts.size)))
        b.rle_ws = torch.empty(b.rle_ws_bytes, dtype=torch.uint8, device=d)
        if self.obb:                  # the OBB fit keeps its own workspace: nothing it leaves there is read by another stage, nor the reverse
            b.obb_yaw = e(M, dtype=torch.float64); b.obb_status = e(M)
            b.obb_ws_bytes = int(L.cm3d_obb_workspace_bytes(M, b.idx_cap))
            b.obb_ws = torch.empty(b.obb_ws_bytes, dtype=torch.uint8, device=d)
        b.n_tables, b.n_lane = len(hb.lane_off) - 1, int(hb.lane.shape[0])
        b.grid_bytes = int(L.cm3d_lane_grid_bytes(b.n_tables, b.n_lane))
        # The spatial index of the lane tables depends on the tables alone (the reference discretises a scene's lanes once,
        # 2d_to_3d.py:406, and looks every frame of the scene up in them): it is built once per distinct set of tables and kept
        # across passes and uploads -- consecutive batches of a scene, and every pass over a resident batch, reuse it.
        # (a caller that knows which tables these are says so -- pipeline_nuscenes: the map locations --; else their checksum)
        # (the key first: on a hit the tables are neither uploaded -- a pageable, host-blocking copy of megabytes -- nor read for a
        # checksum; the checksum of a table set is kept on the host batch.  The cache is shared by the engines of a LiftPipeline:
        # consecutive batches of a job alternate between them.)
        key = hb.lane_tables_key()
        hit = self._lane_cache.get(key)
        if hit is not None:
            self._lane = hit
            b.lane, b.lane_off, b.grid = hit["lane"], hit["lane_off"], hit["grid"]
        else:
            b.lane = t(hb.lane); b.lane_off = t(hb.lane_off)
            b.grid = torch.empty(b.grid_bytes, dtype=torch.uint8, device=d)
            up = torch.cuda.Event()
            up.record(torch.cuda.current_stream(d))         # whichever engine builds the index waits for the tables' copies (its streams are not this one)
            self._lane = {"key": key, "lane": b.lane, "lane_off": b.lane_off, "grid": b.grid, "built": False, "tables_uploaded": up,
                          "built_event": torch.cuda.Event()}
            if len(self._lane_cache) >= 8:                  # a handful of cities per job: keep the cache small
                self._lane_cache.pop(next(iter(self._lane_cache)))
            self._lane_cache[key] = self._lane
        if self.filters is not None:
            b.medoid_pos_kept = e(M); b.on_road = e(M, dtype=torch.uint8)
            b.polygon_index = self._polygon_index(hb, b.n_tables) if self.filters.drivable else None
        if self.cluster is not None:
            b.cl_off = e(M + 1); b.cl_tile_off = e(M + 1); b.cl_status = e(M)
            b.cl_idx = e(b.idx_cap); b.cl_xyz = e(b.idx_cap, 4, dtype=torch.float32)
            b.cl_ws_bytes = int(L.cm3d_depth_cluster_workspace_bytes(M, b.idx_cap))
            b.cl_ws = torch.empty(max(b.cl_ws_bytes, 16), dtype=torch.uint8, device=d)
        if self.strip is not None:
            b.gs_off = e(M + 1); b.gs_tile_off = e(M + 1); b.gs_status = e(M); b.gs_dropped = e(M)
            b.gs_idx = e(b.idx_cap); b.gs_xyz = e(b.idx_cap, 4, dtype=torch.float32)
            b.grid_z = e(F, GRID_CELLS, dtype=torch.float64); b.grid_n = e(F, GRID_CELLS)
            b.gs_ws_bytes = int(L.cm3d_ground_strip_workspace_bytes(M, b.idx_cap))
            b.gs_ws = torch.empty(max(b.gs_ws_bytes, 16), dtype=torch.uint8, device=d)
        if self.owner is not None:
            b.ow_owner = e(b.idx_cap); b.ow_off = e(M + 1); b.ow_tile_off = e(M + 1); b.ow_status = e(M); b.ow_lost = e(M)
            b.ow_idx = e(b.idx_cap); b.ow_xyz = e(b.idx_cap, 4, dtype=torch.float32)
            b.ow_ws_bytes = int(L.cm3d_point_owner_workspace_bytes(F, b.max_pts, M, b.idx_cap))
            b.ow_ws = torch.empty(max(b.ow_ws_bytes, 16), dtype=torch.uint8, device=d)
        if self.yaw is not None:
            b.fit_k = e(M); b.fit_status = e(M); b.fit_rect = e(M, _lib.MATCH_BOX_STRIDE, dtype=torch.float64)
            b.yaw_tab = e(M, 3, dtype=torch.float32); b.yaw_idx = e(M); b.yaw_src = e(M)
            b.yaw_tab_off = t(np.array([0, M], np.int32)); b.yaw_tab_frame = torch.zeros(F, dtype=torch.int32, device=d)
        if self.place is not None:
            b.place_src = e(M); b.place_pushed = e(M, 2, dtype=torch.float64)
        if self.velocity is not None:
            if hb.frame_next is None or hb.frame_time is None:
                raise ValueError("the velocity stage needs HostBatch.frame_next and frame_time (the batch was assembled without the "
                                 "sample table's `next` and `timestamp`): it cannot be enabled for this batch")
            if hb.pose_rt is not None:
                raise ValueError("the velocity stage takes boxes in the global frame (nuScenes); this batch's are in the vehicle frame")
            nxt, tim = _as(hb.frame_next, np.int32).reshape(-1), _as(hb.frame_time, np.float64).reshape(-1)
            if nxt.size != F or tim.size != F:
                raise ValueError("frame_next / frame_time: one entry per frame")
            pair_off = link_table(hb.mask_off, nxt, tim, self.velocity.max_dt, M)[2]      # from the host's arrays alone: no read-back
            b.frame_next, b.frame_time, b.vel_pair_off, b.vel_pairs = t(nxt), t(tim), t(pair_off), int(pair_off[-1])
            b.next_match = e(M); b.prev_match = e(M); b.vel_src = e(M); b.vel = e(M, 2, dtype=torch.float64)
            b.vel_status = torch.zeros(1, dtype=torch.int32, device=d)
            b.vel_ws_bytes = int(L.cm3d_box_velocity_workspace_bytes(b.vel_pairs, M))
            b.vel_ws = torch.empty(max(b.vel_ws_bytes, 16), dtype=torch.uint8, device=d)
        if self.tracks is not None:
            b.track_id = e(M); b.track_pos = e(M); b.track_len = e(M); b.track_stat = e(M, 4, dtype=torch.float64)
            b.vel_smooth = e(M, 2, dtype=torch.float64) if self.tracks.smooth_window > 0 else None
            b.track_status = torch.zeros(1, dtype=torch.int32, device=d)
            b.track_ws_bytes = int(L.cm3d_box_tracks_workspace_bytes(M))
            b.track_ws = torch.empty(max(b.track_ws_bytes, 16), dtype=torch.uint8, device=d)
        if self.size is not None:
            b.size_wlh = e(M, 3, dtype=torch.float64); b.size_src = e(M); b.size_ratio = e(M, 2, dtype=torch.float64); b.size_obs = e(M, 2)
            b.size_placed = e(M, 2, dtype=torch.float64); b.size_vel = e(M, 2, dtype=torch.float64)
            b.size_status = torch.zeros(1, dtype=torch.int32, device=d)
            b.size_ws_bytes = int(L.cm3d_box_size_workspace_bytes(M))
            b.size_ws = torch.empty(max(b.size_ws_bytes, 16), dtype=torch.uint8, device=d)
        if self.vertical is not None:
            b.vert_z = e(M, 2, dtype=torch.float64); b.vert_h = e(M, dtype=torch.float64); b.vert_entry_z = e(M, dtype=torch.float64)
            b.vert_src = e(M); b.vert_status = e(M)
            b.prior_wlh = self.prior_wlh          # (kept_box_sizes: the length and width of a box without a size stage)
        if self.virtual is not None:
            if H > _lib.VP_MAX_ROWS:
                raise ValueError(f"virtual=VirtualPoints(...): images of more than {_lib.VP_MAX_ROWS} rows ({H})")
            K = self.virtual.per_mask
            seeds = np.arange(F, dtype=np.uint32) if hb.frame_seed is None else np.asarray(hb.frame_seed).astype(np.uint32).reshape(-1)
            if seeds.size != F:
                raise ValueError("frame_seed: one word per frame")
            b.frame_seed = t(seeds.view(np.int32))
            b.hit_uvd = e(b.idx_cap, 4, dtype=torch.float32)
            b.vp_count = e(M); b.vp_status = e(M); b.vp_xyz = e(M * K, 3, dtype=torch.float64); b.vp_pix = e(M * K, 2); b.vp_src = e(M * K)
            b.vp_depth = e(M * K, dtype=torch.float32); b.vp_d2 = e(M * K, dtype=torch.float32)
        if self.ground is not None:
            b.ground_z = e(M, dtype=torch.float64); b.ground_h = e(M, dtype=torch.float64); b.ground_zref = e(M, dtype=torch.float64)
            b.ground_n = e(M); b.ground_src = e(M); b.ground_status = e(M)
            b.nm_max = nm_max
            b.prior_wlh = self.prior_wlh
        b.dense = dense_masks
        # The bulk data LAST: sweeps and run lengths come from page-locked staging buffers (cm3d_amd.reader) and copy
        # asynchronously; the small arrays above are pageable, their copies block the host until everything queued before them on
        # the stream is done -- behind the 180 MB of a C2 batch's sweeps that was the whole transfer time (4 ms), per batch.
        b.rle_counts = t(hb.rle_counts.view(np.int32))
        b.intensity = t(hb.intensity) if hb.intensity is not None else None
        b.raw = t(hb.raw)
        # what a pass hands to the library (cm3d_lift_pass), filled once; `refresh_pass_descriptor` adds what changes from pass to pass
        b.desc = self._batch_descriptor(b)
        b.desc_ref = ctypes.byref(b.desc)
        # the opt-in stages (cm3d_lift_pass_opt): one descriptor per stage the engine has -- `b.filter_desc` ... `b.nms_desc`, which keep
        # them alive -- and the record that points at them.  `timed`: those with an event pair, in the order `run` appends their events
        stages = {"filter": self.filters and self._filter_descriptor(b), "cluster": self.cluster and self._cluster_descriptor(b),
                  "yaw": self.yaw and self._yaw_descriptor(b), "nms": self.nms and self._nms_descriptor()}
        stages = {name: desc for name, desc in stages.items() if desc is not None}
        b.opts = _lib.LiftPassOptions()
        b.opts.size = ctypes.sizeof(_lib.LiftPassOptions)
        for name, desc in stages.items():
            setattr(b, name + "_desc", desc)
            setattr(b.opts, name, ctypes.addressof(desc))
        # the stages the options have no member for: cm3d_lift_pass_composed takes their descriptors beside the options
        beside = {"owner": self.owner and self._owner_descriptor(b), "strip": self.strip and self._strip_descriptor(b),
                  "place": self.place and self._place_descriptor(b)}
        beside = {name: desc for name, desc in beside.items() if desc is not None}
        for name, desc in beside.items():
            setattr(b, name + "_desc", desc)
        have = {**stages, **beside}
        b.timed = {name: have[name] for name in TIMED_ORDER if name in have}
        b.opts_ref = ctypes.byref(b.opts) if stages else None
        b.place_ref, b.strip_ref, b.owner_ref = (ctypes.byref(beside[name]) if name in beside else None for name in ("place", "strip", "owner"))
        b.plain_pass = not stages and self.velocity is None and self.vertical is None and self.ground is None and self.strip is None and self.virtual is None and self.owner is None      # what cm3d_pipe_submit can enqueue by itself (LiftPipeline.rerun)
        self.b = b
        return b

    def _polygon_index(self, hb, n_tables):
        """The batch's polygon index on the device: built on the host once per set of polygon tables (drivable.build_index: static data,
        a handful of cities per job) and kept beside the lane index, in the cache the engines of a LiftPipeline share."""
        if hb.polygons is None or len(hb.polygons) != n_tables:
            raise ValueError("the drivable filter needs HostBatch.polygons: one polygon table per lane table")
        key = hb.polygon_tables_key()
        hit = self._lane_cache.get(key)
        if hit is None:
            from . import ops
            hit = ops.upload_polygon_index(drivable.build_index(hb.polygons), self.dev)
            if len(self._lane_cache) >= 8:
                self._lane_cache.pop(next(iter(self._lane_cache)))
            self._lane_cache[key] = hit
        return hit

    def _filter_descriptor(self, b):
        """cm3d_stage2_filter_desc of the resident batch (refresh_pass_descriptor sets its events)."""
        f = _lib.Stage2FilterDesc()
        f.size = ctypes.sizeof(_lib.Stage2FilterDesc)
        if b.polygon_index is not None:
            for name in _lib.POLY_INDEX_ARRAYS:
                setattr(f, name, b.polygon_index[name].data_ptr())
            f.n_poly_tables = b.polygon_index["n_tables"]
        f.needs_road = _ptr(self.needs_road)
        f.medoid_pos_kept, f.on_road = _ptr(b.medoid_pos_kept), _ptr(b.on_road)
        f.lane_max_dist, f.vehicle_lane_max_dist = self.filters.lane_max_dist, self.filters.vehicle_lane_max_dist
        return f

    def _cluster_descriptor(self, b):
        """cm3d_depth_cluster_desc of the resident batch (refresh_pass_descriptor sets its events).  The origin of frame f is ego_xyz[f]: the LIDAR_TOP ego
        translation on nuScenes, zeros on Waymo (vehicle frame) and on KITTI (reference-camera frame)."""
        c = _lib.DepthClusterDesc()
        c.size = ctypes.sizeof(_lib.DepthClusterDesc)
        c.origin = _ptr(b.ego_xyz)
        for name in ("cl_off", "cl_tile_off", "cl_idx", "cl_xyz", "cl_status"):
            setattr(c, name, _ptr(getattr(b, name)))
        c.ws, c.ws_bytes = _ptr(b.cl_ws), b.cl_ws_bytes
        c.eps, c.min_points, c.pick = self.cluster.eps, self.cluster.min_points, self.cluster.pick_index
        return c

    def _strip_descriptor(self, b):
        """cm3d_ground_strip_desc of the resident batch (refresh_pass_descriptor sets its events).  The origin of frame f is ego_xyz[f], as
        the clustering's."""
        s, g = _lib.GroundStripDesc(), self.strip
        s.size = ctypes.sizeof(_lib.GroundStripDesc)
        s.origin = _ptr(b.ego_xyz)
        for name in ("grid_z", "grid_n", "gs_off", "gs_tile_off", "gs_idx", "gs_xyz", "gs_status", "gs_dropped"):
            setattr(s, name, _ptr(getattr(b, name)))
        s.ws, s.ws_bytes = _ptr(b.gs_ws), b.gs_ws_bytes
        s.cell, s.down, s.up, s.quantile, s.margin = g.cell, g.down, g.up, g.quantile, g.margin
        s.min_points, s.min_keep = g.min_points, g.min_keep
        return s

    def _owner_descriptor(self, b):
        """cm3d_point_owner_desc of the resident batch (refresh_pass_descriptor sets its events)."""
        w = _lib.PointOwnerDesc()
        w.size = ctypes.sizeof(_lib.PointOwnerDesc)
        for name in ("ow_owner", "ow_off", "ow_tile_off", "ow_idx", "ow_xyz", "ow_status", "ow_lost"):
            setattr(w, name, _ptr(getattr(b, name)))
        w.ws, w.ws_bytes = _ptr(b.ow_ws), b.ow_ws_bytes
        w.rule, w.min_keep = self.owner.code, self.owner.min_keep
        return w

    def read_lists(self, b=None):
        """The lists the stages behind the seam read, as (xyz, off) device tensors of the resident batch (or of `b`): the clustered ones
        when the engine clusters, else the stripped ones when it strips, else the exclusive ones when it decides ownership, else the raw
        ones.  `medoid_pos` is a position in them."""
        return self._seen_lists(b)[:2]

    def _seen_lists(self, b=None, behind=None):
        """(xyz, off, idx) of the lists behind stage `behind` ("owner", "strip"; None: behind the clustering, the lists the medoid saw)."""
        b = self.b if b is None else b
        if self.cluster is not None and behind is None:
            return b.cl_xyz, b.cl_off, b.cl_idx
        if self.strip is not None and behind != "owner":
            return b.gs_xyz, b.gs_off, b.gs_idx
        if self.owner is not None:
            return b.ow_xyz, b.ow_off, b.ow_idx
        return b.hit_xyz, b.hit_off, b.hit_idx

    def _yaw_descriptor(self, b):
        """cm3d_yaw_fit_desc of the resident batch (refresh_pass_descriptor sets its events).  The lists that are fitted are the clustered
        ones when the engine clusters, the positions that decide about a box the kept ones when it filters: what cm3d_lift_pass_opt
        derives itself, stated here for cm3d_yaw_fit_boxes alone (stage_yaw_fit)."""
        y = _lib.YawFitDesc()
        y.size = ctypes.sizeof(_lib.YawFitDesc)
        y.angle_cs = _ptr(self.angle_cs)
        if self.cluster is not None or self.strip is not None or self.owner is not None:
            xyz, off = self.read_lists(b)
            y.hit_xyz, y.hit_off = _ptr(xyz), _ptr(off)
        if self.filters is not None:
            y.medoid_pos = _ptr(b.medoid_pos_kept)
        for name in ("fit_k", "fit_rect", "fit_status", "yaw_tab", "yaw_idx", "yaw_src"):
            setattr(y, name, _ptr(getattr(b, name)))
        y.tab_off, y.tab_frame = _ptr(b.yaw_tab_off), _ptr(b.yaw_tab_frame)
        y.K, y.min_points = self.yaw.angles, self.yaw.min_points
        y.d0, y.min_length, y.lane_min_dist = self.yaw.d0, self.yaw.min_length, self.yaw.lane_min_dist
        return y

    def _place_descriptor(self, b):
        """cm3d_box_place_desc of the resident batch (refresh_pass_descriptor sets its events)."""
        p = _lib.BoxPlaceDesc()
        p.size = ctypes.sizeof(_lib.BoxPlaceDesc)
        p.place_src, p.place_pushed, p.thin = _ptr(b.place_src), _ptr(b.place_pushed), self.place.thin
        return p

    def _nms_descriptor(self):
        """cm3d_rotated_nms_desc of the engine: what cm3d_box_rotated_nms takes beyond the pass descriptor."""
        n = _lib.RotatedNmsDesc()
        n.size = ctypes.sizeof(_lib.RotatedNmsDesc)
        n.thr, n.n_thr, n.measure, n.class_agnostic = _ptr(self.rot_thr), self.rot_thr.numel(), self.nms.measure_index, int(self.nms.class_agnostic)
        return n

    def _batch_descriptor(self, b):
        """cm3d_lift_pass_desc of the resident batch: the arguments of the calls a pass makes, name for name (the fields that belong to
        the batch; `refresh_pass_descriptor` sets the per-pass ones)."""
        d = _lib.LiftPassDesc()
        d.size = ctypes.sizeof(_lib.LiftPassDesc)
        for name in ("rle_counts", "rle_off", "packed", "bbox", "rle_ws", "status", "hit_count", "removed_bits", "raw", "intensity",
                     "sweep_row_off", "sweep_xf", "frame_sweep_off", "points", "pt_off", "cams", "mask_off", "mask_cam", "hit_words", "pg_ws",
                     "hit_off", "tile_off", "hit_idx", "hit_xyz", "tile_work", "medoid_pos", "centroid", "colsum", "ws", "centroid_g",
                     "mask_frame", "lane", "lane_off", "frame_lane", "grid", "lane_idx", "lane_dist", "class_id", "score", "ego_xyz", "box",
                     "flags", "mask_wh", "pose_rt", "pose_inv"):
            setattr(d, name, _ptr(getattr(b, name)) or None)
        for name in ("prior_wlh", "is_vehicle", "nms_group", "nms_thr"):
            setattr(d, name, _ptr(getattr(self, name)))
        if self.obb:
            d.obb_yaw, d.obb_status, d.obb_ws, d.obb_ws_bytes = _ptr(b.obb_yaw), _ptr(b.obb_status), _ptr(b.obb_ws), b.obb_ws_bytes
        d.md_feedback = self._md_fb.data_ptr()
        d.rle_ws_bytes, d.removed_words, d.pg_ws_bytes, d.ws_bytes = b.rle_ws_bytes, b.removed_words, b.pg_ws_bytes, b.ws_bytes
        d.n_masks, d.total_runs, d.W, d.H = b.M, b.hb.rle_counts.size, b.W, b.H
        d.raw_stride, d.n_sweeps, d.max_sweeps_per_frame, d.pt_cap = b.hb.raw_stride, b.S, b.max_sweeps, b.pt_cap
        d.max_rows_per_sweep = b.hb.max_rows_per_sweep
        d.n_frames, d.max_pts_per_frame, d.n_cams, d.planes, d.idx_cap = b.F, b.max_pts, b.hb.n_cams, b.planes, b.idx_cap
        d.n_tables, d.n_lane_points, d.n_classes = b.n_tables, b.n_lane, len(self.classes.names)
        d.halfw, d.min_dist = b.halfw, self.min_dist
        return d

    def resident_masks(self, masks):
        """What the descriptor's `dense` takes for a mask mode: the resident dense masks, or None for the run lengths."""
        b = self.b
        if masks == "rle":
            return None
        if masks != "dense":
            raise ValueError(masks)
        require_one_mask_size(b.hb)
        if b.dense is None:
            raise Cm3dError("dense masks requested but not resident: call decode_masks_dense() or pass dense_masks")
        return b.dense.data_ptr()

    def refresh_pass_descriptor(self, dense=None, project_events=None, stage_events=None, option_events=None):
        """The descriptor of the next pass over the resident batch, for cm3d_lift_pass[_opt] / cm3d_pipe_submit: sets what may change
        between two passes over one batch -- the mask route (`dense`: resident_masks), the reset, the hint switch, the lane index in use
        and whether its build has to be waited for, the events (project_events: a pair of torch.cuda.Event, stage_events: five,
        option_events: stage name -> pair, for `b.timed`; every slot is set or cleared on every pass, so none keeps the event of an
        earlier one) -- and counts the pass.  The build of the lane index must have been started (start_lane_grid)."""
        b = self.b
        d = b.desc
        d.dense = dense
        d.fused = b.fused
        d.separate_reset = os.environ.get("CM3D_FUSED_RESET", "1") == "0"        # the reset as a launch of its own
        d.md_hint = self._md_hint
        d.grid = b.grid.data_ptr()
        ln = self._lane
        if not ln.get("done") and ln["built_event"].query():
            ln["done"] = True                # the build has completed: nothing left to wait for
        d.lane_ready = None if ln.get("done") else ln["built_event"].cuda_event
        d.ev_project[:] = self._raw_events(project_events, 2)
        d.ev_stage[:] = self._raw_events(stage_events, 5)
        for name, desc in b.timed.items():
            desc.ev[:] = self._raw_events((option_events or {}).get(name), 2)
        ln["passes_since_build"] = ln.get("passes_since_build", 0) + 1
        return b.desc_ref

    def decode_masks_dense(self):
        """a1: RLE -> dense uint8 (M,H,W) on the device (pycocotools.mask.decode, reference :425)."""
        b = self.b
        require_one_mask_size(b.hb)
        if b.dense is None:
            b.dense = torch.empty(b.M, b.H, b.W, dtype=torch.uint8, device=self.dev)
        st = torch.cuda.current_stream(self.dev).cuda_stream
        check(self.lib.cm3d_rle_to_dense(_ptr(b.rle_counts), _ptr(b.rle_off), b.M, b.hb.rle_counts.size, b.W, b.H,
                                         _ptr(b.dense), _ptr(b.rle_ws), b.rle_ws_bytes, st), "cm3d_rle_to_dense")
        return b.dense

    # -- the stages, in reference order
    def stage_begin(self, st, defer_reset=False):
        """Resets the per-pass state and starts the lane-grid build on the side stream.  defer_reset: the reset rides on the mask stage's
        launch instead (stage_masks(..., reset=True): a pass does that for resident run lengths on the fused-sweeps path, one launch less
        per pass)."""
        b = self.b
        if not defer_reset:
            check(self.lib.cm3d_batch_begin(_ptr(b.status), _ptr(b.hit_count), b.M, _ptr(b.removed_bits), b.removed_words, st),
                  "cm3d_batch_begin")
        if not self._lane["built"]:
            self.start_lane_grid()

    def start_lane_grid(self):
        """Builds the lane index on the side stream, behind what the current stream holds so far, and records its event.  (Not needed
        while the lane tables are those of the last build: the index is still valid.)"""
        main = torch.cuda.current_stream(self.dev)
        self.side.wait_stream(main)          # the uploads of the tables have been issued before this point
        self.side.wait_event(self._lane["tables_uploaded"])     # (by another engine of the pipeline, on its stream, when the entry is shared)
        with torch.cuda.stream(self.side):
            self.stage_lane_grid(self.side.cuda_stream)
            self._lane["built_event"].record(self.side)
        self._lane["built"], self._lane["done"], self._lane["passes_since_build"] = True, False, 0

    def wait_lane_grid(self):
        """Orders the current stream behind the build of the lane index (by whichever engine of the pipeline built it; nothing to do
        once the host has seen a pass that followed the build complete: check_status / download / capture_graph note that)."""
        if not self._lane.get("done"):
            torch.cuda.current_stream(self.dev).wait_event(self._lane["built_event"])

    def rebuild_lane_grid(self):
        """Forgets the cached lane index: the next pass builds it again (benchmarks that want the build inside a pass)."""
        if self._lane is not None:
            self._lane["built"], self._lane["done"] = False, False

    def stage_sweeps(self, st):
        b = self.b
        check(self.lib.cm3d_sweep_prep(_ptr(b.raw), b.hb.raw_stride, _ptr(b.intensity), _ptr(b.sweep_row_off), b.S, b.hb.max_rows_per_sweep,
                                       _ptr(b.sweep_xf), _ptr(b.frame_sweep_off), b.F, b.halfw, _ptr(b.points), b.pt_cap,
                                       _ptr(b.pt_off), _ptr(b.removed_bits), _ptr(b.status), st), "cm3d_sweep_prep")

    def stage_masks(self, st, masks="dense", reset=False):
        """reset (run lengths only): this launch also does cm3d_batch_begin's work -- it must then be the first call of the pass."""
        b = self.b
        if reset:
            if masks != "rle":
                raise ValueError("the per-pass reset rides on the run-length mask launch only")
            if b.mask_wh is not None:
                check(self.lib.cm3d_rle_erode_pack_sized_begin(_ptr(b.rle_counts), _ptr(b.rle_off), b.M, b.hb.rle_counts.size, b.W, b.H,
                                                               _ptr(b.mask_wh), _ptr(b.packed), _ptr(b.bbox), _ptr(b.rle_ws), b.rle_ws_bytes,
                                                               _ptr(b.status), _ptr(b.hit_count), b.M, _ptr(b.removed_bits), b.removed_words, st),
                      "cm3d_rle_erode_pack_sized_begin")
                return
            check(self.lib.cm3d_rle_erode_pack_begin(_ptr(b.rle_counts), _ptr(b.rle_off), b.M, b.hb.rle_counts.size, b.W, b.H,
                                                     _ptr(b.packed), _ptr(b.bbox), _ptr(b.rle_ws), b.rle_ws_bytes,
                                                     _ptr(b.status), _ptr(b.hit_count), b.M, _ptr(b.removed_bits), b.removed_words, st),
                  "cm3d_rle_erode_pack_begin")
            return
        if masks == "dense":
            require_one_mask_size(b.hb)
            if b.dense is None:
                raise Cm3dError("dense masks requested but not resident: call decode_masks_dense() or pass dense_masks")
            check(self.lib.cm3d_erode_pack(_ptr(b.dense), b.M, b.W, b.H, _ptr(b.packed), _ptr(b.bbox), st), "cm3d_erode_pack")
        elif masks == "rle" and b.mask_wh is not None:
            check(self.lib.cm3d_rle_erode_pack_sized(_ptr(b.rle_counts), _ptr(b.rle_off), b.M, b.hb.rle_counts.size, b.W, b.H, _ptr(b.mask_wh),
                                                     _ptr(b.packed), _ptr(b.bbox), _ptr(b.rle_ws), b.rle_ws_bytes, st),
                  "cm3d_rle_erode_pack_sized")
        elif masks == "rle":
            check(self.lib.cm3d_rle_erode_pack(_ptr(b.rle_counts), _ptr(b.rle_off), b.M, b.hb.rle_counts.size, b.W, b.H,
                                               _ptr(b.packed), _ptr(b.bbox), _ptr(b.rle_ws), b.rle_ws_bytes, st),
                  "cm3d_rle_erode_pack")
        else:
            raise ValueError(masks)

    def stage_project(self, st, events=None):
        """events: optional pair of torch.cuda.Event (enable_timing) that the library records around the projection
        kernel itself on the launch stream (bench.py's roofline timing)."""
        b = self.b
        e0, e1 = self._raw_events(events, 2)
        check(self.lib.cm3d_project_hits(_ptr(b.points), _ptr(b.pt_off), b.F, b.max_pts, b.pt_cap, _ptr(b.cams), b.hb.n_cams,
                                         _ptr(b.mask_off), _ptr(b.mask_cam), _ptr(b.bbox), _ptr(b.packed), b.M, b.W, b.H,
                                         self.min_dist, b.planes, _ptr(b.hit_words), _ptr(b.hit_count), _ptr(b.status),
                                         _ptr(b.pg_ws), b.pg_ws_bytes, e0, e1, st), "cm3d_project_hits")

    @staticmethod
    def _raw_events(events, n):
        """n torch events -> the hipEvent_t handles the C-ABI takes (created by a first record on the current stream); None: n times none."""
        if events is None:
            return [None] * n
        out = []
        for ev in events:
            if ev.cuda_event == 0 or ev.cuda_event is None:
                ev.record()
            out.append(int(ev.cuda_event))
        if len(out) != n:
            raise ValueError(f"{n} events expected")
        return out

    def can_fuse_sweeps(self):
        return self.b.fused

    def stage_sweep_project(self, st, events=None):
        """Sweep preparation folded into the projection kernel (cm3d_sweep_project_hits): same outputs as
        stage_sweeps + stage_project, the cloud crosses HBM once less.  Needs the masks of the batch (stage_masks) first."""
        b = self.b
        e0, e1 = self._raw_events(events, 2)
        check(self.lib.cm3d_sweep_project_hits(_ptr(b.raw), b.hb.raw_stride, _ptr(b.intensity), _ptr(b.sweep_row_off), b.S, b.max_sweeps, _ptr(b.sweep_xf),
                                               _ptr(b.frame_sweep_off), b.halfw, _ptr(b.points), b.pt_cap, _ptr(b.pt_off),
                                               _ptr(b.removed_bits), b.F, b.max_pts, b.pt_cap, _ptr(b.cams),
                                               b.hb.n_cams, _ptr(b.mask_off), _ptr(b.mask_cam), _ptr(b.bbox), _ptr(b.packed), b.M, b.W,
                                               b.H, self.min_dist, b.planes, _ptr(b.hit_words), _ptr(b.hit_count), _ptr(b.status),
                                               _ptr(b.pg_ws), b.pg_ws_bytes, e0, e1, st), "cm3d_sweep_project_hits")

    def stage_compact(self, st):
        b = self.b
        # coordinates of the in-mask points: from the cloud when it exists, else re-derived from the raw rows
        from_raw = b.points is None
        check(self.lib.cm3d_compact_hits(_ptr(b.hit_words), b.planes, b.F, b.max_pts, b.pt_cap, _ptr(b.mask_off), b.M, _ptr(b.hit_count),
                                         _ptr(b.removed_bits), _ptr(b.raw) if from_raw else 0, b.hb.raw_stride,
                                         _ptr(b.intensity) if from_raw else 0, _ptr(b.sweep_xf) if from_raw else 0, _ptr(b.points), _ptr(b.hit_off), _ptr(b.tile_off),
                                         _ptr(b.hit_idx), 0, _ptr(b.hit_xyz), b.idx_cap, _ptr(b.tile_work), _ptr(b.status),
                                         _ptr(b.pg_ws), b.pg_ws_bytes, st), "cm3d_compact_hits")

    def stage_medoid(self, st):
        """The medoid stage.  In a batch with a list of more than 448 points, lists of more than 256 go a two-pass route that costs two
        launches even when a batch holds no such list (they find that out on the device: 2-3 % of a pass with three batches in flight).  The first launch leaves word 0
        of `self._md_fb` -- page-locked host memory the device writes directly, no copy -- saying whether THIS batch held one; the next
        pass of this engine reads whatever has arrived by then and, if the last batch it heard of had none, asks for the one-pass
        route only (cm3d_medoid2 flags bit 0).  That route is exact for every length: a stale hint costs time on one pass, never a
        result."""
        b = self.b
        flags = 1 if (self._md_hint and int(self._md_fb_np[0]) == 0) else 0
        check(self.lib.cm3d_medoid2(_ptr(b.hit_xyz), 0, 0, b.M, _ptr(b.hit_off), _ptr(b.tile_off), 0, b.idx_cap, _ptr(b.tile_work),
                                    _ptr(b.medoid_pos), _ptr(b.centroid), _ptr(b.colsum), _ptr(b.ws), b.ws_bytes, flags,
                                    self._md_fb.data_ptr(), st), "cm3d_medoid2")

    def stage_lane_grid(self, st):
        """Spatial index of the lane tables.  It depends on the lane tables only, so `run` issues it on
        the side stream at the start of the pass; it overlaps the sweep / mask / projection stages."""
        b = self.b
        check(self.lib.cm3d_lane_grid_build(_ptr(b.lane), _ptr(b.lane_off), b.n_tables, b.n_lane, _ptr(b.grid), b.grid_bytes, st),
              "cm3d_lane_grid_build")

    def stage_lanes(self, st):
        b = self.b
        if b.pose_rt is not None:       # Waymo: the lane lookup happens in the global frame
            check(self.lib.cm3d_centroid_transform(_ptr(b.centroid), _ptr(b.medoid_pos), _ptr(b.mask_frame), b.M, _ptr(b.pose_rt),
                                                   _ptr(b.centroid_g), st), "cm3d_centroid_transform")
        check(self.lib.cm3d_lane_nn(_ptr(b.centroid_g), _ptr(b.medoid_pos), _ptr(b.mask_frame), b.M, _ptr(b.lane), _ptr(b.lane_off),
                                    _ptr(b.frame_lane), b.n_tables, b.n_lane, _ptr(b.grid), _ptr(b.lane_idx),
                                    _ptr(b.lane_dist), _ptr(b.ws), b.ws_bytes, st), "cm3d_lane_nn")

    @staticmethod
    def _mask_bound(b):
        """`planes` words of mask bits per point: no frame of the batch has more than 32 * planes masks -- the bound cm3d_lift_pass hands
        to the box launch, the rotated NMS and the placement."""
        return min(32 * b.planes, _lib.MAX_MASKS_PER_FRAME)

    def stage_boxes(self, st, medoid_pos=None):
        """The box launch on the resident results.  medoid_pos: the positions that decide which masks have a box (None: the medoid
        stage's; an engine with filters hands `b.medoid_pos_kept` for the launch behind the filter)."""
        b = self.b
        check(self.lib.cm3d_box_nms_bounded(_ptr(b.centroid_g), _ptr(b.medoid_pos if medoid_pos is None else medoid_pos), _ptr(b.mask_off),
                                            b.F, b.M, _ptr(b.class_id),
                                            _ptr(b.score), _ptr(b.lane), _ptr(b.lane_off), _ptr(b.frame_lane), _ptr(b.lane_idx),
                                            _ptr(b.lane_dist), _ptr(self.prior_wlh), _ptr(self.is_vehicle), _ptr(self.nms_group),
                                            _ptr(self.nms_thr), len(self.classes.names), _ptr(b.ego_xyz), _ptr(b.pose_inv),
                                            self._mask_bound(b), _ptr(b.box), _ptr(b.flags), st),
              "cm3d_box_nms_bounded")

    def stage_obb(self, st):
        """a18 (KITTI): yaw of the oriented box of every mask's in-mask points (cm3d_obb), on hit_xyz / hit_off of the compaction."""
        b = self.b
        check(self.lib.cm3d_obb(_ptr(b.hit_xyz), _ptr(b.hit_off), b.M, b.idx_cap, _ptr(b.obb_yaw), _ptr(b.obb_status), 0, 0,
                                _ptr(b.obb_ws), b.obb_ws_bytes, st), "cm3d_obb")

    def stage_cluster(self, st):
        """The depth clustering alone, on the raw lists the last pass left resident -- the stripped ones when the engine strips --
        (cm3d_depth_cluster: what the clustered pass enqueues between the compaction, or the strip, and the medoid)."""
        b, c = self.b, self.b.cluster_desc
        if self.strip is not None or self.owner is not None:       # (what the stripped pass, or the owned pass, clusters)
            xyz, off, idx = self._seen_lists(b, "strip")
            check(self.lib.cm3d_depth_cluster(_ptr(xyz), _ptr(idx), _ptr(off), _ptr(b.mask_frame), b.M, b.idx_cap, c.origin, b.F,
                                              c.eps, c.min_points, c.pick, c.cl_off, c.cl_tile_off, c.cl_idx, c.cl_xyz, c.cl_status, c.ws,
                                              c.ws_bytes, st), "cm3d_depth_cluster")
            return
        check(self.lib.cm3d_depth_cluster(_ptr(b.hit_xyz), _ptr(b.hit_idx), _ptr(b.hit_off), _ptr(b.mask_frame), b.M, b.idx_cap, c.origin, b.F,
                                          c.eps, c.min_points, c.pick, c.cl_off, c.cl_tile_off, c.cl_idx, c.cl_xyz, c.cl_status, c.ws,
                                          c.ws_bytes, st), "cm3d_depth_cluster")

    def stage_ground_strip(self, st):
        """The ground strip alone, on the sweep rows and the raw lists the last pass left resident (cm3d_ground_grid, cm3d_ground_strip:
        what the stripped pass enqueues between the compaction and the clustering)."""
        b, s = self.b, self.b.strip_desc
        cloud = b.points is not None
        check(self.lib.cm3d_ground_grid(_ptr(b.points) if cloud else None, _ptr(b.pt_off) if cloud else None, None if cloud else _ptr(b.raw),
                                        b.hb.raw_stride, _ptr(b.sweep_xf), _ptr(b.sweep_row_off), _ptr(b.frame_sweep_off), b.S, b.halfw, b.pt_cap,
                                        s.origin, b.F, s.cell, s.down, s.up, s.quantile, s.min_points, s.grid_z, s.grid_n, st),
              "cm3d_ground_grid")
        xyz, off, idx = self._seen_lists(b, "owner")      # (the exclusive lists when the engine decides ownership, else the raw ones)
        check(self.lib.cm3d_ground_strip(_ptr(xyz), _ptr(idx), _ptr(off), _ptr(b.mask_frame), b.M, b.idx_cap, s.origin,
                                         s.grid_z, b.F, s.cell, s.margin, s.min_keep, s.gs_off, s.gs_tile_off, s.gs_idx, s.gs_xyz, s.gs_status,
                                         s.gs_dropped, s.ws, s.ws_bytes, st), "cm3d_ground_strip")

    def stage_point_owner(self, st):
        """The point ownership alone, on the raw lists the last pass left resident (cm3d_point_owner: what the owned pass enqueues
        between the compaction and the ground strip)."""
        b, w = self.b, self.b.owner_desc
        check(self.lib.cm3d_point_owner(_ptr(b.hit_xyz), _ptr(b.hit_idx), _ptr(b.hit_off), _ptr(b.mask_off), b.F, b.M, b.idx_cap, b.max_pts,
                                        _ptr(b.score), w.rule, w.min_keep, w.ow_owner, w.ow_off, w.ow_tile_off, w.ow_idx, w.ow_xyz, w.ow_status,
                                        w.ow_lost, w.ws, w.ws_bytes, st), "cm3d_point_owner")

    def stage_yaw_fit(self, st):
        """The yaw fit's three launches alone, on what the last pass left resident (cm3d_yaw_fit_boxes: cm3d_bev_fit, cm3d_yaw_select,
        the box launch with the chosen yaws)."""
        check(self.lib.cm3d_yaw_fit_boxes(self.b.desc_ref, ctypes.byref(self.b.yaw_desc), st), "cm3d_yaw_fit_boxes")

    def stage_bev_fit(self, st):
        """cm3d_bev_fit alone, on the lists the yaw-fitted pass fits."""
        b, y = self.b, self.b.yaw_desc
        xyz, off = self.read_lists()
        check(self.lib.cm3d_bev_fit(_ptr(xyz), _ptr(off), b.M, b.idx_cap, y.angle_cs, y.K, y.d0,
                                    y.min_points, y.min_length, y.fit_k, y.fit_rect, y.fit_status, st), "cm3d_bev_fit")

    def stage_rotated_nms(self, st):
        """The opt-in rotated-box NMS on the box rows and flags the pass's (last) box launch wrote (cm3d_box_rotated_nms)."""
        b, n = self.b, self.b.nms_desc
        check(self.lib.cm3d_box_rotated_nms(_ptr(b.box), _ptr(b.flags), _ptr(b.mask_off), b.F, b.M, _ptr(b.class_id), _ptr(self.prior_wlh),
                                            _ptr(self.nms_group), len(self.classes.names), n.thr, n.n_thr, n.measure, n.class_agnostic,
                                            int(b.pose_inv is not None), self._mask_bound(b), st),
              "cm3d_box_rotated_nms")

    def stage_place(self, st):
        """cm3d_box_place alone, on the box rows, flags and rectangles the yaw-fitted pass left resident."""
        b, p = self.b, self.b.place_desc
        check(self.lib.cm3d_box_place(_ptr(b.box), _ptr(b.flags), _ptr(b.mask_off), b.F, b.M, _ptr(b.fit_rect), _ptr(b.yaw_src),
                                      _ptr(self.prior_wlh), _ptr(self.nms_group), _ptr(self.nms_thr), len(self.classes.names), _ptr(b.ego_xyz),
                                      int(b.pose_inv is not None), p.thin, self._mask_bound(b), p.place_src,
                                      p.place_pushed, st), "cm3d_box_place")

    def stage_velocity(self, st):
        """The opt-in velocity stage on the box rows and flags the pass (its rotated NMS included) left (cm3d_box_velocity)."""
        b, v = self.b, self.velocity
        check(self.lib.cm3d_box_velocity(_ptr(b.box), _ptr(b.flags), _ptr(b.mask_off), b.F, b.M, _ptr(b.class_id), _ptr(self.nms_group),
                                         _ptr(self.vel_speed), len(self.classes.names), self.vel_speed.numel(), _ptr(b.frame_next),
                                         _ptr(b.frame_time), v.max_dt, _ptr(b.vel_pair_off), b.F, b.vel_pairs, _ptr(b.next_match),
                                         _ptr(b.prev_match), _ptr(b.vel), _ptr(b.vel_src), _ptr(b.vel_status), _ptr(b.vel_ws),
                                         b.vel_ws_bytes, st), "cm3d_box_velocity")

    def stage_tracks(self, st):
        """The opt-in track stage on the matches the velocity stage left; rewrites scores and keep bits in place (cm3d_box_tracks)."""
        b, tr = self.b, self.tracks
        check(self.lib.cm3d_box_tracks(_ptr(b.box), _ptr(b.flags), _ptr(b.mask_frame), _ptr(b.next_match), _ptr(b.prev_match),
                                       _ptr(b.frame_time), b.M, b.F, tr.min_length, tr.score_mode, tr.smooth_window, _ptr(b.track_id),
                                       _ptr(b.track_pos), _ptr(b.track_len), _ptr(b.track_stat), _ptr(b.vel_smooth), _ptr(b.track_status),
                                       _ptr(b.track_ws), b.track_ws_bytes, st), "cm3d_box_tracks")

    def stage_size(self, st):
        """The opt-in size stage on the rectangles of the yaw fit, the placement's sources and the track stage's arrays; rewrites the
        centres of the sized boxes in place (cm3d_box_size)."""
        b, sz = self.b, self.size
        check(self.lib.cm3d_box_size(_ptr(b.box), _ptr(b.flags), _ptr(b.mask_frame), _ptr(b.fit_rect), _ptr(b.place_src), _ptr(self.prior_wlh),
                                     len(self.classes.names), _ptr(b.ego_xyz), 0, self.place.thin, _ptr(b.next_match), _ptr(b.prev_match),
                                     _ptr(b.track_id), _ptr(b.track_pos), _ptr(b.track_len), _ptr(b.frame_time), b.M, b.F, self.velocity.max_dt,
                                     self.tracks.smooth_window, sz.q, sz.min_obs, sz.lo, sz.hi, _ptr(b.size_wlh), _ptr(b.size_src),
                                     _ptr(b.size_ratio), _ptr(b.size_obs), _ptr(b.size_placed), _ptr(b.size_vel), _ptr(b.size_status),
                                     _ptr(b.size_ws), b.size_ws_bytes, st), "cm3d_box_size")

    def stage_vertical(self, st):
        """The opt-in vertical stage alone, on the lists and the box rows the last pass left resident (cm3d_box_vertical): the clustered
        lists when the engine clusters, else the stripped ones when it strips, the raw ones otherwise -- what stage_bev_fit fits."""
        b, v = self.b, self.vertical
        xyz, off = self.read_lists()
        check(self.lib.cm3d_box_vertical(_ptr(xyz), _ptr(off), b.M, b.idx_cap, _ptr(b.box), _ptr(b.flags), _ptr(self.prior_wlh),
                                         len(self.classes.names), v.q_bot, v.q_top, v.min_points, v.lo, v.hi, _ptr(b.vert_z), _ptr(b.vert_h),
                                         _ptr(b.vert_src), _ptr(b.vert_status), _ptr(b.vert_entry_z), st), "cm3d_box_vertical")

    def stage_virtual(self, st):
        """The opt-in virtual points alone, on the masks, the lists and the flags the last pass left resident (cm3d_hit_project, then
        cm3d_virtual_points): the lists stage_vertical reads."""
        b, v = self.b, self.virtual
        xyz, off = self.read_lists()
        check(self.lib.cm3d_hit_project(_ptr(xyz), _ptr(off), _ptr(b.mask_frame), _ptr(b.mask_cam), _ptr(b.cams), b.hb.n_cams, b.F, b.M,
                                        b.idx_cap, _ptr(b.hit_uvd), st), "cm3d_hit_project")
        check(self.lib.cm3d_virtual_points(_ptr(b.packed), _ptr(b.bbox), b.W, b.H, _ptr(b.cams), b.hb.n_cams, _ptr(b.mask_off),
                                           _ptr(b.mask_frame), _ptr(b.mask_cam), _ptr(b.flags), b.F, b.M, _ptr(b.hit_uvd), _ptr(off), b.idx_cap,
                                           v.per_mask, v.seed, v.max_px, int(v.kept_only), _ptr(b.frame_seed), _ptr(b.vp_count),
                                           _ptr(b.vp_status), _ptr(b.vp_xyz), _ptr(b.vp_pix), _ptr(b.vp_src), _ptr(b.vp_depth), _ptr(b.vp_d2),
                                           st), "cm3d_virtual_points")

    def stage_ground(self, st, zref=None):
        """The opt-in ground stage alone, on the sweep rows and the box rows the last pass left resident (cm3d_box_ground): the cloud where
        the engine has materialised it, the raw rows otherwise.  zref: None -- the reference heights are `vert_entry_z` with a vertical
        stage, else column 2 of `box` --, or a device tensor of M doubles (`ground_zref` itself: the stage again on what a pass left)."""
        b, g, v = self.b, self.ground, self.vertical is not None
        if zref is None and v:
            zref = b.vert_entry_z
        cloud = b.points is not None
        check(self.lib.cm3d_box_ground(_ptr(b.points) if cloud else None, _ptr(b.pt_off) if cloud else None, None if cloud else _ptr(b.raw),
                                       b.hb.raw_stride, _ptr(b.sweep_xf), _ptr(b.sweep_row_off), _ptr(b.frame_sweep_off), b.S, b.halfw, b.pt_cap,
                                       _ptr(b.mask_off), b.F, b.M, b.nm_max, _ptr(b.box), _ptr(b.flags), _ptr(self.prior_wlh),
                                       len(self.classes.names), None if zref is None else _ptr(zref), _ptr(b.vert_status) if v else None,
                                       _ptr(b.vert_z) if v else None, _ptr(b.vert_h) if v else None, g.radius, g.quantile, g.min_points,
                                       g.down, g.up, g.lo, g.hi, _ptr(b.ground_z), _ptr(b.ground_n), _ptr(b.ground_h), _ptr(b.ground_src),
                                       _ptr(b.ground_status), _ptr(b.ground_zref), st), "cm3d_box_ground")

    STAGES = ("sweeps", "masks", "project", "compact", "medoid", "lanes", "boxes")

    def _timed(self, stage, st, stage_events):
        """A stage's call behind the pass, between a new pair of events appended to stage_events when the pass is timed."""
        if stage_events is None:
            return stage(st)
        pair = [torch.cuda.Event(enable_timing=True) for _ in range(2)]
        stage_events.extend(pair)
        pair[0].record(torch.cuda.current_stream(self.dev))
        stage(st)
        pair[1].record(torch.cuda.current_stream(self.dev))

    def run(self, masks="dense", project_events=None, stage_events=None):
        """One pass of the hot path over the resident batch (asynchronous).  project_events: optional pair of
        torch.cuda.Event recorded around the projection launch on the launch stream (bench.py's roofline timing).
        stage_events: optional list; gets timing events appended, from which the entry points' timer buckets (reference :368-378)
        come, in this order:
          - five: before the point/mask stages, behind the compaction, the medoid, the lane search and the boxes;
          - then a pair around each opt-in stage the engine has, in the order of TIMED_ORDER:
              filter   the filter launch (the "drivable" bucket);
              owner    the point ownership's launches (the "owner" bucket; behind the second of the five, in front of the strip's);
              strip    the ground strip's launches (the "strip" bucket; behind the second of the five, in front of the clustering's);
              cluster  the clustering's launches (the "cluster" bucket; between the second and the third of the five);
              yaw      the yaw fit's two launches (the "yawfit" bucket; behind the fifth event);
              place    the placement's launch (the "place" bucket; behind the yaw fit's boxes);
          - then a pair around each of these calls behind the pass: the vertical stage's (the "vertical" bucket), the ground stage's
            (the "ground" bucket; behind the vertical stage's), the virtual points' (the "virtual points" bucket; last of all, behind
            the velocity, track and size stages' calls, which have no events).
        One library call enqueues the pass, opt-in stages included (cm3d_lift_pass_composed; include/cm3d_hip.h states the order); no
        allocation, no synchronisation."""
        dense = self.resident_masks(masks)               # raises before anything is enqueued
        if not self._lane["built"]:
            self.start_lane_grid()
        marks = omarks = None
        if stage_events is not None:
            marks = [torch.cuda.Event(enable_timing=True) for _ in range(5)]
            omarks = {name: [torch.cuda.Event(enable_timing=True) for _ in range(2)] for name in self.b.timed}
            stage_events.extend(marks + [ev for pair in omarks.values() for ev in pair])
        st = torch.cuda.current_stream(self.dev).cuda_stream
        desc = self.refresh_pass_descriptor(dense, project_events, marks, omarks)
        b = self.b
        check(self.lib.cm3d_lift_pass_composed(desc, b.opts_ref, b.place_ref, b.strip_ref, b.owner_ref, st), "cm3d_lift_pass_composed")

        if self.vertical is not None:                    # directly behind the pass: column 2 only, so the stages below see what they saw
            self._timed(self.stage_vertical, st, stage_events)
        if self.ground is not None:                      # behind the vertical stage's call: column 2 only, like it
            self._timed(self.stage_ground, st, stage_events)
        if self.velocity is not None:                    # behind the pass, on its final kept set: one more library call
            self.stage_velocity(st)
        if self.tracks is not None:                      # behind the velocity stage, on its matches: one more
            self.stage_tracks(st)
        if self.size is not None:                        # behind the track stage, on its tracks: one more
            self.stage_size(st)
        if self.virtual is not None:                     # behind everything that writes `flags`; it writes no box, flag or record
            self._timed(self.stage_virtual, st, stage_events)

    def capture_graph(self, masks="rle"):
        """Captures one pass over the resident batch into a HIP graph and returns it (`g.replay()` re-runs the pass
        on the resident buffers).  One graph launch replaces ~13 kernel launches, two event operations and the Python
        between them: what matters for small batches, where a pass is shorter than the time the host needs to enqueue
        it (a 256-frame batch is GPU-bound either way).  Call after at least one eager `run` (first-use attribute
        calls and stream creation must not happen during capture)."""
        torch.cuda.synchronize(self.dev)
        if self._lane is not None and self._lane["built"]:
            self._lane["done"] = True            # everything issued so far has completed, the lane index among it
        self.graph_captured = True
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g):
            self.run(masks=masks)
        return g

    def hit_chunk_rows(self) -> int:
        """Rows of the resident batch that lie in a 256-row block with at least one in-mask point after the last pass: the rows
        whose hit words the projection wrote and the compaction read (bench.py's byte accounting; synchronises the stream)."""
        b = self.b
        out = ctypes.c_int64(0)
        check(self.lib.cm3d_project_hit_rows(_ptr(b.pg_ws), b.pg_ws_bytes, b.F, b.max_pts, b.planes, ctypes.addressof(out),
                                             torch.cuda.current_stream(self.dev).cuda_stream), "cm3d_project_hit_rows")
        return int(out.value)

    def culling(self):
        """What the projection's per-frame tables decided for the resident batch in the last pass (cm3d_project_culling; an aid of
        the tests, synchronises the stream): dict of per-frame arrays -- `apx_ok`, `cam_has`, `wedge` (bit c = camera c), `margin_px`,
        `zmin` (float32)."""
        b = self.b
        out = np.zeros((b.F, 8), np.int32)
        check(self.lib.cm3d_project_culling(_ptr(b.pg_ws), b.pg_ws_bytes, b.F, b.max_pts, b.planes, out.ctypes.data,
                                            torch.cuda.current_stream(self.dev).cuda_stream), "cm3d_project_culling")
        return dict(apx_ok=out[:, 0].copy(), cam_has=out[:, 1].copy(), margin_px=out[:, 2].copy(),
                    zmin=out[:, 3].copy().view(np.float32), wedge=out[:, 4].copy())

    def wedges(self):
        """The view wedges the projection's per-frame tables hold for the resident batch after the last pass (cm3d_project_wedges; an
        aid of the tests, synchronises the stream): float32 [F, CM3D_MAX_CAMS, 8] -- unit normal and offset of the left plane, then
        of the right one; a global point p is looked at for camera c while min(n_L . p + d_L, n_R . p + d_R) >= 0."""
        b = self.b
        out = np.zeros((b.F, 8, 8), np.float32)
        check(self.lib.cm3d_project_wedges(_ptr(b.pg_ws), b.pg_ws_bytes, b.F, b.max_pts, b.planes, out.ctypes.data,
                                           torch.cuda.current_stream(self.dev).cuda_stream), "cm3d_project_wedges")
        return out

    # -- results
    def check_status(self):
        s = self.b.status.cpu().numpy()
        if self._lane is not None and self._lane["built"] and self._lane.get("passes_since_build", 0) > 0:
            self._lane["done"] = True        # a pass that waited for the build has completed
        if s[0] & 1:
            raise Cm3dError(f"point capacity overflow ({s[1]} > {self.b.pt_cap})")
        if s[0] & 2:
            raise Cm3dError(f"hit-index capacity overflow: {s[2]} indices needed, capacity {self.b.idx_cap}; "
                            "raise hits_per_point")
        if s[0] & 4:
            raise Cm3dError("a frame has too many masks or a cam_num is out of range")
        if s[0] & 8:
            raise Cm3dError("quad layout: a frame does not start on a multiple of 4 rows")
        if self.velocity is not None:
            v = int(self.b.vel_status.item())
            if v & 1:
                raise Cm3dError("velocity: a frame_next lies outside the batch")
            if v & 2:
                raise Cm3dError("velocity: pair_off disagrees with mask_off / frame_next, or a linked frame has too many masks")
        if self.tracks is not None:
            v = int(self.b.track_status.item())
            if v & 1:
                raise Cm3dError("tracks: a kept mask's frame lies outside the batch")
            if v & 2:
                raise Cm3dError("tracks: a next_match / prev_match lies outside the batch's masks")
            if v & 4:
                raise Cm3dError("tracks: a match is not mutual, not kept or not forward in time")
        if self.size is not None:
            v = int(self.b.size_status.item())
            if v & 1:
                raise Cm3dError("size: a track array or a match is not what the track stage writes")
            if v & 2:
                raise Cm3dError("size: a track is longer than the batch has frames")
        return s

    def removed_rows(self):
        """Boolean array over the batch's raw rows: True where the reference drops the row (ego box, :442-445).
        Decoded from the device's removed-row bits (frame f's bits start at word (pt_off[f] >> 5) + 8 f)."""
        b = self.b
        words = b.removed_bits.cpu().numpy().view(np.uint32)
        p_off = b.pt_off.cpu().numpy()
        out = np.zeros(int(p_off[-1]), bool)
        for f in range(b.F):
            p0, n = int(p_off[f]), int(p_off[f + 1] - p_off[f])
            if n <= 0:
                continue
            w0 = (p0 >> 5) + 8 * f
            bits = np.unpackbits(words[w0:w0 + (n + 31) // 32].view(np.uint8), bitorder="little")[:n]
            out[p0:p0 + n] = bits.astype(bool)
        return out

    def download(self, full=True):
        """Synchronises, checks the status word and returns numpy results.  full=False: only the per-mask results
        (boxes, flags, medoids, lane matches, list offsets) -- a few hundred KB.  `medoid_pos` is a position in the lists the medoid saw:
        the clustered ones (`cl_off`) when the engine clusters, else the stripped ones (`gs_off`) when it strips, else the exclusive ones (`ow_off`) when it decides ownership, else the raw ones.  full=True adds the index lists
        (`hit_idx`, the reference's track_points), the coordinates of the listed points (`hit_xyz`), `pt_off` in the
        reference's form (the aggregated cloud without the ego-box rows, :445-465) and -- when the engine keeps the cloud
        (keep_cloud) -- `points` in that form too; on the device the cloud keeps the dropped rows as NaN placeholders."""
        b = self.b
        s = self.check_status()
        if not full:
            out = dict(hit_off=b.hit_off.cpu().numpy(), medoid_pos=b.medoid_pos.cpu().numpy(), centroid=b.centroid.cpu().numpy(),
                       lane_idx=b.lane_idx.cpu().numpy(), lane_dist=b.lane_dist.cpu().numpy(),
                       centroid_global=b.centroid_g.cpu().numpy(), box=b.box.cpu().numpy(), flags=b.flags.cpu().numpy())
            if self.obb:
                out.update(obb_yaw=b.obb_yaw.cpu().numpy(), obb_status=b.obb_status.cpu().numpy())
            if self.cluster is not None:
                out.update(cl_off=b.cl_off.cpu().numpy(), cl_status=b.cl_status.cpu().numpy())
            if self.strip is not None:
                out.update(gs_off=b.gs_off.cpu().numpy(), gs_status=b.gs_status.cpu().numpy(), gs_dropped=b.gs_dropped.cpu().numpy())
            if self.owner is not None:
                out.update(ow_off=b.ow_off.cpu().numpy(), ow_status=b.ow_status.cpu().numpy(), ow_lost=b.ow_lost.cpu().numpy())
            if self.yaw is not None:
                out.update(self._yaw_results())
            if self.velocity is not None:
                out.update(self._velocity_results())
            if self.vertical is not None:
                out.update(self._vertical_results())
            if self.ground is not None:
                out.update(self._ground_results())
            if self.virtual is not None:
                out.update(self._virtual_results())
            return out
        n_rows, n_idx = int(s[1]), int(s[2])
        pt_off_rows = b.pt_off.cpu().numpy()
        keep = ~self.removed_rows()[:n_rows]
        if b.hb.frame_rows is not None:         # quad layout: a frame's padding rows are not rows of the reference's cloud
            for f in range(b.F):
                p0 = int(pt_off_rows[f])
                keep[p0 + int(b.hb.frame_rows[f]):int(pt_off_rows[f + 1])] = False
        kept_per_frame = np.add.reduceat(keep.astype(np.int64), pt_off_rows[:-1]) if n_rows else np.zeros(b.F, np.int64)
        kept_per_frame = np.where(np.diff(pt_off_rows) > 0, kept_per_frame, 0)
        out = dict(
            pt_off=np.concatenate([[0], np.cumsum(kept_per_frame)]).astype(np.int32),
            hit_off=b.hit_off.cpu().numpy(), hit_idx=b.hit_idx[:n_idx].cpu().numpy(), hit_xyz=b.hit_xyz[:n_idx].cpu().numpy(),
            bbox=b.bbox[:, :4].cpu().numpy(), medoid_pos=b.medoid_pos.cpu().numpy(), centroid=b.centroid.cpu().numpy(),
            lane_idx=b.lane_idx.cpu().numpy(), lane_dist=b.lane_dist.cpu().numpy(), centroid_global=b.centroid_g.cpu().numpy(),
            box=b.box.cpu().numpy(), flags=b.flags.cpu().numpy())
        if b.points is not None:
            out["points"] = b.points[:n_rows].cpu().numpy()[keep]
        if b.colsum is not None:
            out["colsum"] = b.colsum[:n_idx].cpu().numpy()
        if self.obb:
            out.update(obb_yaw=b.obb_yaw.cpu().numpy(), obb_status=b.obb_status.cpu().numpy())
        if self.filters is not None:
            out.update(on_road=b.on_road.cpu().numpy(), medoid_pos_kept=b.medoid_pos_kept.cpu().numpy())
        if self.cluster is not None:
            cl_off = b.cl_off.cpu().numpy()
            n_cl = int(cl_off[-1])
            out.update(cl_off=cl_off, cl_status=b.cl_status.cpu().numpy(), cl_idx=b.cl_idx[:n_cl].cpu().numpy(),
                       cl_xyz=b.cl_xyz[:n_cl].cpu().numpy())
        if self.strip is not None:
            gs_off = b.gs_off.cpu().numpy()
            n_gs = int(gs_off[-1])
            out.update(gs_off=gs_off, gs_status=b.gs_status.cpu().numpy(), gs_dropped=b.gs_dropped.cpu().numpy(),
                       gs_idx=b.gs_idx[:n_gs].cpu().numpy(), gs_xyz=b.gs_xyz[:n_gs].cpu().numpy(), grid_z=b.grid_z.cpu().numpy(),
                       grid_n=b.grid_n.cpu().numpy())
        if self.owner is not None:
            ow_off = b.ow_off.cpu().numpy()
            n_ow = int(ow_off[-1])
            out.update(ow_off=ow_off, ow_status=b.ow_status.cpu().numpy(), ow_lost=b.ow_lost.cpu().numpy(),
                       ow_owner=b.ow_owner[:n_idx].cpu().numpy(), ow_idx=b.ow_idx[:n_ow].cpu().numpy(), ow_xyz=b.ow_xyz[:n_ow].cpu().numpy())
        if self.yaw is not None:
            out.update(self._yaw_results())
        if self.velocity is not None:
            out.update(self._velocity_results())
        if self.vertical is not None:
            out.update(self._vertical_results())
        if self.ground is not None:
            out.update(self._ground_results())
        if self.virtual is not None:
            out.update(self._virtual_results())
            n_list = int(self.read_lists()[1][-1].item())
            out["hit_uvd"] = b.hit_uvd[:max(0, min(n_list, b.idx_cap))].cpu().numpy()
        return out

    def _virtual_results(self):
        return {k: getattr(self.b, k).cpu().numpy() for k in VIRTUAL_RESULTS}

    def _ground_results(self):
        return {k: getattr(self.b, k).cpu().numpy() for k in GROUND_RESULTS}

    def _vertical_results(self):
        return {k: getattr(self.b, k).cpu().numpy() for k in VERTICAL_RESULTS}

    def _velocity_results(self):
        b = self.b
        out = dict(vel=b.vel.cpu().numpy(), vel_src=b.vel_src.cpu().numpy(), next_match=b.next_match.cpu().numpy(),
                   prev_match=b.prev_match.cpu().numpy())
        if self.tracks is not None:
            out.update(track_id=b.track_id.cpu().numpy(), track_pos=b.track_pos.cpu().numpy(), track_len=b.track_len.cpu().numpy(),
                       track_stat=b.track_stat.cpu().numpy())
            if b.vel_smooth is not None:
                out["vel_smooth"] = b.vel_smooth.cpu().numpy()
        if self.size is not None:
            out.update({k: getattr(b, k).cpu().numpy() for k in ("size_wlh", "size_src", "size_ratio", "size_obs", "size_placed", "size_vel")})
        return out

    def _yaw_results(self):
        b = self.b
        out = dict(yaw_src=b.yaw_src.cpu().numpy(), fit_status=b.fit_status.cpu().numpy(), fit_k=b.fit_k.cpu().numpy(),
                   fit_rect=b.fit_rect.cpu().numpy())
        if self.place is not None:
            out.update(place_src=b.place_src.cpu().numpy(), place_pushed=b.place_pushed.cpu().numpy())
        return out


class LiftPipeline:
    """Keeps `depth` independent lift batches in flight: one LiftEngine (own device buffers) per slot, batches issued round-robin.
    Frames are independent, so consecutive batches of a job never wait for each other; a pass is a chain of ~12
    dependent launches whose tail (scans, lane search, boxes: a few hundred waves) leaves most of the 256 CUs idle, and the next
    batch's HBM-bound stages run there.

    Which stream a pass runs on is decided by the library (cm3d_pipe_*, csrc/pipe_sched.h): work of streams that share a hardware queue
    runs in order, so no more streams execute passes than the process has queues for -- min(depth, 4, GPU_MAX_HW_QUEUES - 1), the
    variable read, never set; 4 queues when it is unset.  With that many streams or more than slots, slot s runs on `streams[s]` as
    it always did.  With fewer, pass number k runs on `streams[k % n]`, the slots take turns, and a slot's event keeps two passes of
    one slot in order when they land on different streams ("Passes rotate over as many streams as the process has queues
    for").  Where that count stops at the queues, the plan adds one executor that is no stream of the pipeline's: the legacy null stream,
    whose queue carries nothing while passes run (cm3d_pipe_create2).  An index from `last_stream` names an
    executor; `exec_stream` maps it to a torch stream (the null executor: the device's default stream), and `streams` stay the slots' own
    (uploads by hand, captures).  The null stream waits for every blocking stream of the process, so every stream here is non-blocking
    (torch's are).  `null_exec` True / False asks for / forbids the null executor; CM3D_PIPE_NULL_EXEC=0 forbids it where nothing is asked.
    `exec_streams` overrides the policy (tests; no null executor unless asked for).  Every pass is enqueued by one library call (cm3d_lift_pass[_opt]): `submit`, a
    `rerun` that has to start the build of the lane index and every pass of engines with opt-in stages go through `LiftEngine.run` on the
    chosen stream, every other `rerun` hands the slot's descriptor to cm3d_pipe_submit, which picks the stream itself.

    Rule for callers that use `streams[slot]` or `engines[slot]` directly (an upload, a pass stage by stage, a graph capture): the device
    must be idle before and after -- `torch.cuda.synchronize()` on both sides --, because the slot's last pass need not have run on
    `streams[slot]`.  Once an engine of the pipeline has captured a graph the pipeline stops rotating for good: the graph replays on the
    stream it was captured on, so slot s stays on `streams[s]`.  `submit` needs the slot collected (`collect`, `collect_records`,
    `check_status`) before it comes round again: the buffers it replaces may be in use on another stream until then."""

    def __init__(self, device="cuda:0", depth=3, exec_streams=None, null_exec=None, **engine_kw):
        if depth < 1:
            raise ValueError("depth >= 1")
        self.dev = torch.device(device)
        shared = {}                                          # one cache of lane tables + indices for all slots
        self.engines = [LiftEngine(device, lane_cache=shared, **engine_kw) for _ in range(depth)]
        self.streams = [torch.cuda.Stream(device=self.dev) for _ in range(depth)]
        self.masks = [None] * depth
        self.uploaded = [torch.cuda.Event() for _ in range(depth)]      # recorded behind a slot's H2D copies (submit)
        self._next = 0
        self.native_passes = 0                               # passes enqueued by cm3d_lift_pass
        self._pinned = False
        L = self.lib = self.engines[0].lib
        handles = (ctypes.c_void_p * depth)(*[s.cuda_stream for s in self.streams])
        with torch.cuda.device(self.dev):
            self._h = L.cm3d_pipe_create2(depth, int(exec_streams or 0), handles, -1 if null_exec is None else int(bool(null_exec)))
        if not self._h:
            raise Cm3dError("cm3d_pipe_create2 failed")
        self.exec_streams = int(L.cm3d_pipe_exec_streams(self._h))
        self._null = torch.cuda.default_stream(self.dev)     # what the null executor's index means (exec_stream)
        # With batches executing side by side the projection launch leaves part of the chip to the other batches' kernels (two workgroups
        # per CU instead of three, one with four streams executing: cm3d_project_workgroups_per_cu -- process-wide, results unaffected):
        # +1-2 % frames/s at three, +4 % at four, while one batch at a time runs fastest with the launch filling the chip.  It follows the
        # streams that execute, not the slots.  CM3D_PIPE_WG_PER_CU overrides (0: never ask).
        want = int(os.environ.get("CM3D_PIPE_WG_PER_CU", "1" if self.exec_streams >= 4 else "2"))
        if self.exec_streams >= 2 and want > 0:
            L.cm3d_project_workgroups_per_cu(want)
        elif self.exec_streams == 1:
            L.cm3d_project_workgroups_per_cu(0)

    def __del__(self):
        h, self._h = getattr(self, "_h", None), None
        if h:
            self.lib.cm3d_pipe_destroy(h)

    @property
    def depth(self):
        return len(self.engines)

    def last_stream(self, slot):
        """Executor index of the slot's last pass (-1 before the first): `exec_stream` gives the torch stream."""
        return int(self.lib.cm3d_pipe_last_stream(self._h, slot))

    @property
    def null_exec(self):
        """The executor index that is the null stream, -1: none (cm3d_pipe_null_exec)."""
        return int(self.lib.cm3d_pipe_null_exec(self._h))

    def exec_stream(self, idx):
        """The torch stream of an executor index (`last_stream`, cm3d_pipe_acquire / _submit): `streams[idx]`, but the device's default
        stream for the null executor."""
        return self._null if idx == self.null_exec else self.streams[idx]

    def _pin_if_captured(self):
        if not self._pinned and any(e.graph_captured for e in self.engines):
            self.lib.cm3d_pipe_pin(self._h)
            self._pinned = True

    def _acquire(self, slot):
        """The stream of the slot's next pass, ordered behind the slot's previous one."""
        idx = self.lib.cm3d_pipe_acquire(self._h, slot)
        if idx < 0:
            check(idx, "cm3d_pipe_acquire")
        return idx

    def _wait(self, slot):
        check(self.lib.cm3d_pipe_wait(self._h, slot), "cm3d_pipe_wait")
        idx = self.last_stream(slot)
        return self.exec_stream(idx if idx >= 0 else slot)

    def submit(self, hb: HostBatch, masks="rle", stage_events=None):
        """Uploads `hb` into the next slot and issues one pass over it on the stream chosen for it (asynchronous).
        Returns the slot; `collect(slot)` must be called before the slot comes round again."""
        slot = self._next
        self._next = (slot + 1) % self.depth
        eng = self.engines[slot]
        self._pin_if_captured()
        st = self.exec_stream(self._acquire(slot))
        try:
            with torch.cuda.stream(st):
                eng.upload(hb)
                self.uploaded[slot].record(st)
                if masks == "dense":
                    eng.decode_masks_dense()
                eng.run(masks=masks, stage_events=stage_events)
        finally:
            self.lib.cm3d_pipe_release(self._h, slot)
        self.native_passes += 1
        self.masks[slot] = masks
        return slot

    def rerun(self, slot, masks=None, project_events=None, stage_events=None):
        """Another pass over the batch resident in `slot` (benchmarks).  stage_events: as LiftEngine.run's; the pass then takes the
        Python branch, which creates and appends them."""
        eng = self.engines[slot]
        mode = masks or self.masks[slot]
        self._pin_if_captured()
        if eng._lane["built"] and eng.b.plain_pass and stage_events is None:     # (cm3d_pipe_submit knows only the plain pass)
            # (no stream context, no Python between the launches: what bench.py's headline times.  A pair of events around the
            # projection kernel rides along, so that a timed pass costs the host what an untimed one does)
            rc = self.lib.cm3d_pipe_submit(self._h, slot, eng.refresh_pass_descriptor(eng.resident_masks(mode), project_events))
            if rc < 0:
                check(rc, "cm3d_pipe_submit")
        else:                                # the pass has to start the build of the lane index first, or has opt-in stages: LiftEngine.run's to do
            st = self.exec_stream(self._acquire(slot))
            try:
                with torch.cuda.stream(st):
                    eng.run(masks=mode, project_events=project_events, stage_events=stage_events)
            finally:
                self.lib.cm3d_pipe_release(self._h, slot)
        self.native_passes += 1

    def check_status(self, slot):
        """Waits for the slot's last pass and checks its status word."""
        with torch.cuda.stream(self._wait(slot)):
            return self.engines[slot].check_status()

    def collect_records(self, slot, frame_ids):
        """Waits for the slot's last pass, checks the status word and returns the slot's kept-box records as a DEVICE tensor
        (kept_box_records): what an entry point hands to the end-of-job gather -- nothing else is downloaded."""
        st = self._wait(slot)
        eng = self.engines[slot]
        eng.check_status()
        with torch.cuda.stream(st):
            rec = kept_box_records(eng.b, frame_ids, self.dev)
        st.synchronize()
        return rec

    def collect(self, slot, full=True):
        """Waits for the slot's last pass only and returns (host batch, numpy results); full=False: per-mask results only
        (LiftEngine.download)."""
        st = self._wait(slot)
        eng = self.engines[slot]
        with torch.cuda.stream(st):
            res = eng.download(full=full)
        return eng.b.hb, res


REC_FRAME_A, REC_FRAME_B = 5, 6       # columns of a shipped record that carry the frame's identity (see kept_box_records)


def kept_box_records(b, frame_ids, device=None):
    """The fixed-size records the multi-GPU gather ships: one row of CM3D_BOX_STRIDE doubles per box that
    survives NMS, in (frame, mask) order.  Columns 0-4, 7-9 are cm3d_box_nms's (centre, rotation, score, class, flags);
    columns 5 and 6 -- lane yaw and distance, which no output file contains -- are overwritten with the frame's identity
    frame_ids[f] = (a, b) (nuScenes: global sample index, 0; Waymo: scene index, frame number), so that rank 0 can rebuild
    every output record from the gathered rows and the job's deterministic frame order alone."""
    device = device or b.box.device
    keep = (b.flags & 3) == 3
    rec = b.box[keep].clone()
    ids = torch.as_tensor(np.ascontiguousarray(frame_ids, np.float64).reshape(-1, 2), device=device)
    fr = b.mask_frame[keep].long()
    rec[:, REC_FRAME_A] = ids[fr, 0]
    rec[:, REC_FRAME_B] = ids[fr, 1]
    return rec


def kept_box_velocities(b):
    """(k, 2) float64 velocities of the masks kept_box_records ships, in its order (an engine with Velocity(...); a device tensor).
    With Tracks(smooth_window > 0): the rows of `vel_smooth`, the slope over the track's window, in place of the neighbours' difference.
    With BoxSize(...): the rows of `size_vel`, the same rule on the sized centres."""
    vel = getattr(b, "size_vel", None)
    if vel is None:
        vel = getattr(b, "vel_smooth", None)
    return (b.vel if vel is None else vel)[(b.flags & 3) == 3].clone()


def virtual_point_frames(eng):
    """The virtual points of the batch resident in `eng` (an engine with VirtualPoints(...), its pass finished), frame by frame: a list
    of F entries, each the dict virtualpoints.frame_records makes -- xyz, pixel, cam, mask, class_id, src_idx (the winner's index in the
    frame's cloud, the reference's track_points numbering), score, depth -- or None for a frame without a point."""
    from . import virtualpoints as vpmod
    b = eng.b
    res = eng._virtual_results()
    off = eng.read_lists()[1].cpu().numpy()
    idx = eng._seen_lists()[2][:max(0, min(int(off[-1]), b.idx_cap))]
    idx, hb = idx.cpu().numpy(), b.hb
    return [vpmod.frame_records(res, f, eng.virtual.per_mask, hb.mask_off, hb.mask_cam, hb.class_id, hb.score, off, idx) for f in range(b.F)]


def point_label_frames(eng):
    """The painted cloud of the batch resident in `eng` (an engine with PointOwner(...), its pass and every stage behind it finished),
    frame by frame: a list of F entries, each the dict pointowner.label_rows makes -- idx, xyz, mask, cam, class_id, score, kept, claims,
    one row per listed point of the frame -- or None for a frame without a listed point.  From `ow_owner` and the raw lists, on the host."""
    from . import pointowner as pomod
    b = eng.b
    hb = b.hb
    off = b.hit_off.cpu().numpy()
    n = max(0, min(int(off[-1]), b.idx_cap))
    idx, xyz, own, flags = b.hit_idx[:n].cpu().numpy(), b.hit_xyz[:n].cpu().numpy(), b.ow_owner[:n].cpu().numpy(), b.flags.cpu().numpy()
    out = []
    for f in range(b.F):
        rows = pomod.label_rows(f, idx, xyz, off, hb.mask_off, own, hb.mask_cam, hb.class_id, hb.score, flags, b.max_pts)
        out.append(rows if len(rows["idx"]) else None)
    return out


def kept_box_sizes(b):
    """(k, 3) float64 [w, l, h] of the masks kept_box_records ships, in its order (an engine with BoxSize(...) or BoxVertical(...); a
    device tensor).  With BoxVertical(...) column 2 is `vert_h`, with BoxGround(...) it is `ground_h` (which carries `vert_h` where the
    ground stage left the box alone), and columns 0 and 1 are the size stage's where the engine has one, else the class's prior (the
    class as cm3d_box_place reads it from column 8 of the box)."""
    keep = (b.flags & 3) == 3
    height, size_wlh = getattr(b, "ground_h", getattr(b, "vert_h", None)), getattr(b, "size_wlh", None)
    if height is None:
        return size_wlh[keep].clone()
    if size_wlh is not None:
        rows = size_wlh[keep].clone()
    else:
        b8 = b.box[keep, 8]
        cls = torch.where((b8 >= 0.0) & (b8 < float(b.prior_wlh.shape[0])), b8, torch.zeros_like(b8)).long()
        rows = b.prior_wlh[cls].clone()
    rows[:, 2] = height[keep]
    return rows


def _size_rows(size, n):
    """The optional `size` of the writers: None, or (n, 3) float64 [w, l, h] rows beside the n records (kept_box_sizes)."""
    if size is None:
        return None
    size = np.ascontiguousarray(size, np.float64).reshape(-1, 3)
    if size.shape[0] != n:
        raise ValueError(f"size: {size.shape[0]} rows for {n} records")
    return size


def _velocity_rows(vel, n):
    """The optional `vel` of the writers: None, or (n, 2) float64 rows beside the n records (kept_box_velocities)."""
    if vel is None:
        return None
    vel = np.ascontiguousarray(vel, np.float64).reshape(-1, 2)
    if vel.shape[0] != n:
        raise ValueError(f"vel: {vel.shape[0]} rows for {n} records")
    return vel


def nuscenes_boxes_from_records(rec, tokens, classes: Optional[ClassTable] = None, vel=None, size=None):
    """Gathered records (numpy (k, 10), see kept_box_records) -> the reference's per-sample box dict lists (:808-817 after NMS
    :913-924): {sample_token: [box, ...]} with every token of `tokens` present ([] when a sample has no box, :845).
    vel: None -- "velocity": [0, 0], the reference's constant --, or the records' (k, 2) velocities (kept_box_velocities): [vx, vy].
    size: None -- "size": the class's prior --, or the records' (k, 3) [w, l, h] rows (kept_box_sizes)."""
    classes = classes or ClassTable.nuscenes()
    results = {t: [] for t in tokens}
    # plain Python floats / ints in one go (tolist), per-class constants built once: the loop below only assembles dicts
    rows = np.asarray(rec, np.float64).reshape(-1, _lib.BOX_STRIDE).tolist()
    vel = _velocity_rows(vel, len(rows))
    vels = vel.tolist() if vel is not None else None
    size = _size_rows(size, len(rows))
    own = size.tolist() if size is not None else None
    sizes = [[float(v) for v in wlh] for wlh in classes.prior_wlh]
    for k, r in enumerate(rows):
        token, ci = tokens[int(r[REC_FRAME_A])], int(r[8])
        name = classes.names[ci]
        results[token].append({
            "sample_token": token,
            "translation": [r[0], r[1], r[2]],
            "size": list(sizes[ci]) if own is None else own[k],
            "rotation": [r[3], 0.0, 0.0, r[4]],
            "velocity": [0, 0] if vels is None else vels[k],
            "detection_name": name,
            "detection_score": r[7],
            "attribute_name": ATTRIBUTE_NAMES[name],
        })
    return results


def nuscenes_results_json(rec, tokens, classes: Optional[ClassTable] = None, meta=None, vel=None, size=None):
    """The text json.dumps({"meta": meta, "results": nuscenes_boxes_from_records(rec, tokens, classes, vel, size)}) produces, written out
    directly from the records: same keys, key order, separators and float repr -- the writer of the reference (:929-930) without
    60 000 dicts and a generic encoder in between (tests/test_host_logic.py holds the two against each other)."""
    import json
    classes = classes or ClassTable.nuscenes()
    rows = np.asarray(rec, np.float64).reshape(-1, _lib.BOX_STRIDE).tolist()
    vel = _velocity_rows(vel, len(rows))
    vels = vel.tolist() if vel is not None else None
    own = _size_rows(size, len(rows))
    own = own.tolist() if own is not None else None
    tok_js = [json.dumps(t) for t in tokens]
    # everything of a box that only depends on its class, rendered once
    tail = []
    for ci, name in enumerate(classes.names):
        size = json.dumps([float(v) for v in classes.prior_wlh[ci]])
        tail.append((size, f'"detection_name": {json.dumps(name)}, "detection_score": ',
                     f', "attribute_name": {json.dumps(ATTRIBUTE_NAMES[name])}}}'))
    per = [[] for _ in tokens]
    from math import isfinite

    def fr(x):                      # json's float text: repr, but Infinity / -Infinity / NaN for what repr calls inf / nan
        return float.__repr__(x) if isfinite(x) else json.dumps(x)
    for k, r in enumerate(rows):
        ti, ci = int(r[REC_FRAME_A]), int(r[8])
        size, mid, end = tail[ci]
        if own is not None:
            size = f'[{fr(own[k][0])}, {fr(own[k][1])}, {fr(own[k][2])}]'
        x, y, z, qw, qz, sc = r[0], r[1], r[2], r[3], r[4], r[7]
        velocity = '"velocity": [0, 0], ' if vels is None else f'"velocity": [{fr(vels[k][0])}, {fr(vels[k][1])}], '
        if isfinite(x + y + z + qw + qz + sc):          # (a sum that overflows only sends a finite row down the careful branch)
            per[ti].append(f'{{"sample_token": {tok_js[ti]}, "translation": [{x!r}, {y!r}, {z!r}], "size": {size}, '
                           f'"rotation": [{qw!r}, 0.0, 0.0, {qz!r}], {velocity}{mid}{sc!r}{end}')
        else:
            per[ti].append(f'{{"sample_token": {tok_js[ti]}, "translation": [{fr(x)}, {fr(y)}, {fr(z)}], "size": {size}, '
                           f'"rotation": [{fr(qw)}, 0.0, 0.0, {fr(qz)}], {velocity}{mid}{fr(sc)}{end}')
    body = ", ".join(f'{tok_js[i]}: [{", ".join(b)}]' for i, b in enumerate(per))
    return f'{{"meta": {json.dumps(meta if meta is not None else {})}, "results": {{{body}}}}}', sum(len(b) for b in per)


def nuscenes_results_json_native(rec, tokens, classes: Optional[ClassTable] = None, meta=None, part=None, vel=None, size=None) -> bytes:
    """nuscenes_results_json through the native writer (libcm3d_reader.so, cm3d_write_results_json): the same bytes
    (tests/test_reader.py), without a Python statement per box -- 60 000 boxes take milliseconds instead of a third of a second.
    part = (first, count): only the entries of tokens[first:first+count] (records whose column 5 lies in that range), without the
    file's head and tail -- the entry point formats every batch's share while the later batches are still on the GPU and joins
    the parts with ", " between nuscenes_results_json_head(meta) and b"}}".
    vel: None, or the (k, 2) velocities of the k records (of the part's records, with `part`): written by the entry point beside
    cm3d_write_results_json that takes them (cm3d_write_results_json_vel).
    size: None, or the (k, 3) [w, l, h] rows of the k records (of the part's records, with `part`): written by
    cm3d_write_results_json_sized (include/cm3d_reader_size.h) in place of the class's prior."""
    import json
    from . import reader as rdmod
    classes = classes or ClassTable.nuscenes()
    vel = _velocity_rows(vel, np.asarray(rec).reshape(-1, _lib.BOX_STRIDE).shape[0])
    size = _size_rows(size, np.asarray(rec).reshape(-1, _lib.BOX_STRIDE).shape[0])
    mid, score, tail = [], [], []
    for ci, name in enumerate(classes.names):
        prior = json.dumps([float(v) for v in classes.prior_wlh[ci]])
        mid.append(f'], "size": {prior}, "rotation": [')
        # (with velocities the writer itself puts '], "velocity": [vx, vy' in front of this piece)
        score.append(('], "velocity": [0, 0' if vel is None else '') + f'], "detection_name": {json.dumps(name)}, "detection_score": ')
        tail.append(f', "attribute_name": {json.dumps(ATTRIBUTE_NAMES[name])}}}')
    prefix = nuscenes_results_json_head(meta).decode()
    if part is not None:
        first, count = part
        rec = np.array(rec, np.float64).reshape(-1, _lib.BOX_STRIDE)
        rec[:, REC_FRAME_A] -= first
        tokens, prefix = tokens[first:first + count], None
    return rdmod.write_results_json(rec, [json.dumps(t) for t in tokens], mid, score, tail, prefix, vel=vel, size=size)


def nuscenes_results_json_head(meta=None) -> bytes:
    import json
    return f'{{"meta": {json.dumps(meta if meta is not None else {})}, "results": {{'.encode()


def box_records(hb: HostBatch, res: dict, classes: Optional[ClassTable] = None):
    """Device results -> the reference's per-sample box dict lists (:808-817, after NMS :913-924).
    Every sample keeps its key; a sample without boxes maps to [] (:845 runs before the `continue` at :896)."""
    classes = classes or ClassTable.nuscenes()
    results = {}
    for f, token in enumerate(hb.tokens):
        boxes = []
        for m in range(hb.mask_off[f], hb.mask_off[f + 1]):
            if (res["flags"][m] & 3) != 3:
                continue
            name = classes.names[hb.class_id[m]]
            bx = res["box"][m]
            boxes.append({
                "sample_token": token,
                "translation": [float(bx[0]), float(bx[1]), float(bx[2])],
                "size": [float(v) for v in classes.prior_wlh[hb.class_id[m]]],
                "rotation": [float(bx[3]), 0.0, 0.0, float(bx[4])],
                "velocity": [0, 0],
                "detection_name": name,
                "detection_score": float(hb.score[m]),
                "attribute_name": ATTRIBUTE_NAMES[name],
            })
        results[token] = boxes
    return results
