"""nuScenes entry point of the lifting path: what `python 2d_to_3d.py` does in the reference
(src/nuscenes/2d_to_3d.py:343-938), with the per-frame work on the GPU.

Zero-argument invocation uses the reference's module constants (:55-59) and split (`mini_val`, :387);
everything is overridable by flags / environment for tests and other splits.  Under
`torch.distributed.run` scenes are sharded over the ranks and rank 0 writes the single output file
after one gather of box records.
"""
import argparse
import contextlib
import json
import os
import time
from dataclasses import dataclass, replace
from typing import List, Optional

import numpy as np
import torch

from . import cluster as clmod
from . import nms as nmsmod
from . import bevfit
from . import boxplace
from . import dist as cdist
from . import lifting, nusc_io
from . import velocity as velmod
from . import tracks as trmod
from . import boxsize as szmod
from . import boxvertical as vtmod
from . import boxground as grmod
from . import groundstrip as gsmod
from . import pointowner as pomod
from . import virtualpoints as vpmod

# module constants of the reference (:55-59)
VER_NAME = "v1.0-trainval"
INPUT_PATH = "../../data/nuScenes/"
OUTPUT_DIR = "../../outputs/nuscenes/"
INPUT_DIR = "../../mask_outputs/nuscenes-detic/"
MINI_VAL = ["scene-0103", "scene-0916"]          # nuscenes.utils.splits.mini_val (:43,:387)
OUTPUT_NAME = "pseudolabels_minival.json"        # :929

META = {"use_camera": True, "use_lidar": False, "use_radar": False, "use_map": True, "use_external": False}   # :357-364


def _load_priors(path):
    if os.path.exists(path):
        with open(path) as f:
            return json.load(f)            # cfg/shape_priors_chatgpt.json (:385)
    return dict(lifting.SHAPE_PRIORS_CHATGPT)


_WORKER_TABLES = {}
_WORKER_READER = None


@dataclass
class BatchTask:
    """What prepare_scene_batch is to prepare: the scenes of one batch, and how to read them (no reader named: the per-frame Python
    reader).  Picklable: reader processes get it under spawn."""
    version: str
    dataroot: str
    mask_dir: str
    names: List[str]
    n_sweeps: int = 3
    ratio: float = 0.64
    missing_ok: bool = False
    priors: Optional[dict] = None
    through_shm: bool = False                      # a reader process: the sweeps (nearly all of the bytes) go through shared memory
    reader_threads: Optional[int] = None           # a reader process: threads of the native loader it creates, once, for itself
    reader: Optional["reader.Reader"] = None       # a caller in this process: the native loader to use
    drivable: bool = False                         # --drivable-filter: the batches carry their maps' drivable-area polygons


_POLYGONS = {}


def drivable_polygons(dataroot, location):
    """The drivable-area polygons of a map location (eval_detection.load_drivable_polygons), loaded once per process."""
    key = (dataroot, location)
    if key not in _POLYGONS:
        from . import eval_detection
        _POLYGONS[key] = eval_detection.load_drivable_polygons(dataroot, location)
    return _POLYGONS[key]


def _attach_polygons(hb, dataroot, locations):
    """The polygon tables of a batch whose lane table k is that of locations[k] (the --drivable-filter route)."""
    hb.polygons = [drivable_polygons(dataroot, loc) for loc in locations]
    hb.polygon_key = (dataroot, tuple(locations))


def _batch_manifest(tables, names, mask_dir, n_sweeps, ratio, missing_ok):
    """The table walk of one batch of scenes (no bulk data): frame manifests, lane tables, lane table of every frame."""
    man, lanes, frame_lane = [], [], []
    for k, name in enumerate(names):
        scene = tables.scene_by_name(name)
        ms = nusc_io.scene_manifest(tables, scene, mask_dir, n_sweeps=n_sweeps, ratio=ratio, missing_ok=missing_ok)
        lanes.append(nusc_io.load_lane_points(tables.dataroot, tables.location(scene)))
        man.extend(ms)
        frame_lane.extend([k] * len(ms))
    return man, lanes, frame_lane


def prepare_scene_batch(task: BatchTask):
    """Host side of one batch of scenes: reads the frames' files, decodes the RLE strings and packs one HostBatch per mask
    size.  Pure numpy -- never touches the GPU -- so `lift_scenes(workers=N)` can run it in N reader processes.
    Returns (sample tokens in order, [HostBatch, ...], seconds spent)."""
    from multiprocessing import shared_memory
    t0 = time.time()
    key = (task.version, task.dataroot)
    if key not in _WORKER_TABLES:
        _WORKER_TABLES[key] = nusc_io.NuscTables(task.version, task.dataroot, annotations=False)
    tables = _WORKER_TABLES[key]
    classes = lifting.ClassTable.nuscenes(task.priors)
    native = task.reader
    if task.reader_threads is not None:    # a reader process: its own loader with that many threads, created once
        global _WORKER_READER
        if _WORKER_READER is None or _WORKER_READER[0] != task.reader_threads:
            from . import reader as rdmod
            _WORKER_READER = (task.reader_threads, rdmod.Reader(task.reader_threads, pinned=False))
        native = _WORKER_READER[1]
    if native is not None:
        # the native loader (libcm3d_reader.so): this thread only walks the tables and the small json files; sweeps and mask
        # pickles of the whole batch are read and parsed by the loader's thread pool, into page-locked staging buffers
        man, lanes, frame_lane = _batch_manifest(tables, task.names, task.mask_dir, task.n_sweeps, task.ratio, task.missing_ok)
        segs = []

        def shm_alloc(n_floats):                # the sweeps go straight from the page cache into the segment the parent maps
            shm = shared_memory.SharedMemory(create=True, size=max(4 * int(n_floats), 16))
            segs.append(shm)
            return np.ndarray((int(n_floats),), np.float32, buffer=shm.buf)
        try:
            hb, _ = lifting.pack_manifest(man, lanes, frame_lane, classes, native, alloc=shm_alloc if task.through_shm else None)
            if task.drivable and hb is not None:
                _attach_polygons(hb, tables.dataroot, [tables.location(tables.scene_by_name(n)) for n in task.names])
            if task.through_shm and hb is not None:
                hb.raw_shm, hb.raw = (segs[-1].name, hb.raw.shape), None
                for shm in segs[:-1]:              # a repack after dropping mask-less frames allocated twice
                    shm.close(); shm.unlink()
                segs[-1].close()
            return [m.token for m in man], ([hb] if hb is not None else []), time.time() - t0
        except lifting.BatchDeclined:
            pass                      # the Python reader below takes the batch
    frames, lanes, frame_lane = [], [], []
    for k, name in enumerate(task.names):
        scene = tables.scene_by_name(name)
        fs = nusc_io.frames_of_scene(tables, scene, task.mask_dir, n_sweeps=task.n_sweeps, ratio=task.ratio, missing_ok=task.missing_ok)
        lanes.append(nusc_io.load_lane_points(tables.dataroot, tables.location(scene)))
        frames.extend(fs)
        frame_lane.extend([k] * len(fs))
    tokens = [f.token for f in frames]
    live = [i for i, f in enumerate(frames) if len(f.rles) > 0]
    batches = []
    # one engine call per mask size (all cameras of nuScenes share one)
    for (W, H) in sorted({(frames[i].width, frames[i].height) for i in live}):
        sel = [i for i in live if (frames[i].width, frames[i].height) == (W, H)]
        batches.append(lifting.pack_frames([frames[i] for i in sel], lanes, [frame_lane[i] for i in sel], classes))
        if task.drivable:
            _attach_polygons(batches[-1], tables.dataroot, [tables.location(tables.scene_by_name(n)) for n in task.names])
    if task.through_shm:
        for hb in batches:
            shm = shared_memory.SharedMemory(create=True, size=max(hb.raw.nbytes, 16))
            np.ndarray(hb.raw.shape, np.float32, buffer=shm.buf)[...] = hb.raw
            hb.raw_shm, hb.raw = (shm.name, hb.raw.shape), None
            shm.close()
    return tokens, batches, time.time() - t0


def _attach_raw(hb, keep):
    """Maps the shared-memory sweeps a reader process left behind (zero copy); `keep` collects the segments until the
    batch has been uploaded."""
    if hb.raw_shm is not None:
        from multiprocessing import shared_memory
        name, shape = hb.raw_shm
        shm = shared_memory.SharedMemory(name=name)
        keep.append(shm)
        hb.raw, hb.raw_shm = np.ndarray(shape, np.float32, buffer=shm.buf), None


def _release(keep):
    for shm in keep:
        try:
            shm.close()
            shm.unlink()
        except (FileNotFoundError, BufferError):
            pass
    keep.clear()


def _ahead(it, depth=1):
    """Iterates `it` in a background thread, `depth` items ahead.  The native loader releases the interpreter lock while its
    threads read, so the Python half of the next batch (table walk, packing) runs under the file reads of this one."""
    import queue
    import threading
    q = queue.Queue(maxsize=depth)
    end = object()

    def work():
        try:
            for x in it:
                q.put(x)
            q.put(end)
        except BaseException as exc:       # handed to the consumer
            q.put(exc)
    threading.Thread(target=work, daemon=True).start()
    while True:
        x = q.get()
        if x is end:
            return
        if isinstance(x, BaseException):
            raise x
        yield x


def sample_tokens(tables, scene_names):
    """The job's sample tokens in output order (scenes in the given order, samples in scene order): every rank derives the
    same list from the tables alone, so a shipped record only needs its index into it."""
    return [s["token"] for name in scene_names for s in tables.samples_of_scene(tables.scene_by_name(name))]


REFERENCE_BUCKETS = ("io", "points in mask", "medoid", "drivable", "closest lane", "nms")       # the reference's timer (:368-378)


def _token_batches(batches, index, host_s):
    """The batches of one prepared task as _lift_batches takes them, frame ids = index[token]; the task's host time rides on the
    first of them (on an empty item when the task has no frame with a mask)."""
    for hb in batches or [None]:
        yield hb, None if hb is None else np.array([[index[t], 0] for t in hb.tokens], np.float64), host_s
        host_s = 0.0


def _lift_batches(prepared, device, classes, masks, timer, on_records=None, filters=None, cluster=None, nms=None, yaw=None,
                  velocity=None, vel_out=None, tracks=None, place=None, size=None, size_out=None, vertical=None, ground=None, strip=None,
                  virtual=None, owner=None, labels=None):
    """The submit / drain loop of both routes.  prepared yields (HostBatch, frame ids (F, 2), seconds the host spent preparing it); two
    batches are in flight on the GPU: batch i+1 is uploaded while batch i runs.  Returns the kept-box records of all batches as ONE
    device tensor (lifting.kept_box_records).  Per-stage GPU times go into `timer` under the reference's bucket names.
    on_records(records of one batch as numpy, first output index, number of samples): called per finished batch whose samples are a
    contiguous run of the output order, with (None, 0, 0) otherwise.  filters: the opt-in stage-2 filters (lifting.Stage2Filters); the
    time of their launch goes into the reference's "drivable" bucket.  cluster: the opt-in depth clustering (cluster.DepthCluster); its
    launches lie between the compaction's event and the medoid's, and their time goes into a "cluster" bucket instead of "medoid".
    nms: the opt-in rotated-box NMS (nms.RotatedNms); its launch lies behind the last event.  yaw: the opt-in yaw fit (bevfit.YawFit);
    its two events come last, and the time between them goes into a "yawfit" bucket.  velocity: the opt-in velocity stage
    (velocity.Velocity), one call behind every pass; the (k, 2) velocities of the returned records (lifting.kept_box_velocities, same
    order) are appended to the list `vel_out` as ONE device tensor, and on_records gets a batch's share as a fourth argument.  tracks: the
    opt-in track stage (tracks.Tracks; with `velocity` only), one more call behind the velocity stage's: the records and velocities
    collected here are already what it left.  place: the opt-in placement (boxplace.BoxPlace; with `yaw` only); its two events come
    behind the yaw fit's, and the time between them goes into a "place" bucket.  size: the opt-in size stage (boxsize.BoxSize; with `yaw`,
    `place` and `velocity` only), one more call behind the track stage's: the (k, 3) sizes of the returned records (lifting.kept_box_sizes)
    are appended to `size_out` as ONE device tensor the way the velocities are, on_records gets a batch's share as a fifth argument, and
    the velocities are those on the sized centres.  vertical: the opt-in vertical stage (boxvertical.BoxVertical; with any option or
    none), one call directly behind the pass; its two events come last, and the time between them goes into a "vertical" bucket.  The
    records' (k, 3) sizes then carry its heights in column 2 (lifting.kept_box_sizes) and are shipped exactly as the size stage's are,
    with or without a size stage.  ground: the opt-in ground stage (boxground.BoxGround; with any option or none), one call behind the
    vertical stage's; its two events come behind that stage's, and the time between them goes into a "ground" bucket.  The size rows'
    column 2 then carries its heights (`ground_h`), shipped the same way.  strip: the opt-in ground strip (groundstrip.GroundStrip; with
    any option or none), inside the pass between the compaction and the clustering; its two events come behind the filter's and in front
    of the clustering's, inside the "medoid" span, and the time between them goes into a "strip" bucket instead.  The records are what
    they were in form: nothing else changes here.  virtual: the opt-in virtual points (virtualpoints.FrameFiles; with any option or none),
    one call behind everything else; its two events come last of all, and the time between them goes into a "virtual points" bucket.  Every
    frame's seed word is its index in the output order, and every finished batch's frames with a point are written to their files here:
    the records are untouched.  owner: the opt-in point ownership (pointowner.PointOwner; with any option or none), inside the pass
    between the compaction and the strip; its two events come behind the filter's and in front of the strip's, inside the "medoid" span,
    and the time between them goes into an "owner" bucket instead.  labels: with `owner`, the virtualpoints.FrameFiles that names the
    job's frames under --point-labels' directory: every finished batch's frames with a listed point are written to their files here."""
    sized = size is not None or vertical is not None or ground is not None      # the records travel with (k, 3) size rows
    kw = {} if yaw is None else {"yaw": yaw}
    if place is not None:
        kw["place"] = place
    if velocity is not None:
        kw["velocity"] = velocity
    if tracks is not None:
        kw["tracks"] = tracks
    if size is not None:
        kw["size"] = size
    if vertical is not None:
        kw["vertical"] = vertical
    if ground is not None:
        kw["ground"] = ground
    if strip is not None:
        kw["strip"] = strip
    if virtual is not None:
        kw["virtual"] = virtual.stage
    if owner is not None:
        kw["owner"] = owner
    vels, sizes = [], []
    pipe = lifting.LiftPipeline(device, depth=2, classes=classes, filters=filters, cluster=cluster, nms=nms, **kw)
    n_f, n_c, n_y = (2 if filters is not None and filters.active else 0), (2 if cluster is not None else 0), (2 if yaw is not None else 0)
    n_p, n_v, n_g = (2 if place is not None else 0), (2 if vertical is not None else 0), (2 if ground is not None else 0)
    n_s, n_vp, n_o = (2 if strip is not None else 0), (2 if virtual is not None else 0), (2 if owner is not None else 0)
    n_f, n_own = n_f + n_o, n_f                                        # (the ownership's pair stands directly behind the filter's, at 5 + n_own)
    n_evs = 5 + n_f + n_s + n_c + n_y + n_p + n_v + n_g + n_vp
    records, pending, segments = [], [], []                            # pending: (slot, frame ids, stage events) in flight, oldest first

    def spent(key, since):
        timer[key] = timer.get(key, 0.0) + time.time() - since

    def drain(keep):
        while len(pending) > keep:
            t1 = time.time()
            slot, ids, evs = pending.pop(0)
            records.append(pipe.collect_records(slot, ids))           # stays on the device until the one gather at the end
            if velocity is not None:                                   # (the slot's stream has been synchronised)
                vels.append(lifting.kept_box_velocities(pipe.engines[slot].b))
            if sized:
                sizes.append(lifting.kept_box_sizes(pipe.engines[slot].b))
            spent("gpu lifting", t1)
            if virtual is not None:                                    # this batch's files; every rank writes its own frames'
                t1 = time.time()
                virtual.write_batch(lifting.virtual_point_frames(pipe.engines[slot]), ids[:, 0])
                spent("write", t1)
            if labels is not None and owner is not None:               # this batch's painted cloud; every rank writes its own frames'
                t1 = time.time()
                pomod.write_batch(labels, lifting.point_label_frames(pipe.engines[slot]), ids[:, 0])
                spent("write", t1)
            if on_records is not None:
                first = int(ids[0, 0]) if len(ids) else 0
                extra = () if velocity is None else (vels[-1].cpu().numpy(),)
                if sized:
                    extra += (None,) * (1 - len(extra)) + (sizes[-1].cpu().numpy(),)
                if len(ids) and np.array_equal(ids[:, 0], np.arange(first, first + len(ids))):
                    on_records(records[-1].cpu().numpy(), first, len(ids), *extra)
                else:
                    on_records(None, 0, 0)
            if len(evs) == n_evs:                                      # (complete: the slot's stream has been synchronised)
                spans = [("points in mask", 0, 1), ("medoid", 1, 2), ("closest lane", 2, 3), ("nms", 3, 4)]
                if filters is not None and filters.active:
                    spans.append(("drivable", 5, 6))
                for key, a, b in spans:
                    timer[key] = timer.get(key, 0.0) + evs[a].elapsed_time(evs[b]) * 1e-3
                if owner is not None:                                  # the two events behind the filter's, inside the "medoid" span
                    dt = evs[5 + n_own].elapsed_time(evs[6 + n_own]) * 1e-3
                    timer["owner"] = timer.get("owner", 0.0) + dt
                    timer["medoid"] -= dt
                if strip is not None:                                  # the two events behind the filter's (and the ownership's), inside the "medoid" span
                    dt = evs[5 + n_f].elapsed_time(evs[6 + n_f]) * 1e-3
                    timer["strip"] = timer.get("strip", 0.0) + dt
                    timer["medoid"] -= dt
                if cluster is not None:                                # the two events behind the strip's, inside the "medoid" span too
                    dt = evs[5 + n_f + n_s].elapsed_time(evs[6 + n_f + n_s]) * 1e-3
                    timer["cluster"] = timer.get("cluster", 0.0) + dt
                    timer["medoid"] -= dt
                if yaw is not None:                                    # behind the pass
                    timer["yawfit"] = timer.get("yawfit", 0.0) + evs[5 + n_f + n_s + n_c].elapsed_time(evs[6 + n_f + n_s + n_c]) * 1e-3
                if place is not None:                                  # behind the yaw fit's boxes
                    at = 5 + n_f + n_s + n_c + n_y
                    timer["place"] = timer.get("place", 0.0) + evs[at].elapsed_time(evs[at + 1]) * 1e-3
                if vertical is not None:                               # behind the pass
                    timer["vertical"] = timer.get("vertical", 0.0) + evs[-2 - n_g - n_vp].elapsed_time(evs[-1 - n_g - n_vp]) * 1e-3
                if ground is not None:                                 # the two events behind the vertical stage's
                    timer["ground"] = timer.get("ground", 0.0) + evs[-2 - n_vp].elapsed_time(evs[-1 - n_vp]) * 1e-3
                if virtual is not None:                                # the last two events
                    timer["virtual points"] = timer.get("virtual points", 0.0) + evs[-2].elapsed_time(evs[-1]) * 1e-3

    try:
        for hb, ids, host_s in prepared:
            timer["io"] = timer.get("io", 0.0) + host_s
            if hb is None:
                continue
            t1 = time.time()
            _attach_raw(hb, segments)
            drain(pipe.depth - 1)                                      # the slot about to be reused is free
            if virtual is not None:                                    # a frame's seed word: its index in the job's output order
                hb.frame_seed = np.asarray(ids[:, 0], np.int64).astype(np.uint32)
            evs = []
            t2 = time.time()
            slot = pipe.submit(hb, masks, stage_events=evs)
            pending.append((slot, ids, evs))
            spent("host upload + launches", t2)
            if segments:                                               # the upload has copied the sweeps: free the segment
                pipe.uploaded[slot].synchronize()                      # (an event behind the H2D copies, not the whole pass)
                hb.raw = None
                _release(segments)
            spent("gpu lifting", t1)
        drain(0)
    finally:
        _release(segments)
    if vel_out is not None and velocity is not None:
        vel_out.append(torch.cat(vels, 0) if vels else torch.zeros(0, 2, dtype=torch.float64, device=device))
    if size_out is not None and sized:
        size_out.append(torch.cat(sizes, 0) if sizes else torch.zeros(0, 3, dtype=torch.float64, device=device))
    if records:
        return torch.cat(records, 0)
    return torch.zeros(0, 10, dtype=torch.float64, device=device)


def lift_scenes(tables, scene_names, mask_dir, classes, device, n_sweeps=3, ratio=0.64, masks="rle", timer=None,
                scenes_per_batch=4, missing_ok=False, workers=0, priors=None, token_index=None, reader_threads=-1, filters=None,
                cluster=None, nms=None, yaw=None, velocity=None, vel_out=None, tracks=None, place=None, size=None, size_out=None,
                vertical=None, ground=None, strip=None, virtual=None, owner=None, labels=None):
    """Runs the hot path over the given scenes; returns the kept-box records of all their frames as ONE device tensor
    (lifting.kept_box_records; column 5 = token_index[sample token], default: the index into sample_tokens(scene_names)).
    workers > 0: that many reader processes prepare the batches (prepare_scene_batch: file reads, RLE strings,
    packing -- single-threaded Python does ~360 frames/s of it, the GPU loop 63 k) while this process only uploads,
    launches and collects; each reader loads the tables itself, and runs the native loader on reader_threads threads
    (0: its share of the cores, -1: the Python reader)."""
    timer = timer if timer is not None else {}
    if token_index is None:
        token_index = {t: i for i, t in enumerate(sample_tokens(tables, scene_names))}
    _WORKER_TABLES.setdefault((tables.version, tables.dataroot), tables)
    tasks = [BatchTask(tables.version, tables.dataroot, mask_dir, list(scene_names[b0:b0 + scenes_per_batch]), n_sweeps, ratio, missing_ok, priors,
                       drivable=bool(filters is not None and filters.drivable))
             for b0 in range(0, len(scene_names), scenes_per_batch)]

    def prepared():                                    # (starts with the first batch asked for: the readers spawn once the engines exist)
        pool, done = None, map(prepare_scene_batch, tasks)
        if workers > 0 and len(tasks) > 1:
            import multiprocessing as mp
            nproc = min(workers, len(tasks))
            pool = mp.get_context("spawn").Pool(nproc)     # spawn: the readers never inherit GPU state
            per = None
            if reader_threads >= 0:                        # every reader process runs the native loader on its share of the cores
                per = int(reader_threads if reader_threads > 0 else max(1, (os.cpu_count() or nproc) // nproc))
            done = pool.imap(prepare_scene_batch, [replace(t, through_shm=True, reader_threads=per) for t in tasks])
        try:
            for _, batches, io_s in done:
                yield from _token_batches(batches, token_index, io_s)
        finally:
            if pool is not None:
                pool.terminate()
                pool.join()
    with contextlib.closing(prepared()) as batches:
        return _lift_batches(batches, device, classes, masks, timer, filters=filters, cluster=cluster, nms=nms, yaw=yaw, velocity=velocity,
                             vel_out=vel_out, tracks=tracks, place=place, size=size, size_out=size_out, vertical=vertical, ground=ground,
                             strip=strip, virtual=virtual, owner=owner, labels=labels)


def _native_batch_lanes(nt, names, lane_cache):
    """The scenes' lane tables (one per map location, cached) and the table every frame of the batch uses."""
    # one table per distinct LOCATION of the batch (four scenes of one city used to upload and index that city's table
    # four times), in sorted order so that batches with the same set of cities carry the same tables -- the engines' shared cache
    # of lane indices (lifting.LiftEngine) is keyed by that set
    scene_loc = [nt.location(name) for name in names]
    locs = sorted(set(scene_loc))
    for loc in locs:
        if loc not in lane_cache:
            lane_cache[loc] = np.asarray(nusc_io.load_lane_points(nt.dataroot, loc), np.float64).astype(np.float32).reshape(-1, 3)   # torch.Tensor(...) at :278
    lanes = [lane_cache[loc] for loc in locs]
    frame_lane = []
    for name, loc in zip(names, scene_loc):
        frame_lane.extend([locs.index(loc)] * nt.scene_samples(name))
    return lanes, frame_lane, locs


def _native_batch_head(nt, names, mask_dir, n_sweeps, ratio, classes, missing_ok, lane_cache, sub=None, pool=None):
    """First host stage of a batch on the native route: table walk, <f>_data.json, mask pickles + RLE strings (reader.Tables /
    reader.Manifest) and the scenes' lane tables -- the latter on `pool` (a one-thread executor) beside the former when one is
    given: a job whose scenes all have their own map location loads a table per scene.  Returns what _native_batch_tail needs;
    lifting.BatchDeclined when the batch needs the Python reader (frames without masks to be dropped, mixed mask sizes, a pickle
    the native parser does not know)."""
    t = [time.perf_counter()]
    lanes_job = pool.submit(_native_batch_lanes, nt, names, lane_cache) if pool is not None else None
    with lifting.declining_unknown_formats():
        man = nt.manifest(names, mask_dir, n_sweeps, ratio, classes.names, missing_ok)
        t.append(time.perf_counter())
        counts, rle_off, fmo, wh = man.load_masks()
        t.append(time.perf_counter())
    if man.n_masks == 0 or (np.diff(fmo) == 0).any() or not np.array_equal(fmo, man.frame_mask_off):
        raise lifting.BatchDeclined("frames without masks, or mask files that disagree with the data files")
    if np.any(wh != wh[0]):
        raise lifting.BatchDeclined("masks of different image sizes in one batch")
    lanes, frame_lane, locs = lanes_job.result() if lanes_job is not None else _native_batch_lanes(nt, names, lane_cache)
    t.append(time.perf_counter())
    if sub is not None:
        for key, a in (("host table walk + data.json", 0), ("host mask files", 1), ("host lane tables", 2)):
            sub[key] = sub.get(key, 0.0) + t[a + 1] - t[a]
    return man, counts, rle_off, fmo, wh, lanes, frame_lane, locs


def _native_batch_tail(nt, head, sub=None, rd=None, drivable=False):
    """Second host stage: the batch's sweeps read straight into a page-locked buffer, and the HostBatch put together -- without
    a Python statement per frame.  Returns (HostBatch, rows of its frames in sample.json)."""
    man, counts, rle_off, fmo, wh, lanes, frame_lane, locs = head
    t0 = time.perf_counter()
    # the sweeps go straight into the batch's layout: quads (12 of a row's 20 bytes reach the page-locked buffer and the GPU; the
    # intensity is not uploaded -- no output of the entry point holds it) unless CM3D_RAW_LAYOUT=rows asks for the files' rows
    intensity = frame_rows = None
    if lifting.default_layout() == "quads":
        raw, intensity, row_off, frame_rows = man.load_sweeps_quads(5, rd)
        stride = lifting._lib.RAW_QUADS
    else:
        raw, row_off = man.load_sweeps(5, rd)
        stride = 5
    t1 = time.perf_counter()
    hb = lifting.assemble_batch(
        raw=raw, raw_stride=stride, intensity=intensity, frame_rows=frame_rows, sweep_row_off=row_off, sweep_xf=man.sweep_xf,
        frame_sweep_off=man.frame_sweep_off, cams=man.cams, mask_off=fmo, mask_cam=man.mask_cam, mask_wh=wh, rle_counts=counts, rle_off=rle_off,
        class_id=man.class_id, score=man.score, detections_per_frame=[np.diff(man.frame_mask_off)], lane_tables=lanes, frame_lane=frame_lane,
        ego_xyz=man.ego_xyz, width=int(wh[0, 0]), height=int(wh[0, 1]),
        lane_key=(nt.dataroot, tuple(locs)))              # which lane tables these are: LiftEngine keeps their spatial index across batches
    next_rows, stamps = nt.sample_links(man.sample_index)      # the sample table's `next` and `timestamp`: what lifting.Velocity reads
    hb.frame_next, hb.frame_time = velmod.frame_next_of_rows(man.sample_index, next_rows), velmod.frame_times(stamps)
    if drivable:                                           # the same locations' polygons, cached like the lane tables
        _attach_polygons(hb, nt.dataroot, locs)
    if sub is not None:
        sub["host sweep files"] = sub.get("host sweep files", 0.0) + t1 - t0
        sub["host assemble"] = sub.get("host assemble", 0.0) + time.perf_counter() - t1
    return hb, man.sample_index


def lift_scenes_native(nt, scene_names, mask_dir, classes, device, row_to_out, n_sweeps=3, ratio=0.64, masks="rle", timer=None,
                       scenes_per_batch=4, missing_ok=False, python_batch=None, on_records=None, filters=None, cluster=None, nms=None, yaw=None,
                       velocity=None, vel_out=None, tracks=None, place=None, size=None, size_out=None, vertical=None, ground=None, strip=None,
                       virtual=None, owner=None, labels=None):
    """lift_scenes with the whole host side in libcm3d_reader.so (reader.Tables): per batch one native table walk, one native read
    of all its files, one upload, one pass.  Three host threads in a row -- the reads of batch k+1 run under the upload and the
    launches of batch k -- and two batches in flight on the GPU.  row_to_out: row in sample.json -> index of the sample in the
    job's output order.  python_batch(names) -> (tokens, [HostBatch]) is the fallback for a batch the native path declines.
    on_records as in _lift_batches -- the caller can then write a batch's share of the result file while later batches still run."""
    timer = timer if timer is not None else {}
    lane_cache = {}
    from . import reader as rdmod
    rd_sweeps = rdmod.Reader(nt.rd.threads)                    # the sweep stage runs on a thread of its own: its own pool and buffers
    # (both pools together oversubscribe the cores by two: the table / mask stage is short and mostly waits on the sweep stage)
    # three host threads in a row: (1) table walk, data files, mask files and lane tables of batch k+2, (2) the sweep files of
    # batch k+1 into a page-locked buffer, (3) the caller's: upload and launches of batch k.  The native calls release the
    # interpreter lock, so the three really overlap.
    from concurrent.futures import ThreadPoolExecutor
    lane_pool = ThreadPoolExecutor(max_workers=1)

    def heads():
        for b0 in range(0, len(scene_names), scenes_per_batch):
            names = list(scene_names[b0:b0 + scenes_per_batch])
            t0 = time.time()
            try:
                head = _native_batch_head(nt, names, mask_dir, n_sweeps, ratio, classes, missing_ok, lane_cache, timer, lane_pool)
            except lifting.BatchDeclined:
                head = None
            yield names, head, time.time() - t0

    def tails():
        for names, head, io_s in _ahead(heads(), depth=1):
            t0 = time.time()
            got = None if head is None else _native_batch_tail(nt, head, timer, rd_sweeps, bool(filters is not None and filters.drivable))
            yield names, got, max(io_s, time.time() - t0)       # the two stages overlap: the longer one is the wall time

    def prepared():
        for names, got, io_s in _ahead(tails(), depth=1):
            if got is None:                                     # the Python reader takes this batch (its frames named by their rows)
                t0 = time.time()
                _, batches = python_batch(names)
                yield from _token_batches(batches, row_to_out, io_s + time.time() - t0)
            else:
                hb, rows = got
                yield hb, np.stack([row_to_out[rows].astype(np.float64), np.zeros(len(rows))], 1), io_s
    try:
        return _lift_batches(prepared(), device, classes, masks, timer, on_records, filters, cluster, nms, yaw, velocity, vel_out, tracks, place,
                             size, size_out, vertical, ground, strip, virtual, owner=owner, labels=labels)
    finally:
        lane_pool.shutdown(wait=False)


def main(argv=None):
    ap = argparse.ArgumentParser(description="CM3D 2D->3D lifting (nuScenes), MI355X path")
    ap.add_argument("--version", default=os.environ.get("CM3D_VER_NAME", VER_NAME))
    ap.add_argument("--dataroot", default=os.environ.get("CM3D_INPUT_PATH", INPUT_PATH))
    ap.add_argument("--mask-dir", default=os.environ.get("CM3D_INPUT_DIR", INPUT_DIR))
    ap.add_argument("--output-dir", default=os.environ.get("CM3D_OUTPUT_DIR", OUTPUT_DIR))
    ap.add_argument("--output-name", default=OUTPUT_NAME)
    ap.add_argument("--scenes", default=os.environ.get("CM3D_SCENES", ""), help="comma separated scene names (default: mini_val)")
    ap.add_argument("--priors", default="cfg/shape_priors_chatgpt.json")
    ap.add_argument("--ratio", type=float, default=0.64)          # :419
    ap.add_argument("--n-sweeps", type=int, default=3)            # :437
    ap.add_argument("--masks", default="rle", choices=["rle", "dense"])
    ap.add_argument("--missing-ok", action="store_true", help="frames without mask files yield no boxes instead of an error")
    ap.add_argument("--scenes-per-batch", type=int, default=4, help="scenes whose frames form one GPU batch")
    ap.add_argument("--workers", type=int, default=int(os.environ.get("CM3D_WORKERS", "0")),
                    help="reader processes that read and pack the batches with the Python reader (0: in this process)")
    ap.add_argument("--reader-threads", type=int, default=int(os.environ.get("CM3D_READER_THREADS", "0")),
                    help="threads of the native loader (libcm3d_reader.so) that reads sweeps and mask files; 0 = one per core, "
                         "-1 = the Python reader (pickle.load / np.fromfile per frame, like the reference)")
    # the stage-2 filters the reference ships commented out (:755-785); off unless asked for
    ap.add_argument("--drivable-filter", action="store_true",
                    help="drop car / truck / bus boxes whose medoid is not on a drivable-area polygon of the map (maps/expansion/<location>.json)")
    ap.add_argument("--lane-max-dist", type=float, default=None, metavar="M",
                    help="drop boxes farther than M metres from the nearest lane point (the reference's commented value: 20)")
    ap.add_argument("--vehicle-lane-max-dist", type=float, default=None, metavar="M",
                    help="the same for the pushed (vehicle) classes (the reference's commented value: 4)")
    clmod.add_arguments(ap)
    nmsmod.add_arguments(ap)
    bevfit.add_arguments(ap)
    boxplace.add_arguments(ap)
    velmod.add_arguments(ap)
    trmod.add_arguments(ap)
    szmod.add_arguments(ap)
    vtmod.add_arguments(ap)
    grmod.add_arguments(ap)
    gsmod.add_arguments(ap)
    vpmod.add_arguments(ap)
    pomod.add_arguments(ap)
    args = ap.parse_args(argv)
    cluster = clmod.from_namespace(args)
    nms = nmsmod.from_args(args)
    yaw = bevfit.from_namespace(args)
    place = boxplace.from_namespace(args, ap)       # (--place fit without --yaw fit: an error of the command line)
    velocity = velmod.from_args(args)
    tracks = trmod.from_args(args, ap)              # (a track flag without --velocity track: an error of the command line)
    size = szmod.from_args(args, ap)                # (--size track without --yaw fit --place fit --velocity track, or a --size-* flag alone: the same)
    vertical = vtmod.from_args(args, ap)            # (a --vertical-* flag without --vertical fit: the same)
    ground = grmod.from_args(args, ap)              # (a --ground-* flag without --ground fit: the same)
    strip = gsmod.from_namespace(args, ap)          # (a --ground-strip-* flag without --ground-strip grid: the same)
    vp_stage = vpmod.from_args(args, ap)            # (a --virtual-points-* flag without --virtual-points DIR: the same)
    owner = pomod.from_namespace(args, ap)          # (--point-owner-min-keep or --point-labels without --point-owner: the same)
    sized = size is not None or vertical is not None or ground is not None
    size_mine = []                                 # with --size track, --vertical fit or --ground fit: the sizes of this rank's records, one device tensor
    vel_mine = []                                  # with --velocity track: the velocities of this rank's records, one device tensor
    filters = lifting.Stage2Filters.from_args(args.drivable_filter, args.lane_max_dist, args.vehicle_lane_max_dist)

    total_start = time.time()
    rank, world, local_rank = cdist.init_from_env()
    if os.environ.get("CM3D_SINGLE_DEVICE"):      # rehearsal of the N>1 path on a one-GPU box (with CM3D_DIST_BACKEND=gloo)
        local_rank = 0
    device = f"cuda:{local_rank}"
    timer = {k: 0.0 for k in REFERENCE_BUCKETS}
    timer.update({"tables": 0.0, "gpu lifting": 0.0, "gather": 0.0, "write": 0.0, "total": 0.0})
    priors = _load_priors(args.priors)
    classes = lifting.ClassTable.nuscenes(priors)
    native = args.reader_threads >= 0 and args.workers <= 0
    py_tables = []

    def tables_py():                       # the Python tables, when something needs them (fallback batches, the Python reader)
        if not py_tables:
            py_tables.append(nusc_io.NuscTables(args.version, args.dataroot, annotations=False))
        return py_tables[0]
    if native:
        # the whole host side in libcm3d_reader.so: tables parsed once (natively, on the reader's threads), per batch one native
        # table walk + one native read of all its files; the Python tables are only loaded if a batch falls back
        from . import reader as rdmod
        nt = rdmod.Tables(rdmod.Reader(args.reader_threads), args.dataroot, args.version)
        known, n_samples = nt.scene_names(), nt.scene_samples
    else:
        tables = tables_py()
        known, n_samples = [s["name"] for s in tables.scenes()], lambda n: tables.scene_by_name(n)["nbr_samples"]
    timer["tables"] = time.time() - total_start
    names = [s for s in args.scenes.split(",") if s] or [n for n in MINI_VAL]
    if not args.scenes and not all(n in known for n in names):
        names = sorted(known)
    # scene-aligned sharding: each rank loads only its scenes' lane tables
    lo, hi = cdist.shard_scenes([n_samples(n) for n in names], world)[rank]
    if native:
        tokens, rows = nt.job_tokens(names)                    # the whole job's samples, identical on every rank
        virtual = None if vp_stage is None else vpmod.FrameFiles(vp_stage, args.virtual_points, list(tokens))
        labels = None if args.point_labels is None else vpmod.FrameFiles(None, args.point_labels, list(tokens))
        row_to_out = np.full(int(rows.max()) + 1 if len(rows) else 1, -1, np.int64)
        row_to_out[rows] = np.arange(len(rows))

        def python_batch(batch_names):
            tabs = tables_py()
            toks, batches, _ = prepare_scene_batch(BatchTask(args.version, args.dataroot, args.mask_dir, batch_names, args.n_sweeps, args.ratio,
                                                             args.missing_ok, priors, drivable=args.drivable_filter))
            sample_rows = {t: i for i, t in enumerate(tabs.t["sample"].keys())}
            for hb in batches:                                 # its frames named by their row in sample.json, like the native batches'
                hb.tokens = [sample_rows[t] for t in hb.tokens]
            return toks, batches
        # one rank: every finished batch's share of the result file is formatted right away, under the GPU work of the next ones
        # (on a thread of its own: formatting a batch's boxes takes as long as uploading and launching the next batch)
        import queue
        import threading
        parts, next_first, streamed = [], [0], [world == 1]
        write_q = queue.Queue()

        def write_worker():
            while True:
                item = write_q.get()
                if item is None:
                    return
                rec_np, first, count, vel_np, size_np = item
                t0 = time.time()
                if rec_np is None or first != next_first[0]:
                    streamed[0] = False
                elif streamed[0]:
                    parts.append(lifting.nuscenes_results_json_native(rec_np, tokens, classes, None, part=(first, count), vel=vel_np, size=size_np))
                    next_first[0] = first + count
                timer["write"] += time.time() - t0
        writer = threading.Thread(target=write_worker, daemon=True)
        writer.start()

        def on_records(rec_np, first, count, vel_np=None, size_np=None):
            write_q.put((rec_np, first, count, vel_np, size_np))
        mine = lift_scenes_native(nt, names[lo:hi], args.mask_dir, classes, device, row_to_out, args.n_sweeps, args.ratio, args.masks, timer,
                                  scenes_per_batch=max(1, args.scenes_per_batch), missing_ok=args.missing_ok, python_batch=python_batch,
                                  on_records=on_records if world == 1 else None, filters=filters, cluster=cluster, nms=nms, yaw=yaw,
                                  velocity=velocity, vel_out=vel_mine, tracks=tracks, place=place, size=size, size_out=size_mine,
                                  vertical=vertical, ground=ground, strip=strip, virtual=virtual, owner=owner, labels=labels)
        write_q.put(None)
        writer.join()
        streamed[0] = streamed[0] and next_first[0] == len(tokens)
    else:
        tokens = sample_tokens(tables, names)                  # the whole job's samples, identical on every rank
        virtual = None if vp_stage is None else vpmod.FrameFiles(vp_stage, args.virtual_points, list(tokens))
        labels = None if args.point_labels is None else vpmod.FrameFiles(None, args.point_labels, list(tokens))
        mine = lift_scenes(tables, names[lo:hi], args.mask_dir, classes, device, args.n_sweeps, args.ratio, args.masks, timer,
                           missing_ok=args.missing_ok, workers=args.workers, priors=priors, scenes_per_batch=max(1, args.scenes_per_batch),
                           token_index={t: i for i, t in enumerate(tokens)}, reader_threads=args.reader_threads, filters=filters, cluster=cluster, nms=nms, yaw=yaw,
                           velocity=velocity, vel_out=vel_mine, tracks=tracks, place=place, size=size, size_out=size_mine, vertical=vertical, ground=ground,
                           strip=strip, virtual=virtual, owner=owner, labels=labels)

    # the single exchange of the job: fixed-size box records -> rank 0 (one RCCL all_gather of payload; also the path of a
    # one-rank run).  Ranks hold contiguous scene blocks, so rank order is sample order.
    t0 = time.time()
    gathered = cdist.gather_records(mine, dst=0)
    gathered_vel = cdist.gather_records(vel_mine[0], dst=0) if velocity is not None else None      # rank order is sample order here too
    gathered_size = cdist.gather_records(size_mine[0], dst=0) if sized else None
    if world > 1:
        torch.distributed.barrier()
        torch.distributed.destroy_process_group()
    if rank != 0:
        return 0
    rec = torch.cat([g.cpu() for g in gathered], 0).numpy()
    vel = torch.cat([g.cpu() for g in gathered_vel], 0).numpy() if velocity is not None else None
    sizes = torch.cat([g.cpu() for g in gathered_size], 0).numpy() if sized else None
    timer["gather"] = time.time() - t0

    # the writer (:929-930): the records straight to the text json.dump would produce for the reference's dict of box lists
    t0 = time.time()
    os.makedirs(args.output_dir, exist_ok=True)
    if native:
        with open(os.path.join(args.output_dir, args.output_name), "wb") as f:
            if streamed[0]:
                f.write(lifting.nuscenes_results_json_head(dict(META)) + b", ".join(parts) + b"}}")
            else:
                f.write(lifting.nuscenes_results_json_native(rec, tokens, classes, dict(META), vel=vel, size=sizes))
    else:
        text, _ = lifting.nuscenes_results_json(rec, tokens, classes, dict(META), vel=vel, size=sizes)
        with open(os.path.join(args.output_dir, args.output_name), "w") as f:
            f.write(text)
    timer["write"] += time.time() - t0
    print(f"wrote {len(tokens)} samples.")
    timer["total"] = time.time() - total_start
    for op, v in timer.items():
        print(op, ":\t\t", v)
    return 0
