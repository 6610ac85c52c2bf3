// Host side of a pass: one call that enqueues every launch of a pass over a resident batch (cm3d_lift_pass: the only statement of a
// pass's order, include/cm3d_hip.h spells it out; its two halves, through the compaction and from the medoid on, are exported too), and the pipeline object that decides which stream a slot's pass goes to
// (csrc/pipe_sched.h) and keeps two passes of one slot in order when they land on different streams.  No kernel lives here: every
// launch goes through the entry points of include/cm3d_hip.h.
#include <hip/hip_runtime_api.h>

#include <cstdlib>
#include <new>

#include "../../include/cm3d_hip.h"
#include "pipe_sched.h"

static int record(void *ev, cm3d_stream_t st)
{
    return !ev || hipEventRecord((hipEvent_t)ev, (hipStream_t)st) == hipSuccess ? CM3D_OK : CM3D_ERR_LAUNCH;
}

static int lift_masks(const cm3d_lift_pass_desc *d, bool on_masks, cm3d_stream_t st)
{
    if (d->dense) return cm3d_erode_pack(d->dense, d->n_masks, d->W, d->H, d->packed, d->bbox, st);
    if (d->mask_wh)
        return on_masks ? cm3d_rle_erode_pack_sized_begin(d->rle_counts, d->rle_off, d->n_masks, d->total_runs, d->W, d->H, d->mask_wh,
                                                          d->packed, d->bbox, d->rle_ws, d->rle_ws_bytes, d->status, d->hit_count,
                                                          d->n_masks, d->removed_bits, d->removed_words, st)
                        : cm3d_rle_erode_pack_sized(d->rle_counts, d->rle_off, d->n_masks, d->total_runs, d->W, d->H, d->mask_wh, d->packed,
                                                    d->bbox, d->rle_ws, d->rle_ws_bytes, st);
    return on_masks ? cm3d_rle_erode_pack_begin(d->rle_counts, d->rle_off, d->n_masks, d->total_runs, d->W, d->H, d->packed, d->bbox,
                                                d->rle_ws, d->rle_ws_bytes, d->status, d->hit_count, d->n_masks, d->removed_bits,
                                                d->removed_words, st)
                    : cm3d_rle_erode_pack(d->rle_counts, d->rle_off, d->n_masks, d->total_runs, d->W, d->H, d->packed, d->bbox, d->rle_ws,
                                          d->rle_ws_bytes, st);
}

static bool bad_desc(const cm3d_lift_pass_desc *d)
{
    if (!d || d->size != (int64_t)sizeof(cm3d_lift_pass_desc)) return true;
    return !d->fused && !d->points;                          // the separate launches hand the cloud from one to the other
}

extern "C" int cm3d_lift_pass(const cm3d_lift_pass_desc *d, cm3d_stream_t st)
{
    if (bad_desc(d)) return CM3D_ERR_ARG;
    const int rc = cm3d_lift_pass_head(d, st);
    return rc != CM3D_OK ? rc : cm3d_lift_pass_tail(d, st);
}

extern "C" int cm3d_lift_pass_head(const cm3d_lift_pass_desc *d, cm3d_stream_t st)
{
    if (bad_desc(d)) return CM3D_ERR_ARG;
    int rc;
    // (resident run lengths on the fused-sweeps path: the mask launch is the pass's first and carries the reset -- one launch and one
    // launch boundary less per pass)
    const bool on_masks = !d->dense && d->fused && !d->separate_reset;
    if (!on_masks && (rc = cm3d_batch_begin(d->status, d->hit_count, d->n_masks, d->removed_bits, d->removed_words, st)) != CM3D_OK)
        return rc;
    if ((rc = record(d->ev_stage[0], st)) != CM3D_OK) return rc;
    if (!d->fused && (rc = cm3d_sweep_prep(d->raw, d->raw_stride, d->intensity, d->sweep_row_off, d->n_sweeps, d->max_rows_per_sweep,
                                           d->sweep_xf, d->frame_sweep_off, d->n_frames, d->halfw, d->points, d->pt_cap, d->pt_off,
                                           d->removed_bits, d->status, st)) != CM3D_OK)
        return rc;
    if ((rc = lift_masks(d, on_masks, st)) != CM3D_OK) return rc;
    rc = d->fused ? cm3d_sweep_project_hits(d->raw, d->raw_stride, d->intensity, d->sweep_row_off, d->n_sweeps, d->max_sweeps_per_frame,
                                            d->sweep_xf, d->frame_sweep_off, d->halfw, d->points, d->pt_cap, d->pt_off, d->removed_bits,
                                            d->n_frames, d->max_pts_per_frame, d->pt_cap, d->cams, d->n_cams, d->mask_off, d->mask_cam, d->bbox,
                                            d->packed, d->n_masks, d->W, d->H, d->min_dist, d->planes, d->hit_words, d->hit_count, d->status,
                                            d->pg_ws, d->pg_ws_bytes, d->ev_project[0], d->ev_project[1], st)
                  : cm3d_project_hits(d->points, d->pt_off, d->n_frames, d->max_pts_per_frame, d->pt_cap, d->cams, d->n_cams, d->mask_off,
                                      d->mask_cam, d->bbox, d->packed, d->n_masks, d->W, d->H, d->min_dist, d->planes, d->hit_words,
                                      d->hit_count, d->status, d->pg_ws, d->pg_ws_bytes, d->ev_project[0], d->ev_project[1], st);
    if (rc != CM3D_OK) return rc;
    // coordinates of the in-mask points: from the cloud when it exists, else re-derived from the raw rows
    const bool from_raw = d->points == nullptr;
    rc = cm3d_compact_hits(d->hit_words, d->planes, d->n_frames, d->max_pts_per_frame, d->pt_cap, d->mask_off, d->n_masks, d->hit_count,
                           d->removed_bits, from_raw ? d->raw : nullptr, d->raw_stride, from_raw ? d->intensity : nullptr,
                           from_raw ? d->sweep_xf : nullptr, d->points, d->hit_off, d->tile_off, d->hit_idx, nullptr, d->hit_xyz, d->idx_cap,
                           d->tile_work, d->status, d->pg_ws, d->pg_ws_bytes, st);
    return rc != CM3D_OK ? rc : record(d->ev_stage[1], st);
}

extern "C" int cm3d_lift_pass_tail(const cm3d_lift_pass_desc *d, cm3d_stream_t st)
{
    if (bad_desc(d)) return CM3D_ERR_ARG;
    int rc;
    // the hint: whatever the device has written into the page-locked word by now (a stale value costs time on one pass, never a result)
    int32_t md_flags = 0;
    if (d->md_hint && d->md_feedback && *(const volatile int32_t *)d->md_feedback == 0) md_flags = 1;
    rc = cm3d_medoid2(d->hit_xyz, nullptr, nullptr, d->n_masks, d->hit_off, d->tile_off, nullptr, d->idx_cap, d->tile_work, d->medoid_pos,
                      d->centroid, d->colsum, d->ws, d->ws_bytes, md_flags, d->md_feedback, st);
    if (rc != CM3D_OK || (rc = record(d->ev_stage[2], st)) != CM3D_OK) return rc;
    if (d->lane_ready && hipStreamWaitEvent((hipStream_t)st, (hipEvent_t)d->lane_ready, 0) != hipSuccess) return CM3D_ERR_LAUNCH;
    // (Waymo: the lane lookup happens in the global frame)
    if (d->pose_rt && (rc = cm3d_centroid_transform(d->centroid, d->medoid_pos, d->mask_frame, d->n_masks, d->pose_rt, d->centroid_g,
                                                    st)) != CM3D_OK) return rc;
    rc = cm3d_lane_nn(d->centroid_g, d->medoid_pos, d->mask_frame, d->n_masks, d->lane, d->lane_off, d->frame_lane, d->n_tables,
                      d->n_lane_points, d->grid, d->lane_idx, d->lane_dist, d->ws, d->ws_bytes, st);
    if (rc != CM3D_OK || (rc = record(d->ev_stage[3], st)) != CM3D_OK) return rc;
    // (`planes` words of mask bits per point: no frame of the batch has more than 32 * planes masks)
    rc = cm3d_box_nms_bounded(d->centroid_g, d->medoid_pos, d->mask_off, d->n_frames, d->n_masks, d->class_id, d->score, d->lane,
                              d->lane_off, d->frame_lane, d->lane_idx, d->lane_dist, d->prior_wlh, d->is_vehicle, d->nms_group, d->nms_thr,
                              d->n_classes, d->ego_xyz, d->pose_inv,
                              d->planes > 0 && d->planes < CM3D_MAX_MASKS_PER_FRAME / 32 ? 32 * d->planes : CM3D_MAX_MASKS_PER_FRAME,
                              d->box, d->flags, st);
    if (rc != CM3D_OK || (rc = record(d->ev_stage[4], st)) != CM3D_OK) return rc;
    if (d->obb_yaw)
        return cm3d_obb(d->hit_xyz, d->hit_off, d->n_masks, d->idx_cap, d->obb_yaw, d->obb_status, nullptr, nullptr, d->obb_ws,
                        d->obb_ws_bytes, st);
    return CM3D_OK;
}

extern "C" int cm3d_pipe_exec_streams_for(int32_t depth, int32_t hw_queues)
{
    if (hw_queues <= 0) hw_queues = cm3d::pipe_hw_queues(std::getenv("GPU_MAX_HW_QUEUES"));
    return cm3d::pipe_exec_streams(depth, hw_queues);
}

namespace {

struct Pipe {
    cm3d::PipeSched sched;
    hipStream_t streams[cm3d::kPipeMaxDepth];  // the slots' own (uploads, captures, a pinned pipeline's passes)
    hipStream_t exec[cm3d::kPipeMaxDepth];     // what a ticket's index means: streams[i], but handle 0 at null_exec
    int null_exec;                             // the executor that is the legacy null stream, -1: none
    hipEvent_t done[cm3d::kPipeMaxDepth];      // behind the slot's last pass (timing disabled)
    bool recorded[cm3d::kPipeMaxDepth];
    Pipe(int depth, int n_exec) : sched(depth, n_exec), null_exec(-1) {}
};

// the executor of the slot's next pass, ordered behind the slot's previous pass where that ran elsewhere; < 0: error
int pipe_take(Pipe *p, int32_t slot)
{
    if (!p || slot < 0 || slot >= p->sched.depth) return CM3D_ERR_ARG;
    const cm3d::PipeTicket t = p->sched.next(slot);
    if (t.wait && p->recorded[slot] && hipEventQuery(p->done[slot]) != hipSuccess) {
        (void)hipGetLastError();                // hipErrorNotReady is the expected answer, not a sticky error
        if (hipStreamWaitEvent(p->exec[t.stream], p->done[slot], 0) != hipSuccess) return CM3D_ERR_LAUNCH;
    }
    return t.stream;
}

int pipe_mark(Pipe *p, int32_t slot)
{
    const int s = p->sched.last[slot];
    if (s < 0) return CM3D_ERR_ARG;
    if (hipEventRecord(p->done[slot], p->exec[s]) != hipSuccess) return CM3D_ERR_LAUNCH;
    p->recorded[slot] = true;
    return CM3D_OK;
}

// CM3D_PIPE_NULL_EXEC=0 in the environment: the plan never takes the null stream
bool null_exec_allowed()
{
    const char *v = std::getenv("CM3D_PIPE_NULL_EXEC");
    return !(v && v[0] == '0' && v[1] == '\0');
}

}  // namespace

extern "C" void *cm3d_pipe_create(int32_t depth, int32_t exec_streams, const cm3d_stream_t *streams)
{
    return cm3d_pipe_create2(depth, exec_streams, streams, 0);
}

extern "C" void *cm3d_pipe_create2(int32_t depth, int32_t exec_streams, const cm3d_stream_t *streams, int32_t null_exec)
{
    if (depth < 1 || depth > cm3d::kPipeMaxDepth || !streams || null_exec < -1 || null_exec > 1) return nullptr;
    int n_exec = exec_streams > 0 ? (exec_streams < depth ? exec_streams : depth) : cm3d_pipe_exec_streams_for(depth, 0);
    bool null_last = null_exec == 1;
    // the plan's count where the caller names none: with null_exec = -1 its null executor too, with 1 a null executor in any case
    if (exec_streams <= 0 && (null_exec == 1 || (null_exec < 0 && null_exec_allowed()))) {
        const cm3d::PipeExecPlan plan = cm3d::pipe_exec_plan(depth, cm3d::pipe_hw_queues(std::getenv("GPU_MAX_HW_QUEUES")));
        n_exec = plan.n_exec;
        null_last = null_last || plan.null_last;
    }
    Pipe *p = new (std::nothrow) Pipe(depth, n_exec);
    if (!p) return nullptr;
    for (int i = 0; i < cm3d::kPipeMaxDepth; ++i) {
        p->streams[i] = nullptr;
        p->exec[i] = nullptr;
        p->done[i] = nullptr;
        p->recorded[i] = false;
    }
    for (int i = 0; i < depth; ++i) {
        p->streams[i] = p->exec[i] = (hipStream_t)streams[i];
        if (hipEventCreateWithFlags(&p->done[i], hipEventDisableTiming) != hipSuccess) {
            cm3d_pipe_destroy(p);
            return nullptr;
        }
    }
    if (null_last && p->sched.n_exec >= 2) {
        p->null_exec = p->sched.n_exec - 1;
        p->exec[p->null_exec] = nullptr;        // the legacy null stream
    }
    return p;
}

extern "C" void cm3d_pipe_destroy(void *pipe)
{
    Pipe *p = (Pipe *)pipe;
    if (!p) return;
    for (int i = 0; i < p->sched.depth; ++i)
        if (p->done[i]) (void)hipEventDestroy(p->done[i]);
    delete p;
}

extern "C" int cm3d_pipe_exec_streams(const void *pipe)
{
    return pipe ? ((const Pipe *)pipe)->sched.n_exec : CM3D_ERR_ARG;
}

extern "C" int cm3d_pipe_submit(void *pipe, int32_t slot, const cm3d_lift_pass_desc *desc)
{
    Pipe *p = (Pipe *)pipe;
    if (!desc) return CM3D_ERR_ARG;
    const int s = pipe_take(p, slot);
    if (s < 0) return s;
    const int rc = cm3d_lift_pass(desc, (cm3d_stream_t)p->exec[s]);
    // (the event also behind a pass that stopped half-way: what it did enqueue is what the slot's next pass must wait for)
    const int rm = pipe_mark(p, slot);
    if (rc != CM3D_OK) return rc;
    return rm != CM3D_OK ? rm : s;
}

extern "C" int cm3d_pipe_acquire(void *pipe, int32_t slot) { return pipe_take((Pipe *)pipe, slot); }

extern "C" int cm3d_pipe_release(void *pipe, int32_t slot)
{
    Pipe *p = (Pipe *)pipe;
    if (!p || slot < 0 || slot >= p->sched.depth) return CM3D_ERR_ARG;
    return pipe_mark(p, slot);
}

extern "C" int cm3d_pipe_wait(void *pipe, int32_t slot)
{
    Pipe *p = (Pipe *)pipe;
    if (!p || slot < 0 || slot >= p->sched.depth) return CM3D_ERR_ARG;
    if (!p->recorded[slot]) return CM3D_OK;
    return hipEventSynchronize(p->done[slot]) == hipSuccess ? CM3D_OK : CM3D_ERR_LAUNCH;
}

extern "C" int cm3d_pipe_pin(void *pipe)
{
    Pipe *p = (Pipe *)pipe;
    if (!p) return CM3D_ERR_ARG;
    p->sched.pin();
    // a graph replays on the slot's own stream, so the null executor ends here: its index means streams[index] again, and the slot whose
    // last pass it ran is ordered behind that pass now (the scheduler sees the same index and would not ask)
    const int e = p->null_exec;
    if (e >= 0) {
        p->null_exec = -1;
        p->exec[e] = p->streams[e];
        if (p->sched.last[e] == e && p->recorded[e] && hipStreamWaitEvent(p->streams[e], p->done[e], 0) != hipSuccess) return CM3D_ERR_LAUNCH;
    }
    return CM3D_OK;
}

extern "C" int cm3d_pipe_null_exec(const void *pipe) { return pipe ? ((const Pipe *)pipe)->null_exec : -1; }

extern "C" int cm3d_pipe_last_stream(const void *pipe, int32_t slot)
{
    const Pipe *p = (const Pipe *)pipe;
    if (!p || slot < 0 || slot >= p->sched.depth) return CM3D_ERR_ARG;
    return p->sched.last[slot];
}
