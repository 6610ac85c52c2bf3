// Host side of the opt-in clustered pass (cm3d_lift_pass_clustered, include/cm3d_hip.h): the pass through the compaction, the depth
// clustering of the in-mask lists it left in device memory, and the rest of the pass on the clustered lists.  No kernel lives here,
// and csrc/pipeline.cpp knows nothing of this file: the plain pass and cm3d_pipe_submit stay what they are.
#include <hip/hip_runtime_api.h>

#include "../../include/cm3d_hip.h"

static int record(void *ev, cm3d_stream_t st)
{
    return !ev || hipEventRecord((hipEvent_t)ev, (hipStream_t)st) == hipSuccess ? CM3D_OK : CM3D_ERR_LAUNCH;
}

extern "C" int cm3d_lift_pass_clustered(const cm3d_lift_pass_desc *d, const cm3d_depth_cluster_desc *c, cm3d_stream_t st)
{
    if (!d || !c || c->size != (int64_t)sizeof(cm3d_depth_cluster_desc)) return CM3D_ERR_ARG;
    if (!c->cl_off || !c->cl_tile_off || !c->cl_xyz || !c->cl_status || (d->hit_idx && !c->cl_idx)) return CM3D_ERR_ARG;
    int rc;
    if ((rc = cm3d_lift_pass_head(d, st)) != CM3D_OK || (rc = record(c->ev[0], st)) != CM3D_OK) return rc;
    rc = cm3d_depth_cluster(d->hit_xyz, d->hit_idx, d->hit_off, d->mask_frame, d->n_masks, d->idx_cap, c->origin, d->n_frames, c->eps,
                            c->min_points, c->pick, c->cl_off, c->cl_tile_off, d->hit_idx ? c->cl_idx : nullptr, c->cl_xyz, c->cl_status,
                            c->ws, c->ws_bytes, st);
    if (rc != CM3D_OK || (rc = record(c->ev[1], st)) != CM3D_OK) return rc;
    // the rest of the pass on the clustered lists; their work list is built by the medoid stage (tile_work belongs to the raw lists)
    cm3d_lift_pass_desc t = *d;
    t.hit_off = c->cl_off, t.tile_off = c->cl_tile_off, t.hit_idx = c->cl_idx, t.hit_xyz = c->cl_xyz, t.tile_work = nullptr;
    return cm3d_lift_pass_tail(&t, st);
}
