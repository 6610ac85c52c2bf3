// The seam of a composed pass (csrc/pass_options.cpp) for the file that puts stages between the compaction and the clustering
// (csrc/pass_compose.cpp), and the two helpers both files share.  Host code of the library; no part of the C-ABI of include/cm3d_hip.h.
//   lists   a copy of desc whose hit_off, tile_off, hit_idx, hit_xyz are the lists the pass goes on with and whose tile_work is NULL
//           (desc itself: nothing has been enqueued yet, the head runs inside)
//   check   CM3D_OK iff desc, opt (may be NULL) and every member of opt are what cm3d_lift_pass_opt accepts for those lists; no call
//   run     the same check, then: cluster ? cm3d_depth_cluster (lists -> cl_*) ; cm3d_lift_pass_tail ; filter ; yaw ; nms
#pragma once
#include <hip/hip_runtime_api.h>

#include "../../include/cm3d_hip.h"

extern "C" {
int cm3d_pass_seam_check(const cm3d_lift_pass_desc *desc, const cm3d_lift_pass_desc *lists, const cm3d_lift_pass_options *opt);
int cm3d_pass_seam_run(const cm3d_lift_pass_desc *desc, const cm3d_lift_pass_desc *lists, const cm3d_lift_pass_options *opt, cm3d_stream_t stream);
}

static inline int record(void *ev, cm3d_stream_t st)        // an optional event: NULL is skipped
{
    return !ev || hipEventRecord((hipEvent_t)ev, (hipStream_t)st) == hipSuccess ? CM3D_OK : CM3D_ERR_LAUNCH;
}

static inline int32_t bound(const cm3d_lift_pass_desc *d)   // no frame has more than 32 * planes masks
{
    return d->planes > 0 && d->planes < CM3D_MAX_MASKS_PER_FRAME / 32 ? 32 * d->planes : CM3D_MAX_MASKS_PER_FRAME;
}
