// Points in drivable-area polygons (eval_custom.py:496-526 of the reference, and the commented stage-2 filters of
// 2d_to_3d.py:755-785): the exact float64 even-odd test of cm3d_amd.eval_detection.point_in_polygons for many points against a
// city-sized polygon table, and the stage-2 filter rule on top of it (include/cm3d_hip.h spells both out).
//
// The index is built on the host (cm3d_amd/drivable.py): per table a uniform set of y-slabs, each listing -- grouped by ring, rings in
// polygon order, a polygon's exterior first -- the edges whose closed y-interval touches the slab.  A query is one wave: the lanes
// take the slab's entries 64 at a time, one ballot gives the crossings, and the runs of equal ring ids inside the chunk are walked
// with wave-uniform scalars (parity per ring, rings into polygons, OR over polygons).  Nothing here writes anything but the outputs
// at the point's / mask's own index, and every table or class id read from memory is range-checked before it is used as an index.
#include "common.h"

namespace {

struct PolyIndex {
    const double *tab_y;        // [T][3] y-min, y-max, slabs per unit of y
    const int32_t *tab_slab;    // [T][2] first slab, number of slabs
    const int32_t *slab_off;    // [slabs + 1] entries of slab s at [slab_off[s], slab_off[s + 1])
    const int32_t *ent_edge;    // [entries] edge of the entry
    const int32_t *ent_ring;    // [entries] ring of that edge
    const double *edge;         // [E][4] xs, ys, xn, yn
    const int32_t *ring_info;   // [R] 2 * polygon + (1 for a hole)
    int32_t n_tables;
};

// Called by a whole wave with wave-uniform t, x, y; every lane gets the answer.
__device__ bool poly_inside(const PolyIndex &ix, int t, double x, double y)
{
    if (t < 0 || t >= ix.n_tables) return false;
    const double ymin = ix.tab_y[3 * t], ymax = ix.tab_y[3 * t + 1], per_y = ix.tab_y[3 * t + 2];
    const int s0 = ix.tab_slab[2 * t], n_slabs = ix.tab_slab[2 * t + 1];
    if (n_slabs <= 0 || !(y >= ymin && y <= ymax)) return false;        // (a NaN is outside, as it crosses no edge)
    // the slab: the host lists an edge in every slab this very expression gives for a y of its closed interval (it is monotone in y),
    // and one more on either side
    const double f = (y - ymin) * per_y;
    const int s = f < (double)(n_slabs - 1) ? (int)f : n_slabs - 1;
    const int e0 = ix.slab_off[s0 + s], e1 = ix.slab_off[s0 + s + 1];
    const int lane = cm3d_lane();
    int cur_ring = -1, cur_info = 0, cur_poly = -1;
    unsigned par = 0;
    bool ext_odd = false, hole_odd = false, inside = false;
    for (int c = e0; c < e1 && !inside; c += CM3D_WAVE) {
        const int i = c + lane;
        int ring = -1;
        bool cross = false;
        if (i < e1) {
            ring = ix.ent_ring[i];
            const double *e = ix.edge + 4 * (int64_t)ix.ent_edge[i];
            const double xs = e[0], ys = e[1], xn = e[2], yn = e[3];
            if ((ys > y) != (yn > y)) cross = x < ((xn - xs) * (y - ys)) / (yn - ys) + xs;
        }
        const uint64_t crossed = __ballot(cross);
        uint64_t rest = __ballot(i < e1);
        while (rest) {
            const int r = __builtin_amdgcn_readlane(ring, __ffsll((unsigned long long)rest) - 1);
            const uint64_t same = __ballot(ring == r) & rest;
            if (r != cur_ring) {
                if (cur_ring >= 0) {
                    if (cur_info & 1) hole_odd |= par != 0;
                    else ext_odd = par != 0;
                }
                cur_ring = r, cur_info = ix.ring_info[r], par = 0;
                if ((cur_info >> 1) != cur_poly) {
                    inside |= ext_odd && !hole_odd;
                    ext_odd = hole_odd = false;
                    cur_poly = cur_info >> 1;
                }
            }
            par ^= (unsigned)__popcll(crossed & same) & 1u;
            rest &= ~same;
        }
    }
    if (cur_ring >= 0) {
        if (cur_info & 1) hole_odd |= par != 0;
        else ext_odd = par != 0;
    }
    return inside || (ext_odd && !hole_odd);
}

__global__ __launch_bounds__(256) void k_points_in_polygons(const double *__restrict__ xy, const int32_t *__restrict__ point_table,
                                                            int32_t n_points, PolyIndex ix, uint8_t *__restrict__ inside)
{
    const int p = blockIdx.x * 4 + __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    if (p >= n_points) return;
    const bool in = poly_inside(ix, point_table[p], xy[2 * (int64_t)p], xy[2 * (int64_t)p + 1]);
    if (cm3d_lane() == 0) inside[p] = in ? 1 : 0;
}

__global__ __launch_bounds__(256) void k_stage2_filter(const float *__restrict__ centroid_g, const int32_t *__restrict__ medoid_pos,
                                                       const int32_t *__restrict__ mask_frame, const int32_t *__restrict__ frame_lane,
                                                       const int32_t *__restrict__ class_id, const double *__restrict__ lane_dist,
                                                       int32_t n_masks, int32_t n_frames, PolyIndex ix, bool have_polygons,
                                                       const int32_t *__restrict__ needs_road, const int32_t *__restrict__ is_vehicle,
                                                       int32_t n_classes, double lane_max_dist, double vehicle_lane_max_dist,
                                                       int32_t *__restrict__ medoid_pos_kept, uint8_t *__restrict__ on_road)
{
    const int m = blockIdx.x * 4 + __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    if (m >= n_masks) return;
    const int mp = medoid_pos[m];
    int kept = mp;
    bool on = false;
    if (mp >= 0) {
        const int cls = class_id[m], f = mask_frame[m];
        const bool known = cls >= 0 && cls < n_classes;
        const double ld = lane_dist[m];
        bool drop = ld > lane_max_dist || (known && is_vehicle[cls] && ld > vehicle_lane_max_dist);
        if (have_polygons) {
            // the medoid itself (the reference's float(m_x), float(m_y)), not the pushed centre
            on = f >= 0 && f < n_frames && poly_inside(ix, frame_lane[f], (double)centroid_g[3 * (int64_t)m], (double)centroid_g[3 * (int64_t)m + 1]);
            drop |= known && needs_road[cls] && !on;
        }
        if (drop) kept = -1;
    }
    if (cm3d_lane() == 0) {
        medoid_pos_kept[m] = kept;
        on_road[m] = on ? 1 : 0;
    }
}

}  // namespace

extern "C" int cm3d_points_in_polygons(const double *xy, const int32_t *point_table, int32_t n_points, const double *tab_y,
                                       const int32_t *tab_slab, const int32_t *slab_off, const int32_t *ent_edge, const int32_t *ent_ring,
                                       const double *edge, const int32_t *ring_info, int32_t n_tables, uint8_t *inside, cm3d_stream_t stream)
{
    if (n_points < 0 || n_tables <= 0) return CM3D_ERR_ARG;
    if (n_points == 0) return CM3D_OK;
    if (!xy || !point_table || !tab_y || !tab_slab || !slab_off || !ent_edge || !ent_ring || !edge || !ring_info || !inside) return CM3D_ERR_ARG;
    const PolyIndex ix = {tab_y, tab_slab, slab_off, ent_edge, ent_ring, edge, ring_info, n_tables};
    hipLaunchKernelGGL(k_points_in_polygons, dim3((n_points + 3) / 4), dim3(256), 0, (hipStream_t)stream, xy, point_table, n_points, ix, inside);
    CM3D_CHECK_LAUNCH();
    return CM3D_OK;
}

extern "C" int cm3d_stage2_filter(const float *centroid_g, const int32_t *medoid_pos, const int32_t *mask_frame, const int32_t *frame_lane,
                                  const int32_t *class_id, const double *lane_dist, int32_t n_masks, int32_t n_frames, const double *tab_y,
                                  const int32_t *tab_slab, const int32_t *slab_off, const int32_t *ent_edge, const int32_t *ent_ring,
                                  const double *edge, const int32_t *ring_info, int32_t n_tables, const int32_t *needs_road,
                                  const int32_t *is_vehicle, int32_t n_classes, double lane_max_dist, double vehicle_lane_max_dist,
                                  int32_t *medoid_pos_kept, uint8_t *on_road, cm3d_stream_t stream)
{
    if (n_masks <= 0 || n_frames <= 0 || n_classes <= 0) return CM3D_ERR_ARG;
    if (!centroid_g || !medoid_pos || !mask_frame || !frame_lane || !class_id || !lane_dist || !is_vehicle || !medoid_pos_kept || !on_road)
        return CM3D_ERR_ARG;
    const bool have = tab_y != nullptr;
    if (have && (!tab_slab || !slab_off || !ent_edge || !ent_ring || !edge || !ring_info || !needs_road || n_tables <= 0)) return CM3D_ERR_ARG;
    const PolyIndex ix = {tab_y, tab_slab, slab_off, ent_edge, ent_ring, edge, ring_info, have ? n_tables : 0};
    hipLaunchKernelGGL(k_stage2_filter, dim3((n_masks + 3) / 4), dim3(256), 0, (hipStream_t)stream, centroid_g, medoid_pos, mask_frame,
                       frame_lane, class_id, lane_dist, n_masks, n_frames, ix, have, needs_road, is_vehicle, n_classes, lane_max_dist,
                       vehicle_lane_max_dist, medoid_pos_kept, on_road);
    CM3D_CHECK_LAUNCH();
    return CM3D_OK;
}
