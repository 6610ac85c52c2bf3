/*
 * cm3d_hip.h -- C-ABI of libcm3d_hip.so: the MI355X (gfx950) kernels of CM3D's
 * 2D->3D pseudo-label lifting path.
 *
 * The reference has no FFI: its hot path is inline torch/numpy/OpenCV code in
 * src/{nuscenes,waymo,kitti}/2d_to_3d.py.  Each entry point below replaces the
 * block of reference code it cites (paths relative to the reference checkout,
 * src/nuscenes/ unless noted); INTEGRATION.md shows the ctypes stub a maintainer
 * of the reference would add.
 *
 * Conventions
 *  - every pointer is a DEVICE pointer unless its name ends in _host;
 *  - the caller owns every buffer; nothing is allocated or freed inside;
 *  - every call is asynchronous on `stream` (a hipStream_t passed as void*),
 *    never synchronises, and is safe to capture into a hipGraph;
 *  - return value: CM3D_OK or a negative CM3D_ERR_*; nothing throws;
 *  - thread-safe for distinct streams and distinct workspaces; no global state;
 *  - index arithmetic is int32: a batch holds < 2^31 points / mask words.
 *
 * Batch data model ("lift batch"): F frames; frame f owns sweeps
 * [frame_sweep_off[f], frame_sweep_off[f+1]), points [pt_off[f], pt_off[f+1])
 * and masks [mask_off[f], mask_off[f+1]).
 */
#ifndef CM3D_HIP_H
#define CM3D_HIP_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define CM3D_ABI_VERSION 5

#define CM3D_OK 0
#define CM3D_ERR_ARG (-1)      /* null pointer / non-positive size / unsupported shape */
#define CM3D_ERR_LAUNCH (-2)   /* hipGetLastError() != hipSuccess after a launch      */
#define CM3D_ERR_WORKSPACE (-3)/* workspace smaller than cm3d_*_workspace_bytes says  */

#define CM3D_CAM_STRIDE 64       /* floats per camera record, see cm3d_project_hits   */
#define CM3D_SWEEP_XF_STRIDE 24  /* floats per sweep transform, see cm3d_sweep_prep   */
#define CM3D_RAW_QUADS 3         /* raw_stride value that selects the quad layout of the raw rows, see cm3d_sweep_prep (ABI v4) */
#define CM3D_MAX_CAMS 8          /* cameras per frame                                  */
#define CM3D_MAX_MASKS_PER_FRAME 1024
#define CM3D_BBOX_STRIDE 8                 /* int32 per mask in `bbox` (ABI v3): eroded bounds [0..3], stored rectangle [4..7] */
#define CM3D_BOX_STRIDE 10       /* doubles per box record, see cm3d_box_nms           */
#define CM3D_MEDOID_TILE 64      /* columns per medoid tile (one wave)                 */
#define CM3D_MAX_MATCH_BOXES 1024 /* boxes per sample and side, see cm3d_bev_match    */
#define CM3D_MATCH_BOX_STRIDE 6  /* doubles per box of cm3d_bev_match                  */
#define CM3D_OBB_ROT_STRIDE 9    /* doubles per mask in cm3d_obb's rot_opt (row-major 3x3, ABI v5) */
#define CM3D_WM_BOX_STRIDE 8     /* doubles per box of cm3d_waymo_metrics                */
#define CM3D_WM_BREAKDOWNS 16    /* breakdowns of cm3d_waymo_metrics: (type - 1) * 4 + shard */
#define CM3D_WM_CUTOFFS 101      /* score cutoffs of cm3d_waymo_metrics: float32(c * 0.01) */
#define CM3D_WM_SWEEP_MAX_ALPHAS 1024 /* alphas of one cm3d_waymo_metrics_sweep call (added within ABI v5) */
#define CM3D_DEPTH_CLUSTER_LDS_POINTS 4096 /* longest list cm3d_depth_cluster sorts in LDS (added within ABI v5): 12 bytes per point,
                                              48 KiB per workgroup, three workgroups in a CU's 160 KiB */

/* status word written by kernels (int32[4] in device memory, zero it per batch):
 *  [0] bit0: point capacity overflow (cm3d_sweep_prep), bit1: hit-index capacity
 *      overflow (cm3d_compact_hits), bit2: too many masks in a frame / cams out of range,
 *      bit3: quad layout with a frame that does not start on a quad (cm3d_sweep_project_hits)
 *  [1] total points produced by cm3d_sweep_prep
 *  [2] total hit indices required by cm3d_compact_hits
 *  [3] total medoid tiles */
#define CM3D_STATUS_WORDS 4

typedef void *cm3d_stream_t;

int cm3d_abi_version(void);
const char *cm3d_error_string(int code);

/* Resets the per-pass device state: the status word, hit_count[n_masks] and (when not NULL) the removed-row bits
 * (removed_words = cm3d_removed_words(rows of the batch, n_frames) 32-bit words).  First call of every pass over a batch. */
int64_t cm3d_removed_words(int32_t n_rows, int32_t n_frames);
int cm3d_batch_begin(int32_t *status, int32_t *hit_count, int32_t n_masks, uint32_t *removed_bits, int64_t removed_words,
                     cm3d_stream_t stream);

/* ---- a2: sweep preparation -------------------------------------------------
 * Replaces 2d_to_3d.py:437-465 + utils/pcd.py:159-172,246-257: strip a raw sweep to 4 columns,
 * sensor->ego->global (rotate then translate, twice), sweeps of a frame back to back; one streaming pass.
 * The ego-box rows (|x|<halfw && |y|<halfw, halfw = f32(sqrt(2.3)), :442-445) are NOT compacted away:
 * they are written as NaN points (inert downstream) and marked in a bit set, and cm3d_compact_hits turns row
 * indices into indices of the reference's compacted cloud.  So point p of frame f sits at row pt_off[f]+p
 * of its raw rows.
 *  raw          float[rows][raw_stride]   all sweeps of the batch, back to back (raw_stride >= 4: the .bin files' rows), or
 *                                         raw_stride == CM3D_RAW_QUADS (ABI v4): the QUAD layout, float[ceil(rows/4)][3][4] --
 *                                         rows 4q..4q+3 of the batch as x0 x1 x2 x3 y0 y1 y2 y3 z0 z1 z2 z3, 16-byte aligned.
 *                                         12 bytes per row cross HBM (the path never reads the .bin files' ring index, and the
 *                                         intensity only for the points it lists), a lane's four rows are three 16-byte loads.
 *                                         In this layout every frame's first row is a multiple of 4: the loader pads a frame
 *                                         with up to 3 rows of NaN coordinates, which belong to the frame's last sweep and are
 *                                         rows like any other (never dropped, in no mask, at the end of the frame, so no index
 *                                         of a real row moves); status bit 8 reports a frame that starts inside a quad
 *  intensity    float[rows] or NULL       quad layout only: the rows' fourth column (goes into points / hit_xyz; NULL: zeros)
 *  sweep_row_off int32[S+1]               row offsets of the sweeps into raw
 *  sweep_xf     float[S][24]              [0..8] R_cs, [9..11] t_cs, [12..20] R_ego, [21..23] t_ego (float32,
 *                                         exactly the tensors the reference passes to rotate/translate)
 *  frame_sweep_off int32[F+1]
 *  points       float[pt_cap][4]  OUT     x,y,z,intensity in the global frame at the raw row index (pt_cap >= rows)
 *  pt_off       int32[F+1]        OUT     first row of each frame (= sweep_row_off[frame_sweep_off[f]])
 *  removed_bits uint32[cm3d_removed_words(rows, F)] IN/OUT  one bit per dropped row; must be zero on entry
 *                                         (cm3d_batch_begin).  Frame f's bits start at word (pt_off[f] >> 5) + 8 f,
 *                                         bit (r & 31) of word r >> 5 for its frame-local row r */
int cm3d_sweep_prep(const float *raw, int32_t raw_stride, const float *intensity, const int32_t *sweep_row_off, int32_t n_sweeps,
                    int32_t max_rows_per_sweep, const float *sweep_xf, const int32_t *frame_sweep_off,
                    int32_t n_frames, float halfw, float *points, int32_t pt_cap, int32_t *pt_off,
                    uint32_t *removed_bits, int32_t *status, cm3d_stream_t stream);

/* ---- a1: COCO-RLE expansion ------------------------------------------------
 * Replaces pycocotools.mask.decode at 2d_to_3d.py:425 (+ the transpose at :428): run
 * lengths -> dense uint8 [n][H][W] image-layout masks of 0/1.
 *  rle_counts uint32[]  run lengths of all masks back to back (alternating 0-run,1-run,...)
 *  rle_off    int32[n+1]
 *  W          1 .. 4096, like the erosion behind it (CM3D_ERR_ARG otherwise)
 *  workspace: cm3d_rle_workspace_bytes(total_runs) */
int64_t cm3d_rle_workspace_bytes(int32_t total_runs);
int cm3d_rle_to_dense(const uint32_t *rle_counts, const int32_t *rle_off, int32_t n_masks, int32_t total_runs,
                      int32_t W, int32_t H, uint8_t *dense, void *workspace, int64_t workspace_bytes,
                      cm3d_stream_t stream);

/* ---- a3: 3x3 erosion + bit-packing ------------------------------------------
 * Replaces cv2.erode(mask, ones((3,3))) + astype(bool) + transpose + H2D at
 * 2d_to_3d.py:526-527,542-544.  Out-of-image neighbours are ignored.
 *  dense   uint8[n][H][W]   non-zero = set
 *  packed  uint32[n][H*Wp]  OUT, Wp = (W+31)/32: one slot of H*Wp words per mask.  A mask's eroded bits are stored as the rows of a
 *          RECTANGLE of whole words (ABI v3): word columns xw0 .. xw0+wc-1, image rows y0 .. y0+rows-1, row after row from the start
 *          of the slot, wc words each: bit (x&31) of slot word (y - y0) * wc + (x>>5) - xw0 = eroded pixel (x,y).  cm3d_erode_pack
 *          stores the whole image (xw0 = y0 = 0, wc = Wp, rows = H: the layout of ABI v2); cm3d_rle_erode_pack the rectangle of the
 *          mask's set pixels, so that a mask's words are contiguous in memory.  Words of `packed` outside the stored rectangles are
 *          NEVER WRITTEN: the slot words behind a rectangle's rows * wc, the whole slot of a mask without a set pixel and whatever
 *          lies behind the last slot keep what they held before the call (when cm3d_rle_erode_pack takes its workgroup-per-mask form
 *          -- lists that average more than 1024 runs -- it reports the whole image as the stored rectangle, writes only the words of
 *          the set pixels' rectangle, at the image's row stride, and leaves the others as they were; the eroded bounds bbox[0..3] lie
 *          inside what was written).  n*H*Wp must stay below 2^31 (mask offsets are signed 32-bit word numbers).
 *  bbox    int32[n][CM3D_BBOX_STRIDE] OUT: [0..3] x0,y0,x1,y1 inclusive bounds of the eroded mask (x0>x1 when empty),
 *          [4..7] xw0, y0, wc, rows of the stored rectangle (all 0 for a mask without a set pixel) */
int cm3d_erode_pack(const uint8_t *dense, int32_t n_masks, int32_t W, int32_t H, uint32_t *packed,
                    int32_t *bbox, cm3d_stream_t stream);

/* f1: same result straight from run lengths, no dense intermediate
 * (fuses 2d_to_3d.py:425 with :526-527,542-544).  Stores the rectangle of the mask's set pixels (see `packed` above): only words
 * that can hold an eroded pixel are written. */
int cm3d_rle_erode_pack(const uint32_t *rle_counts, const int32_t *rle_off, int32_t n_masks, int32_t total_runs,
                        int32_t W, int32_t H, uint32_t *packed, int32_t *bbox, void *workspace,
                        int64_t workspace_bytes, cm3d_stream_t stream);

/* The same launch carrying the per-pass reset of cm3d_batch_begin (status word, hit_count[n_count_masks], removed-row bits): the mask stage is the
 * first stage of a pass over resident run lengths, and a launch of its own for the reset cost the pass a launch boundary (r04).  Only for passes
 * whose FIRST call is this one (cm3d_sweep_prep, which writes status and removed bits, must not have run before it in the pass). */
int cm3d_rle_erode_pack_begin(const uint32_t *rle_counts, const int32_t *rle_off, int32_t n_masks, int32_t total_runs,
                              int32_t W, int32_t H, uint32_t *packed, int32_t *bbox, void *workspace, int64_t workspace_bytes,
                              int32_t *status, int32_t *hit_count, int32_t n_count_masks, uint32_t *removed_bits, int64_t removed_words,
                              cm3d_stream_t stream);

/* f1 for batches whose masks have DIFFERENT IMAGE SIZES (Waymo: 1920x1280 and 1920x886 images in one frame, thumbnailed per image
 * by the mask producer; the reference decodes every mask at its own size, src/waymo/2d_to_3d.py:520-521, and tests points against
 * that mask's own shape, :600-606).  W, H is the batch's CANVAS -- the elementwise maximum of the masks' sizes -- and what every
 * later stage (cm3d_project_hits, ...) is called with; mask m's run list covers its own image of (w, h) = mask_wh[m].
 *  mask_wh  int32[n][2]  w, h of each mask's own image, 1 <= w <= W, 1 <= h <= H (values outside are clamped into that range on
 *           the device: no table content moves a write outside the mask's slot).  A run list that overruns w*h is cut off at
 *           row h-1, like cm3d_rle_erode_pack cuts one at H-1.
 * RULE R: the result is what cm3d_rle_erode_pack stores for the mask pasted top-left into a W x H canvas of zeros -- pixels
 * outside w x h but inside the canvas are zeros, pixels outside the canvas are ignored as before.  The in-mask lists that follow
 * equal the reference's: it can only hit pixels 1 <= floor(u) <= w-2, 1 <= floor(v) <= h-2 (its in-image test and its
 * floor != 0 quirk), whose 3x3 neighbourhoods lie inside the mask's own image, so that its border rule and the canvas's never
 * differ there; and where w < W the canvas's column w-1 has zero neighbours and erodes to zero (rows h-1 likewise), so that
 * nothing the canvas-sized in-image test admits beyond the reference's can be hit.
 * `packed`, `bbox` and the never-written words are as described at cm3d_erode_pack, slots of H*Wp words of the CANVAS; argument
 * checks as cm3d_rle_erode_pack's, for the canvas.  The run lists are read as the producer wrote them: nothing is re-encoded. */
int cm3d_rle_erode_pack_sized(const uint32_t *rle_counts, const int32_t *rle_off, int32_t n_masks, int32_t total_runs,
                              int32_t W, int32_t H, const int32_t *mask_wh, uint32_t *packed, int32_t *bbox, void *workspace,
                              int64_t workspace_bytes, cm3d_stream_t stream);

/* cm3d_rle_erode_pack_sized carrying the per-pass reset, as cm3d_rle_erode_pack_begin does for cm3d_rle_erode_pack. */
int cm3d_rle_erode_pack_sized_begin(const uint32_t *rle_counts, const int32_t *rle_off, int32_t n_masks, int32_t total_runs,
                                    int32_t W, int32_t H, const int32_t *mask_wh, uint32_t *packed, int32_t *bbox, void *workspace,
                                    int64_t workspace_bytes, int32_t *status, int32_t *hit_count, int32_t n_count_masks,
                                    uint32_t *removed_bits, int64_t removed_words, cm3d_stream_t stream);

/* ---- a4-a7: projection + in-image + in-mask test ----------------------------
 * Replaces the per-mask block 2d_to_3d.py:553-613 (clone, 2x translate/rotate,
 * view_points, in-image test, floor, mask gather incl. the floor(u)!=0 && floor(v)!=0
 * quirk) for ALL masks of ALL frames in one pass over the points.
 *  cams  float[F][n_cams][CM3D_CAM_STRIDE]: up to three rigid stages, each `p += t_pre; p = R p; p += t_post`
 *        (either translation optional), then K':
 *        stage s at [15s .. 15s+14] = t_pre(3), R(9, row-major), t_post(3);  [45..53] K' (3x3);
 *        [54] number of stages (2 nuScenes :569-577, 1 Waymo src/waymo/2d_to_3d.py:575-576,
 *        3 KITTI src/kitti/2d_to_3d.py:1238-1240 = ref->velo, velo->ref, ref->rect);
 *        [55] flags: bit 2s = stage s has t_pre, bit 2s+1 = stage s has t_post.
 *        All float32 exactly as the reference hands them to translate/rotate/matmul/view_points.
 *  hit_words uint32[planes][n_points_total] OUT, planes = (max masks per frame + 31)/32;
 *        bit (k&31) of hit_words[k>>5][p] = point p lies in mask mask_off[f]+k.  An intermediate for cm3d_compact_hits:
 *        written per block of 256 consecutive rows of a frame, and only for blocks that hold at least one in-mask point
 *        (the per-block flags travel in the workspace); the words of the other blocks keep what the buffer held before
 *  hit_count int32[n_masks] IN/OUT accumulated with atomics; zeroed by cm3d_batch_begin
 *  workspace: cm3d_project_workspace_bytes(F, max_pts_per_frame, planes), 16-byte aligned; it receives the per-frame
 *        tables and the per-(256-row chunk, mask) hit counts and must be handed unchanged to cm3d_compact_hits
 *  ev_start, ev_stop: optional hipEvent_t (NULL = none), recorded on `stream` right before and after the projection
 *        kernel itself -- behind the small per-frame table kernel the call launches first -- for callers that time it */
int64_t cm3d_project_workspace_bytes(int32_t n_frames, int32_t max_pts_per_frame, int32_t planes);
/* Accounting aid for bench.py's byte counts (nothing on the path calls it; synchronous): rows of the batch that lie in a block of
 * 256 rows with at least one in-mask point, read back from the workspace of the last cm3d_(sweep_)project_hits on `stream`. */
int cm3d_project_hit_rows(const void *workspace, int64_t workspace_bytes, int32_t n_frames, int32_t max_pts_per_frame,
                          int32_t planes, int64_t *rows_out, cm3d_stream_t stream);
/* Accounting aid for the tests of the per-camera culling (nothing on the path calls it; synchronous): what the per-frame table
 * kernel of the last cm3d_(sweep_)project_hits on `stream` decided, read back from the workspace.
 *  out  int32[n_frames][8]: [0] bit c = camera c has an approximate projection, [1] bit c = camera c has a non-empty mask,
 *       [2] the frame's pixel margin (largest of its cameras'), [3] the smallest depth the approximate projection may accept
 *       (float bits; smallest of the cameras'), [4] bit c = camera c has a view wedge (0: every point is projected exactly),
 *       [5..7] zero. */
int cm3d_project_culling(const void *workspace, int64_t workspace_bytes, int32_t n_frames, int32_t max_pts_per_frame,
                         int32_t planes, int32_t *out, cm3d_stream_t stream);
/* Accounting aid for the tests of the view wedges (added within ABI v5: a new symbol, no existing call changes; nothing on the
 * path calls it; synchronous): the planes the per-frame table kernel of the last cm3d_(sweep_)project_hits on `stream` wrote.
 * A camera's wedge is two planes through its centre; a point p (global) is looked at for that camera only while
 * min(n_L . p + d_L, n_R . p + d_R) >= 0.  The planes stand on a pixel-column interval [u_lo, u_hi]: the hull of the columns of
 * the camera's non-empty eroded masks in this frame, [min bb.x - pad, max bb.z + 1 + pad] clamped to [0, W], where pad is the
 * camera's pixel bound on the exact chain's column (at least 1 + ceil(2 max(fx, fy) delta / zmin)); the whole image, [0, W], for
 * a camera without such a bound (zmin <= 0.1, a composition that is not a rotation to 1e-5) or without a non-empty mask.  The
 * wedge only ever culls work: no point outside the columns of a camera's masks can land in one of them.
 *  out  float[n_frames][CM3D_MAX_CAMS][8]: n_L (unit, 3), d_L + margin, n_R (3), d_R + margin.  A record the derivation does not
 *       cover (skew, a non-trivial last row of K', stages that are not rigid) reads (0, 0, 0, 1) twice -- every point is inside --,
 *       a slot beyond n_cams (0, 0, 0, -1) twice -- none is. */
int cm3d_project_wedges(const void *workspace, int64_t workspace_bytes, int32_t n_frames, int32_t max_pts_per_frame,
                        int32_t planes, float *out, cm3d_stream_t stream);
int cm3d_project_hits(const float *points, const int32_t *pt_off, int32_t n_frames, int32_t max_pts_per_frame,
                      int32_t n_points_total, const float *cams, int32_t n_cams, const int32_t *mask_off,
                      const int32_t *mask_cam, const int32_t *bbox, const uint32_t *packed, int32_t n_masks,
                      int32_t W, int32_t H, float min_dist, int32_t planes, uint32_t *hit_words,
                      int32_t *hit_count, int32_t *status, void *workspace, int64_t workspace_bytes,
                      void *ev_start, void *ev_stop, cm3d_stream_t stream);

/* a2 + a4-a7 in one launch: cm3d_sweep_prep folded into cm3d_project_hits.  The kernel reads the raw sweep rows,
 * applies the ego-box drop and the sensor -> ego -> global chains (2d_to_3d.py:437-465) on the fly, writes pt_off, the
 * removed-row bits and status[1] exactly as cm3d_sweep_prep does, and produces hit_words / hit_count exactly as
 * cm3d_project_hits does.  `points` is OPTIONAL: NULL = the transformed cloud is not materialised at all (the later stages
 * only need the in-mask points, which cm3d_compact_hits re-derives from the raw rows into hit_xyz); non-NULL = the cloud
 * is also written, bit for bit what cm3d_sweep_prep writes.  max_sweeps_per_frame (host-side knowledge of
 * frame_sweep_off) must be <= 16; use the two separate calls otherwise.  Arguments as in cm3d_sweep_prep and
 * cm3d_project_hits.  Rows of 4 or 5 floats (the reference's .bin layouts) and the quad layout have their own instantiations. */
#define CM3D_MAX_FUSED_SWEEPS 16
/* How much of the chip one projection launch takes (process-wide; r04).  0 (the default): as many workgroups as fit minus one per
 * CU -- the fastest launch when nothing else runs.  n >= 1: n workgroups per CU.  A caller that keeps several batches in flight on
 * streams of their own (cm3d_amd.lifting.LiftPipeline) asks for 2: the launch alone takes 62 instead of 52 us on the headline shape, but
 * the kernels of the other batches run beside it instead of behind it (three batches in flight: +1-2 % frames/s on C2, C1 and C4).
 * Returns the previous value.  Results do not depend on it.  (Honoured by the launch for frames of up to 32 masks on the quad layout, the one the
 * other batches' kernels queue behind; the multi-plane launch keeps its grid.) */
int cm3d_project_workgroups_per_cu(int32_t n);

int cm3d_sweep_project_hits(const float *raw, int32_t raw_stride, const float *intensity, const int32_t *sweep_row_off, int32_t n_sweeps,
                            int32_t max_sweeps_per_frame, const float *sweep_xf, const int32_t *frame_sweep_off,
                            float halfw, float *points, int32_t pt_cap, int32_t *pt_off, uint32_t *removed_bits,
                            int32_t n_frames, int32_t max_pts_per_frame, int32_t n_points_total,
                            const float *cams, int32_t n_cams, const int32_t *mask_off, const int32_t *mask_cam,
                            const int32_t *bbox, const uint32_t *packed, int32_t n_masks, int32_t W, int32_t H,
                            float min_dist, int32_t planes, uint32_t *hit_words, int32_t *hit_count, int32_t *status,
                            void *workspace, int64_t workspace_bytes, void *ev_start, void *ev_stop, cm3d_stream_t stream);

/* ---- a7-a8: ordered compaction of the hits ----------------------------------
 * Replaces torch.where + the two .cpu() index-tracking steps at 2d_to_3d.py:606,613-617.
 *  removed_bits  from cm3d_sweep_prep / cm3d_sweep_project_hits (NULL when the points were not produced by them)
 *  raw, raw_stride, intensity, sweep_xf  the raw rows the fused launch read (NULL when `points` is given)
 *  points   float[pt_cap][4] the transformed cloud, or NULL when it was not materialised
 *  hit_off  int32[n_masks+1] OUT exclusive scan of hit_count
 *  tile_off int32[n_masks+1] OUT exclusive scan of ceil(hit_count/CM3D_MEDOID_TILE)
 *  hit_idx  int32[idx_cap]   OUT ascending point indices of mask m at [hit_off[m], hit_off[m+1]): indices into the
 *                                frame's cloud WITHOUT the dropped rows, i.e. the reference's track_points
 *  hit_row  int32[idx_cap]   OUT, optional: the same points as frame-local row indices
 *  hit_xyz  float[idx_cap][4] OUT, optional: global-frame x,y,z,intensity of every listed point (the gather of :620),
 *                                laid out like hit_idx; from `points` when given, else from the raw rows through the
 *                                very fma chains of the sweep preparation (bit-identical)
 *  tile_work OUT, optional (may be NULL): cm3d_tile_work_bytes(n_masks, idx_cap) bytes; the work list of
 *            cm3d_medoid (one record per medoid tile, longest lists first), built beside the compaction
 *  workspace: the buffer cm3d_project_hits / cm3d_sweep_project_hits filled (per wave-chunk: hit counts per mask, whether it
 *            holds a hit at all, dropped rows; their sums over groups of 16 wave-chunks; in-mask points per frame)
 * Two launches, no scan kernel: the compaction computes its own output offsets from those counts, never reads the hit words of a
 * wave-chunk without a hit, builds hit_off / tile_off / tile_work in the same launch, and leaves (row, sweep) tags in hit_xyz;
 * a one-thread-per-point launch then fetches and transforms the listed rows (all gathers in flight at once). */
int cm3d_compact_hits(const uint32_t *hit_words, int32_t planes, int32_t n_frames, int32_t max_pts_per_frame,
                      int32_t n_points_total, const int32_t *mask_off, int32_t n_masks, const int32_t *hit_count,
                      const uint32_t *removed_bits, const float *raw, int32_t raw_stride, const float *intensity, const float *sweep_xf,
                      const float *points, int32_t *hit_off, int32_t *tile_off, int32_t *hit_idx, int32_t *hit_row,
                      float *hit_xyz, int32_t idx_cap, int32_t *tile_work, int32_t *status, void *workspace,
                      int64_t workspace_bytes, cm3d_stream_t stream);
int64_t cm3d_tile_work_bytes(int32_t n_masks, int32_t idx_cap);

/* ---- a9: medoid --------------------------------------------------------------
 * Replaces get_medoid (2d_to_3d.py:116-119) + the gather at :620,645-647:
 * argmin_j sum_i cdist(P,P)[i][j] with torch.cdist's float32 arithmetic (direct form
 * for <=25 points, matmul expansion otherwise), rows summed in ascending i, first minimum.
 *  points / pt_off / mask_frame / hit_row: either the cloud, the frames' first rows, the frame of every mask and the
 *             row-index list of cm3d_compact_hits (gathers go through it) -- or hit_row = NULL and `points` = the hit_xyz
 *             array of cm3d_compact_hits (float[idx_cap][4], laid out like hit_idx; pt_off and mask_frame are then unused
 *             and may be NULL): the in-mask points are then read as contiguous runs
 *  tile_work  the work list cm3d_compact_hits wrote for the same hit_off / tile_off, or NULL (then it is built here,
 *             one more launch)
 *  medoid_pos int32[n_masks]    OUT position in the mask's index list (-1 if the list is empty)
 *  centroid   float[n_masks][3] OUT global-frame xyz of the medoid point
 *  colsum_opt float[idx_cap] OUT, optional (may be NULL): every column sum, laid out like hit_idx.  When NULL, lists of
 *             more than 256 points (in a batch whose longest list has more than 448) are settled in two passes (approximate sums for all columns, exact float32 sums only
 *             for the columns a proven error bound cannot exclude): the same position, less work
 *  workspace: cm3d_medoid_workspace_bytes(n_masks, idx_cap) */
int64_t cm3d_medoid_workspace_bytes(int32_t n_masks, int32_t idx_cap);
int cm3d_medoid(const float *points, const int32_t *pt_off, const int32_t *mask_frame, int32_t n_masks,
                const int32_t *hit_off, const int32_t *tile_off, const int32_t *hit_row, int32_t idx_cap,
                const int32_t *tile_work, int32_t *medoid_pos, float *centroid, float *colsum_opt, void *workspace,
                int64_t workspace_bytes, cm3d_stream_t stream);
/* The same with a hint and a feedback word (ABI v3), for callers that run batch after batch:
 *  flags     bit 0: expect no list of more than 448 points in this batch -- every list then takes the exact one-pass route and the two
 *            launches of the two-pass route that would find nothing to do are not made.  Only ever a matter of time: the one-pass
 *            route is exact for every length.
 *  feedback  optional int32[1] the DEVICE can write (device memory, or page-locked host memory that is mapped into the device's address
 *            space: then the caller reads it without a copy): 1 if this batch holds such a list, else 0, written by the first launch.
 *            cm3d_amd.lifting.LiftEngine feeds it back as the next pass's flag. */
int cm3d_medoid2(const float *points, const int32_t *pt_off, const int32_t *mask_frame, int32_t n_masks,
                 const int32_t *hit_off, const int32_t *tile_off, const int32_t *hit_row, int32_t idx_cap,
                 const int32_t *tile_work, int32_t *medoid_pos, float *centroid, float *colsum_opt, void *workspace,
                 int64_t workspace_bytes, int32_t flags, int32_t *feedback, cm3d_stream_t stream);

/* Diagnostic for the tests: `count` pseudo-random (numerator, denominator) pairs, denominators over the projection
 * kernel's shortcut domain [1e-30, 1e30), quotients next to integers over-represented, through the kernel's division
 * sequence and through the IEEE division; n_bad (device, 2 words): [0] = differing quotients q with 1/8 <= |q| < 2^96
 * (must be 0), [1] = differing quotients with |q| < 1/8 in both forms (numerators below 2^-103; the pixel range test
 * rejects those points whatever the low bits are). */
int cm3d_selftest_div(uint64_t seed, uint64_t count, uint64_t *n_bad, cm3d_stream_t stream);

/* Diagnostic for the tests: the first pass over long medoid lists takes its squared distances from the matrix pipe
 * (three v_mfma_f32_32x32x2_f32 = the reference's five-term fma chain).  2048 waves x tiles_per_wave tiles of 32 x 32 pairs of
 * pseudo-random points at global-frame magnitudes through the MFMAs and through the vector fma chain; *n_bad (device) = values
 * that differ in any bit (must be 0). */
int cm3d_selftest_mfma(uint64_t seed, int32_t tiles_per_wave, uint64_t *n_bad, cm3d_stream_t stream);

/* Diagnostic for the tests: runs every float32 bit pattern in [first_bits, last_bits] (positive values) that lies in
 * the medoid kernel's fast-path domain [1e-30, 1e30) through the kernel's square root, its reference form and sqrtf();
 * *n_bad (device) = number of values on which the three are not bit-identical, *first_bad = smallest such pattern. */
int cm3d_selftest_sqrt(uint32_t first_bits, uint32_t last_bits, uint64_t *n_bad, uint32_t *first_bad, cm3d_stream_t stream);

/* ---- a10: nearest lane point --------------------------------------------------
 * Replaces lane_yaws_distances_and_coords (2d_to_3d.py:277-302): float64 Euclidean
 * distance on (x,y) between float32-rounded centroids and lane points, first minimum.
 *  lane      float[L_total][3]  x,y,yaw (float32-rounded, as torch.Tensor(...) does at :278)
 *  lane_off  int32[T+1]         lane tables back to back
 *  frame_lane int32[F]          table of each frame, in [0, T) (T = 1: every frame is on table 0; the search reads neither
 *                               frame_lane nor mask_frame then)
 *  lane_idx  int32[n_masks] OUT index into the frame's table (-1 for masks without centroid)
 *  lane_dist double[n_masks] OUT
 *  Exactly the brute-force result (first minimum of the float64 distance); internally the lane points are
 *  binned into a uniform grid per table (cm3d_lane_grid_build) and searched in growing rings, one wave per
 *  centroid; centroids farther than ~10 cells from every lane fall back to a brute-force kernel.
 *  grid: the buffer cm3d_lane_grid_build filled; workspace: cm3d_lane_nn_workspace_bytes(n_masks) bytes, reserved
 *  (centroids the grid search cannot settle are scanned against their whole table by the same wave) */
/* Spatial index of the lane tables (uniform grid per table, points in cell order): built by one
 * workgroup per table; depends only on the lane tables, so a driver may build it on a side stream. */
int64_t cm3d_lane_grid_bytes(int32_t n_tables, int32_t n_lane_points);
int cm3d_lane_grid_build(const float *lane, const int32_t *lane_off, int32_t n_tables, int32_t n_lane_points, void *grid,
                         int64_t grid_bytes, cm3d_stream_t stream);
int64_t cm3d_lane_nn_workspace_bytes(int32_t n_masks);
int cm3d_lane_nn(const float *centroid, const int32_t *medoid_pos, const int32_t *mask_frame, int32_t n_masks,
                 const float *lane, const int32_t *lane_off, const int32_t *frame_lane, int32_t n_tables,
                 int32_t n_lane_points, const void *grid, int32_t *lane_idx, double *lane_dist, void *workspace,
                 int64_t workspace_bytes, cm3d_stream_t stream);

/* ---- a11-a15: box assembly + class-aware circle NMS ----------------------------
 * Replaces stage 2 (2d_to_3d.py:745-817: shape prior, lane-yaw rotation, push_centroid
 * :164-198) and circle_nms (:309-332 with the thresholds of :850-861).
 *  class_id int32[n_masks] index into the class tables; score double[n_masks]
 *  prior_wlh double[n_classes][3]; is_vehicle int32[n_classes] (pushed classes, :763);
 *  nms_group int32[n_classes] NMS label of each class (the class itself for nuScenes, the Waymo type
 *  for Waymo, src/waymo/cfg/prompt_cfg.py:286-297); nms_thr double[] squared-distance threshold per NMS label
 *  ego_xyz double[F][3]   LIDAR_TOP ego_pose translation of each frame (:793-795)            (nuScenes mode)
 *  pose_inv float[F][16]  NULL for nuScenes.  Waymo mode (a17, src/waymo/2d_to_3d.py:812-816,978-1001):
 *        inverse of the float32 frame pose; centroids are global, the kernel maps them back to the vehicle
 *        frame in float64, pushes with ego_frame=True and emits the heading instead of a quaternion.
 *  box   double[n_masks][CM3D_BOX_STRIDE] OUT: tx,ty,tz, qw,qz (rotation = [qw,0,0,qz]; Waymo: heading,0),
 *        lane yaw, lane dist, score, class id, flags -- the fixed-size record that the multi-GPU gather ships
 *  flags int32[n_masks] OUT: bit0 box exists (mask had points), bit1 box survives NMS */
int cm3d_box_nms(const float *centroid, const int32_t *medoid_pos, const int32_t *mask_off, int32_t n_frames,
                 int32_t n_masks, const int32_t *class_id, const double *score, const float *lane,
                 const int32_t *lane_off, const int32_t *frame_lane, const int32_t *lane_idx,
                 const double *lane_dist, const double *prior_wlh, const int32_t *is_vehicle,
                 const int32_t *nms_group, const double *nms_thr, int32_t n_classes, const double *ego_xyz,
                 const float *pose_inv, double *box, int32_t *flags, cm3d_stream_t stream);
/* The same for a caller that knows max_masks_per_frame, the most masks a frame of the batch has (added within ABI v5): the launch
 * takes its LDS by that bound instead of by CM3D_MAX_MASKS_PER_FRAME -- none up to 64, where a frame's NMS runs in one wave's
 * registers -- and finds room beside the kernels of other passes sooner.  A frame with more masks than the bound gets, for the masks
 * beyond it, the record of a mask without points (flags 0).  cm3d_box_nms is this call with CM3D_MAX_MASKS_PER_FRAME. */
int cm3d_box_nms_bounded(const float *centroid, const int32_t *medoid_pos, const int32_t *mask_off, int32_t n_frames,
                         int32_t n_masks, const int32_t *class_id, const double *score, const float *lane,
                         const int32_t *lane_off, const int32_t *frame_lane, const int32_t *lane_idx,
                         const double *lane_dist, const double *prior_wlh, const int32_t *is_vehicle,
                         const int32_t *nms_group, const double *nms_thr, int32_t n_classes, const double *ego_xyz,
                         const float *pose_inv, int32_t max_masks_per_frame, double *box, int32_t *flags, cm3d_stream_t stream);

/* a17 (Waymo): medoid in the vehicle frame -> global frame, float32 rotate then translate
 * (src/waymo/2d_to_3d.py:684-690).  pose_rt float[F][12]: [0..8] rotation row-major, [9..11] translation. */
int cm3d_centroid_transform(const float *centroid_in, const int32_t *medoid_pos, const int32_t *mask_frame,
                            int32_t n_masks, const float *pose_rt, float *centroid_out, cm3d_stream_t stream);

/* circle_nms alone (2d_to_3d.py:309-332) on float64 centres: boxes [frame_off[f], frame_off[f+1]) form
 * one sample; keep[i] = 1 for the survivors.  Order: descending score, ties by descending index. */
int cm3d_circle_nms(const double *x, const double *y, const double *score, const int32_t *label,
                    const int32_t *frame_off, int32_t n_frames, const double *nms_thr, int32_t n_classes,
                    int32_t *keep, cm3d_stream_t stream);

/* ---- opt-in: greedy NMS on the bird's-eye-view overlap of the rotated boxes (added within ABI v5) ----------------
 * In place of circle_nms's centre distance: the rotated-rectangle nms(rrects, scores, ...) the reference carries as dead code
 * (src/kitti/2d_to_3d.py:359-599; strict > at :596, nms_threshold 0.4 at :531-534), with the float64 clip of cm3d_bev_match as the
 * overlap instead of its rasterised polygons.  cm3d_amd/nms.py (rotated_nms_host) states the rule to the bit:
 *  order: descending score, ties by descending index; the box of rank r, unless suppressed, is kept and suppresses every
 *  later-ranked, not yet suppressed box j with (class_agnostic || group[j] == group[i]) and measure(i, j) > thr[group[j]].
 *  measure 0 "iou":   the bird's-eye-view IoU of cm3d_bev_match (0 when either area is not positive, at most 1);
 *  measure 1 "cover": intersection area / (length_j * width_j), at most 1: the share of the lower-scored box the kept one covers
 *        (the reference's ratio).  In both the kept box is the one the clip's coordinates are relative to.
 *  A box whose float64 area is not positive or whose centre is not finite neither suppresses nor is suppressed.  Scores are finite.
 *  rec   double[n][6]  cx, cy, length, width, cos(heading), sin(heading) -- the record of cm3d_bev_match
 *  group int32[n] NMS group of each box (outside [0, n_groups): 0); thr double[n_groups]
 *  frame_off int32[F+1]: boxes [frame_off[f], frame_off[f+1]) form one frame (an empty frame is legal); the boxes of a frame beyond
 *        its CM3D_MAX_MASKS_PER_FRAME-th get keep 0
 *  keep  int32[n] OUT, written whole: 1 for the survivors */
int cm3d_rotated_nms(const double *rec, const double *score, const int32_t *group, const int32_t *frame_off, int32_t n_frames,
                     const double *thr, int32_t n_groups, int32_t measure, int32_t class_agnostic, int32_t *keep,
                     cm3d_stream_t stream);
/* The same behind the box launch of a pass (cm3d_box_nms / cm3d_box_nms_bounded), on the `box` rows and `flags` it wrote: only boxes with
 * flags & 1 take part; bit 1 of `flags` and column 9 of `box` are rewritten for EVERY mask of the batch (nothing of the circle NMS's
 * decision remains), nothing else is touched.  The record of a box is built from stored values only: cx, cy = box[0], box[1];
 * class = box[8] (what the box launch stored of class_id, which is only checked here); length = prior_wlh[3 * class + 1],
 * width = prior_wlh[3 * class + 0] (the [w, l, h] table: length along the heading); nuScenes (waymo == 0): the axis of the rotation
 * [qw, 0, 0, qz], c = qw * qw - qz * qz, s = 2 * qw * qz, every product and the difference rounded on their own (a box of a class
 * that is not rotated is the axis-aligned rectangle its record describes); Waymo (waymo != 0): c, s = cos, sin of box[3] in
 * float64.  group = nms_group[class], score = box[7].  max_masks_per_frame as in cm3d_box_nms_bounded: the launch's LDS is sized
 * by it (none up to 64), and the masks of a frame beyond it -- which that launch gave flags 0 -- take no part. */
int cm3d_box_rotated_nms(double *box, int32_t *flags, const int32_t *mask_off, int32_t n_frames, int32_t n_masks,
                         const int32_t *class_id, const double *prior_wlh, const int32_t *nms_group, int32_t n_classes,
                         const double *thr, int32_t n_groups, int32_t measure, int32_t class_agnostic, int32_t waymo,
                         int32_t max_masks_per_frame, cm3d_stream_t stream);

/* ---- f4: box matching of the SAM3D fusion step ------------------------------------
 * Replaces `match(pred_boxes, sam3d_boxes, 0.2, Type.TYPE_2D)` of src/nuscenes/linear_matching.py:53-121,
 * called per sample at :231-259 (src/waymo/linear_matching.py:251-283 alike): waymo_open_dataset's
 * py_metrics_ops.match with TYPE_HUNGARIAN -- bird's-eye-view IoU of rotated rectangles, quantised to
 * integers (x 1e6), maximum-weight assignment, pairs with IoU < iou_thr dropped.  All samples in one call.
 *  pred  double[n_pred][6]  cx, cy, length, width, cos(heading), sin(heading) -- the float32-rounded box
 *        values of `tf.convert_to_tensor(..., dtype=float)` (:248-249) widened to double; a box with
 *        length*width == 0 is "no box" (:65) and never matches
 *  pred_off int32[F+1], gt_off int32[F+1]   sample f owns pred [pred_off[f], pred_off[f+1]) and
 *        gt (SAM3D) boxes [gt_off[f], gt_off[f+1]); at most CM3D_MAX_MATCH_BOXES per sample and side
 *        (status bit0 is set and the sample left unmatched otherwise)
 *  pair_off int64[F+1]      prefix sums of P_f * G_f; total_pairs = pair_off[F]
 *  pred_match int32[n_pred] OUT: index of the matched gt box inside its sample, or -1
 *  gt_match   int32[n_gt]   OUT: index of the matched prediction inside its sample, or -1
 *  match_iou  double[n_pred] OUT: IoU of the match (0 when unmatched)
 *  status int32[1] (zero it before the call); workspace: cm3d_bev_match_workspace_bytes(total_pairs) */
int64_t cm3d_bev_match_workspace_bytes(int64_t total_pairs);
int cm3d_bev_match(const double *pred, const int32_t *pred_off, int32_t n_pred, const double *gt,
                   const int32_t *gt_off, int32_t n_gt, const int64_t *pair_off, int32_t n_frames,
                   int64_t total_pairs, double iou_thr, int32_t *pred_match, int32_t *gt_match, double *match_iou,
                   int32_t *status, void *workspace, int64_t workspace_bytes, cm3d_stream_t stream);

/* ---- a18 (KITTI, ABI v5): yaw of the oriented bounding box of every mask ------------
 * Replaces the per-mask Open3D box of src/kitti/2d_to_3d.py:855-876 (get_oriented_bounding_box: PCA of the convex-hull
 * vertices) and the yaw taken from it at :1524 (Rotation.from_matrix(R).as_euler("zyx")[0]), host restatement
 * cm3d_amd.kitti.obb_yaw.  One launch for all masks, one workgroup of one wave per mask, float64 throughout on coordinates shifted
 * to the list's AABB centre:
 *   1. hull vertices = the extreme points of the list (Qhull's ConvexHull(p).vertices: a point on a face or an edge that is no
 *      corner is no vertex, a vertex listed several times counts once; outside tolerance 16 DBL_EPSILON x half the list's extent);
 *      a flat, collinear or single-point list has no hull (Qhull raises; the reference falls back to the identity box, :1481-1484);
 *   2. mean and population covariance of the vertices (a fixed summation order: the same bits on every run);
 *   3. 3x3 eigen-solve (cyclic Jacobi), columns by descending eigenvalue.  The signs of the eigenvectors are an implementation
 *      detail of LAPACK / Open3D; here each unit eigenvector is negated if needed so that its component of largest magnitude is
 *      positive (the first one on an exact tie) -- cm3d_amd.kitti.obb_canonical restates this rule on the host.  det < 0: column 2
 *      negated;
 *   4./5. extents = max - min of all points; columns re-ordered as [rank z, rank y, rank x] of the stable ascending sort of the
 *      extents; det < 0: column 0 negated;
 *   6. yaw = scipy's as_euler('zyx')[0] of that matrix (quaternion method, gimbal-lock branch included).
 *  hit_xyz   float[idx_cap][4]  the compaction's in-mask points (cm3d_compact_hits), mask m at [hit_off[m], hit_off[m+1])
 *  hit_off   int32[n_masks+1]
 *  yaw       double[n_masks] OUT   obb_status int32[n_masks] OUT:
 *              0 fitted; 1 three points or fewer, skipped (:1479-1480), yaw NaN; 2 no hull (flat / collinear / one distinct
 *              point), yaw 0.0 and rot = identity; 4 the construction could not go on (more than 512 facets seen from one
 *              point, or a numerically degenerate new facet), yaw NaN -- nothing is written out of range.  The workspace holds every
 *              hull a list can have: no list fails for lack of room
 *  rot_opt   double[n_masks][9] OUT, optional (NULL): the final row-major matrix (NaN for status 1 and 4)
 *  vertex_opt uint8[idx_cap] OUT, optional (NULL): laid out like hit_xyz, 1 at the list positions of the hull vertices (the first
 *              position of a repeated vertex that the construction reached), else 0
 *  workspace: cm3d_obb_workspace_bytes(n_masks, idx_cap) = 8 idx_cap + 48 (3 idx_cap + 64 n_masks) bytes, 8-byte aligned: 8 bytes per
 *             list position (live points) and, for the hulls too large for LDS, a region of 3 n + 64 facets per list of n points at
 *             facet 3 hit_off[m] + 64 m (room for any hull of the list; placed by the offsets, so results never depend on the order
 *             in which masks run).  hit_off must be non-decreasing, as cm3d_compact_hits writes it */
int64_t cm3d_obb_workspace_bytes(int32_t n_masks, int32_t idx_cap);
int cm3d_obb(const float *hit_xyz, const int32_t *hit_off, int32_t n_masks, int32_t idx_cap, double *yaw, int32_t *obb_status,
             double *rot_opt, uint8_t *vertex_opt, void *workspace, int64_t workspace_bytes, cm3d_stream_t stream);

/* Diagnostic for the tests: the yaw step of cm3d_obb alone -- as_euler('zyx')[0] of n row-major 3x3 rotation matrices R
 * (double[n][9]) into yaw (double[n]). */
int cm3d_selftest_obb_yaw(const double *R, int32_t n, double *yaw, cm3d_stream_t stream);

/* ---- Waymo 3D detection metrics: the counting of waymo-open-dataset's compute_detection_metrics_main --------
 * The host side (cm3d_amd/waymo_eval.py) groups the boxes of a file pair and turns the counts into mAP / mAPH.
 * A group is (frame, type 1..4, shard): shard 0 holds every box of the type, shards 1..3 the boxes whose centre lies
 * [0, 30), [30, 50), [50, +inf) m from the origin; its breakdown is group_bd = (type - 1) * 4 + shard.  Group g owns
 * predictions [pred_off[g], pred_off[g+1]) in descending score order and ground truth [gt_off[g], gt_off[g+1]).
 * Per group and cutoff c (float32(c * 0.01), c = 0..100) the predictions with score >= cutoff are matched one to one
 * with the group's ground truth: maximum-weight assignment on int(3D IoU x 1e6), pairs below the IoU threshold of the
 * type (vehicle 0.7, else 0.5) never match.  One solve per group serves every cutoff (rows are added in score order);
 * per_cutoff != 0 solves each cutoff on its own instead (same counts; for tests).
 *  pred_box, gt_box double[n][CM3D_WM_BOX_STRIDE]  cx, cy, length, width, cos(heading), sin(heading), cz, height
 *  pred_heading, gt_heading float[n]  heading (float32) for the heading accuracy 1 - |d| / pi, d wrapped to [-pi, pi]
 *  pred_score float[n_pred]; gt_level int32[n_gt] 1 or 2
 *  pair_off int64[n_groups+1]  prefix sums of P_g * G_g; total_pairs = pair_off[n_groups]
 *  counts int64[CM3D_WM_BREAKDOWNS][CM3D_WM_CUTOFFS][4] OUT: TP, FP, FN at LEVEL_1, FN at LEVEL_2 (written whole: the call
 *        zeroes them first); a prediction matched to LEVEL_2 ground truth is a TP at LEVEL_1 too
 *  heading_sum int64[CM3D_WM_BREAKDOWNS][CM3D_WM_CUTOFFS] OUT: heading accuracy of the TPs, in 2^-32 units
 *  status int32[1] (zero it before the call): bit0 a group with more than CM3D_MAX_MATCH_BOXES boxes on a side, bit1 a
 *        group_bd outside [0, CM3D_WM_BREAKDOWNS) -- such a group is skipped, nothing is written out of range
 *  workspace: cm3d_waymo_metrics_workspace_bytes(total_pairs).  Integer atomics only: every run gives the same bits. */
int64_t cm3d_waymo_metrics_workspace_bytes(int64_t total_pairs);
int cm3d_waymo_metrics(const double *pred_box, const float *pred_heading, const float *pred_score, const int32_t *pred_off,
                       const double *gt_box, const float *gt_heading, const int32_t *gt_level, const int32_t *gt_off,
                       const int32_t *group_bd, const int64_t *pair_off, int32_t n_groups, int64_t total_pairs,
                       int32_t per_cutoff, int64_t *counts, int64_t *heading_sum, int32_t *status, void *workspace,
                       int64_t workspace_bytes, cm3d_stream_t stream);

/* ---- Waymo metrics of every alpha of the SAM3D fusion grid search in one call --------
 * Added within ABI v5: two new symbols, no existing call changes, so CM3D_ABI_VERSION stays.
 * The fused file of src/waymo/linear_matching.py:335-470 differs between alphas only in scores and in which box of a matched pair
 * it holds, so the host (cm3d_amd/waymo_eval.pack_candidates) packs a CANDIDATE superset once and this call counts every alpha's
 * file from it.  Groups, breakdowns, ground truth, cutoffs, weights and matching are those of cm3d_waymo_metrics; candidates take
 * the place of the predictions.  Group g owns candidates [cand_off[g], cand_off[g+1]) in CANDIDATE ORDER (the order in which the
 * fused file lists the objects; the two candidates of a pair are neighbours).  For alpha a, with prod = s * a in double:
 *   kind 0  unmatched prediction        always active, score (float)p
 *   kind 1  unmatched SAM3D box         always active, score (float)clip(prod, 0, 1)
 *   kind 2  a pair's prediction box     active iff !(prod > p), score (float)p
 *   kind 3  a pair's SAM3D box          active iff prod > p, score (float)clip(prod, 0, 1)   (any other kind: never active)
 * The active candidates are ranked by descending score, ties by ascending position in the group (-0 equals +0) -- the order
 * waymo_eval.pack_arrays gives the decoded fused file -- and counted like the predictions of cm3d_waymo_metrics.
 *  cand_box double[n_cand][CM3D_WM_BOX_STRIDE], cand_heading float[n_cand]   as pred_box, pred_heading of cm3d_waymo_metrics
 *  cand_kind int32[n_cand]; cand_p, cand_s double[n_cand]   the prediction's and the SAM3D box's score (the one a kind lacks is ignored)
 *  cand_off int32[n_groups+1]; gt_box, gt_heading, gt_level, gt_off, group_bd as in cm3d_waymo_metrics
 *  pair_off int64[n_groups+1]  prefix sums of C_g * G_g (candidates x ground truth); total_pairs = pair_off[n_groups]
 *  group_static int32[n_groups]  non-zero: every candidate of the group is kind 0.  Such a group does not depend on alpha: it is
 *        solved once and its counts are added to every alpha (a non-zero flag on a group with other kinds gives that group's
 *        counts at alpha 0 everywhere)
 *  alphas double[n_alphas], 1 <= n_alphas <= CM3D_WM_SWEEP_MAX_ALPHAS (the caller hands a longer grid over in several calls)
 *  counts int64[n_alphas][CM3D_WM_BREAKDOWNS][CM3D_WM_CUTOFFS][4] OUT, heading_sum int64[n_alphas][CM3D_WM_BREAKDOWNS][CM3D_WM_CUTOFFS]
 *        OUT: per alpha what cm3d_waymo_metrics writes for that alpha's fused file (written whole)
 *  status int32[1] (zero it before the call): bit0 a group with more than CM3D_MAX_MATCH_BOXES ground-truth boxes or more than
 *        CM3D_MAX_MATCH_BOXES CANDIDATES (the ranking holds that many; a group whose active candidates would fit
 *        cm3d_waymo_metrics at every alpha while its superset does not is refused here -- score such a grid alpha by alpha),
 *        bit1 a group_bd outside [0, CM3D_WM_BREAKDOWNS) -- such a group is skipped, nothing is written out of range
 *  workspace: cm3d_waymo_metrics_sweep_workspace_bytes(total_pairs), 8-byte aligned.  The weights are computed once for all
 *        alphas; one wave per group and slice of the alphas ranks in LDS and solves.  Integer atomics only: every run gives the
 *        same bits. */
int64_t cm3d_waymo_metrics_sweep_workspace_bytes(int64_t total_pairs);
int cm3d_waymo_metrics_sweep(const double *cand_box, const float *cand_heading, const int32_t *cand_kind, const double *cand_p,
                             const double *cand_s, const int32_t *cand_off, const double *gt_box, const float *gt_heading,
                             const int32_t *gt_level, const int32_t *gt_off, const int32_t *group_bd, const int64_t *pair_off,
                             const int32_t *group_static, int32_t n_groups, int64_t total_pairs, const double *alphas,
                             int32_t n_alphas, int64_t *counts, int64_t *heading_sum, int32_t *status, void *workspace,
                             int64_t workspace_bytes, cm3d_stream_t stream);

/* ---- nuScenes detection matching for every alpha of the SAM3D fusion grid search in one call --------
 * Added within ABI v5: two new symbols, no existing call changes, so CM3D_ABI_VERSION stays.
 * The greedy matching of the reference's eval_custom.py (accumulate_object_class :542-706, accumulate_with_recall :709-864) only
 * ever pairs boxes of one sample, so the host (cm3d_amd/nusc_eval.pack) packs GROUPS -- one sample for the class-agnostic "object"
 * scoring, one (sample, class) for the class-aware one; the call does not know which -- and this call decides every group.  Group
 * g owns candidates [cand_off[g], cand_off[g+1]) in FILE ORDER and ground truth [gt_off[g], gt_off[g+1]).  A candidate's POSITION
 * is its index in the candidate arrays.  For alpha a, with prod = s * a (one float64 multiply):
 *   kind 0  unmatched prediction        always active, score p
 *   kind 1  unmatched SAM3D box         always active, score clip(prod, 0, 1)
 *   kind 2  a pair's prediction box     active iff !(prod > p), score p
 *   kind 3  a pair's SAM3D box          active iff prod > p, score clip(prod, 0, 1)       (any other kind: never active)
 * A plain result file is all kind 0 with one dummy alpha.  Per (group, alpha, threshold t), each threshold on its own: the active
 * candidates are walked by descending score (float64; -0 equals +0), equal scores by DESCENDING position -- Python's
 * sorted((score, index))[::-1] -- and each takes, among the group's ground-truth boxes nobody took before it, the one of smallest
 * d2 = dx * dx + dy * dy (dx = cand_x - gt_x, float64, no contraction; the lowest ground-truth index on equal d2) if
 * d2 < dist_th[t] * dist_th[t]; otherwise it is a false positive and takes nothing.  (The reference compares numpy's norm with
 * dist_th[t]: the two can differ only for a distance within an ulp of the threshold or of another distance)
 *  cand_xy double[n_cand][2]; cand_kind int32[n_cand]; cand_p, cand_s double[n_cand]   (the score a kind lacks is ignored)
 *  cand_off, gt_off int32[n_groups+1], non-decreasing, cand_off[n_groups] <= n_cand; gt_xy double[gt_off[n_groups]][2]
 *  alphas double[n_alphas], 1 <= n_alphas <= CM3D_NUSC_MAX_ALPHAS (the caller hands a longer grid over in several calls)
 *  dist_th double[n_th], 1 <= n_th <= CM3D_NUSC_MAX_TH
 *  tp_bits uint8[n_alphas][n_cand] OUT: bit t = true positive at threshold t, bit 7 = active at this alpha; 0 for an inactive
 *        candidate.  Every candidate of every group is written; candidates outside all groups are left alone.
 *  match_idx int32[n_alphas][n_cand][n_th] OUT or NULL: the group-local index of the box taken, -1 for none
 *  status int32[1] (zero it before the call): bit0 a group with more than CM3D_NUSC_MAX_CAND candidates or more than
 *        CM3D_NUSC_MAX_GT ground-truth boxes (or negative counts) -- such a group is skipped and nothing of it is written
 *  workspace: cm3d_nusc_match_workspace_bytes(...), which is 0 today (keys and permutation live in LDS; NULL is accepted then).
 *        No allocation inside the call; one launch, no atomics on the outputs: every run gives the same bytes. */
#define CM3D_NUSC_MAX_CAND 1024
#define CM3D_NUSC_MAX_GT 256
#define CM3D_NUSC_MAX_TH 4
#define CM3D_NUSC_MAX_ALPHAS 1024
int64_t cm3d_nusc_match_workspace_bytes(int32_t n_groups, int64_t n_cand, int32_t n_alphas);
int cm3d_nusc_match(const double *cand_xy, const int32_t *cand_kind, const double *cand_p, const double *cand_s,
                    const int32_t *cand_off, const double *gt_xy, const int32_t *gt_off, int32_t n_groups, int64_t n_cand,
                    const double *alphas, int32_t n_alphas, const double *dist_th, int32_t n_th, uint8_t *tp_bits,
                    int32_t *match_idx, int32_t *status, void *workspace, int64_t workspace_bytes, cm3d_stream_t stream);

/* ---- One pass over a resident batch in one call; passes of several batches on as many streams as the process has queues for ----
 * Added within ABI v5: new symbols only, no existing call changes, so CM3D_ABI_VERSION stays.  Host code (csrc/pipeline.cpp):
 * no kernel of its own.
 *
 * The descriptor holds what the calls of a pass take, under the names their declarations above use.  `size` is
 * sizeof(cm3d_lift_pass_desc): a caller built against another layout is refused (CM3D_ERR_ARG).  `points`, `intensity` and `colsum`
 * may be NULL as in those calls; with `points` NULL the compaction re-derives the in-mask points from the raw rows.  `centroid_g` is
 * what the lane search and the boxes read (without `pose_rt`: the same buffer as `centroid`). */
typedef struct cm3d_lift_pass_desc {
    int64_t size;
    /* masks */
    const uint32_t *rle_counts; const int32_t *rle_off; uint32_t *packed; int32_t *bbox; void *rle_ws; int64_t rle_ws_bytes;
    /* per-pass state */
    int32_t *status; int32_t *hit_count; uint32_t *removed_bits; int64_t removed_words;
    /* sweeps + projection */
    const float *raw; const float *intensity; const int32_t *sweep_row_off; const float *sweep_xf; const int32_t *frame_sweep_off;
    float *points; int32_t *pt_off; const float *cams; const int32_t *mask_off; const int32_t *mask_cam; uint32_t *hit_words;
    void *pg_ws; int64_t pg_ws_bytes;
    /* compaction + medoid */
    int32_t *hit_off; int32_t *tile_off; int32_t *hit_idx; float *hit_xyz; int32_t *tile_work; int32_t *medoid_pos; float *centroid;
    float *colsum; void *ws; int64_t ws_bytes;
    int32_t *md_feedback;        /* cm3d_medoid2's feedback word: page-locked host memory the device writes; read here for the hint */
    /* lanes + boxes */
    float *centroid_g; const int32_t *mask_frame; const float *lane; const int32_t *lane_off; const int32_t *frame_lane;
    const void *grid; int32_t *lane_idx; double *lane_dist; const int32_t *class_id; const double *score; const double *prior_wlh;
    const int32_t *is_vehicle; const int32_t *nms_group; const double *nms_thr; const double *ego_xyz; double *box; int32_t *flags;
    /* what only some batches have */
    const int32_t *mask_wh;      /* NULL: one mask size; else the cm3d_rle_erode_pack_sized launches */
    const float *pose_rt;        /* NULL: nuScenes; else cm3d_centroid_transform (centroid -> centroid_g) in front of the lane search */
    const float *pose_inv;       /* cm3d_box_nms_bounded's (NULL: nuScenes) */
    double *obb_yaw; int32_t *obb_status; void *obb_ws; int64_t obb_ws_bytes;        /* obb_yaw NULL: no cm3d_obb */
    /* set anew for every pass */
    const uint8_t *dense;        /* non-NULL: cm3d_erode_pack of these dense masks instead of the run lengths */
    void *lane_ready;            /* hipEvent_t the stream waits for in front of the lane search (the build of `grid`); NULL: nothing */
    void *ev_project[2];         /* optional hipEvent_t: cm3d_(sweep_)project_hits' ev_start, ev_stop */
    void *ev_stage[5];           /* optional hipEvent_t, recorded in front of the point/mask stages, behind the compaction, the medoid,
                                    the lane search and the boxes */
    /* sizes */
    int32_t n_masks, total_runs, W, H, raw_stride, n_sweeps, max_sweeps_per_frame, max_rows_per_sweep, pt_cap, n_frames,
            max_pts_per_frame, n_cams, planes, idx_cap, n_tables, n_lane_points, n_classes;
    float halfw, min_dist;
    /* set anew for every pass */
    int32_t md_hint;             /* non-zero: ask for the one-pass medoid route when *md_feedback says the last batch held no long list */
    int32_t fused;               /* 0: cm3d_sweep_prep and cm3d_project_hits (needs `points`); else cm3d_sweep_project_hits */
    int32_t separate_reset;      /* non-zero: cm3d_batch_begin as a launch of its own even where the mask launch could carry the reset */
} cm3d_lift_pass_desc;

/* Every pass over a resident batch: enqueues on `stream`, stopping at and returning the first error (a failed event call:
 * CM3D_ERR_LAUNCH); NULL events are skipped.  CM3D_ERR_ARG and no call for another `size`, or for !fused without `points`.  This is the only statement of a pass's order -- cm3d_amd.lifting.LiftEngine.run and
 * cm3d_pipe_submit both end here:
 *
 *   the reset rides on the mask launch when !dense && fused && !separate_reset; else   cm3d_batch_begin
 *   record ev_stage[0]
 *   if (!fused)           cm3d_sweep_prep
 *   masks                 dense ? cm3d_erode_pack : cm3d_rle_erode_pack[_sized][_begin]      (_sized: mask_wh; _begin: carries the reset)
 *   projection            fused ? cm3d_sweep_project_hits : cm3d_project_hits               (ev_project handed through)
 *   cm3d_compact_hits                                                                       (raw rows only when points == NULL)
 *   record ev_stage[1]
 *   cm3d_medoid2                                                                            (flags bit 0 from md_hint and *md_feedback)
 *   record ev_stage[2]
 *   if (lane_ready)       hipStreamWaitEvent
 *   if (pose_rt)          cm3d_centroid_transform
 *   cm3d_lane_nn
 *   record ev_stage[3]
 *   cm3d_box_nms_bounded                                                                    (pose_inv; bound 32 * planes: no frame has more)
 *   record ev_stage[4]
 *   if (obb_yaw)          cm3d_obb */
int cm3d_lift_pass(const cm3d_lift_pass_desc *desc, cm3d_stream_t stream);
/* The two halves of that sequence, each with cm3d_lift_pass's argument checks: cm3d_lift_pass_head is everything through
 * `record ev_stage[1]`, cm3d_lift_pass_tail is cm3d_medoid2 onward.  cm3d_lift_pass is head, then tail. */
int cm3d_lift_pass_head(const cm3d_lift_pass_desc *desc, cm3d_stream_t stream);
int cm3d_lift_pass_tail(const cm3d_lift_pass_desc *desc, cm3d_stream_t stream);

/* min(depth, 4, max(1, hw_queues - 1)): the streams that execute passes at the same time (csrc/pipe_sched.h).  hw_queues <= 0: the
 * value of GPU_MAX_HW_QUEUES in the environment, 4 when it is not set. */
int cm3d_pipe_exec_streams_for(int32_t depth, int32_t hw_queues);

/* A pipeline of `depth` slots over the caller's streams (`streams[depth]`, kept alive by the caller).  exec_streams <= 0: the policy
 * above; else that many (at most depth).  With fewer executing streams than slots, pass number k goes to streams[k % n], and a slot
 * whose previous pass ran on another stream is ordered behind it by the slot's event (not waited for when it has already fired).
 * With n >= depth slot s always runs on streams[s] and no event is ever waited for.  NULL on a bad argument or a runtime error. */
void *cm3d_pipe_create(int32_t depth, int32_t exec_streams, const cm3d_stream_t *streams);
/* The same with a choice of executors (added within ABI v5: new symbols only).  An index the calls below return names an executor:
 * executor i is streams[i], except the null executor, which is the legacy null stream (handle 0) -- its hardware queue carries
 * nothing while passes run, so where the policy above stops at the queues (max(1, hw_queues - 1) < min(depth, 4)) the plan is one
 * executor more, the null stream as the last (csrc/pipe_sched.h, pipe_exec_plan: (4, 4 queues) -> 4 with it, (4, 2) -> 2 with it,
 * (3, 4), (4, 8), (1, any) -> the policy's own, without).  Every stream of `streams` and every other stream whose work must overlap
 * the null stream's has to be non-blocking (hipStreamNonBlocking; torch's are).
 *   null_exec -1: exec_streams <= 0 follows the plan (CM3D_PIPE_NULL_EXEC=0 in the environment: the policy above, no null executor);
 *                 exec_streams > 0 is that many of the caller's streams, no null executor
 *   null_exec  0: never: cm3d_pipe_create
 *   null_exec  1: the last executor is the null stream whenever there are at least two (exec_streams <= 0: the plan's count) */
void *cm3d_pipe_create2(int32_t depth, int32_t exec_streams, const cm3d_stream_t *streams, int32_t null_exec);
/* The executor index that is the null stream, -1: none (also once cm3d_pipe_pin has ended it). */
int cm3d_pipe_null_exec(const void *pipe);
void cm3d_pipe_destroy(void *pipe);
int cm3d_pipe_exec_streams(const void *pipe);
/* Picks the stream of the slot's next pass, orders it behind the slot's previous pass, enqueues cm3d_lift_pass there and records the
 * slot's event.  Returns the stream's index (>= 0) or an error code (< 0). */
int cm3d_pipe_submit(void *pipe, int32_t slot, const cm3d_lift_pass_desc *desc);
/* The same choice and ordering without the pass, for work the caller enqueues itself on streams[returned index]; the caller then
 * calls cm3d_pipe_release, which records the slot's event behind that work. */
int cm3d_pipe_acquire(void *pipe, int32_t slot);
int cm3d_pipe_release(void *pipe, int32_t slot);
/* Blocks the host until the slot's last pass (submit or acquire/release) has completed. */
int cm3d_pipe_wait(void *pipe, int32_t slot);
/* From now on slot s stays on streams[s] (something else, a captured graph, runs there): a null executor ends here, and the slot whose
 * last pass it ran is ordered behind that pass.  Returns CM3D_OK. */
int cm3d_pipe_pin(void *pipe);
/* Index of the stream of the slot's last pass, -1 before the first. */
int cm3d_pipe_last_stream(const void *pipe, int32_t slot);

/* ---- Points in drivable-area polygons, the stage-2 filters and the filtered pass (opt-in) ----
 * Added within ABI v5: three new symbols, no existing call changes, so CM3D_ABI_VERSION stays.
 * Replaces the per-box loop of eval_custom.py:496-526 and the filters the reference ships commented out at 2d_to_3d.py:755-785
 * ("Object lane thresh", "Uncomment for drivable filtering", "Vehicle lane thresh"; src/waymo/2d_to_3d.py:881-934).
 *
 * The test, in float64 and without contraction (host statement: cm3d_amd.eval_detection.point_in_polygons): an edge (xs, ys) ->
 * (xn, yn) of a ring is crossed iff (ys > y) != (yn > y) and x < ((xn - xs) * (y - ys)) / (yn - ys) + xs; a ring's parity is the
 * parity of its crossed edges, counted PER RING; a ring of fewer than 3 nodes is ignored; a point is inside a polygon iff its exterior's
 * parity is odd and no hole's is; the result is the OR over the table's polygons.  The answer is the brute-force answer for every input
 * (points on vertices and edges included: the formula decides them).
 *
 * The polygon index is built on the host (cm3d_amd.drivable.build_index), once per set of tables; T tables back to back:
 *  tab_y     double[T][3]  y-min and y-max over the table's nodes, slabs per unit of y (0 with a single slab)
 *  tab_slab  int32[T][2]   the table's first slab and its number of slabs (0: a table without edges -- every point is outside)
 *  slab_off  int32[slabs+1] entries of slab s at [slab_off[s], slab_off[s+1]).  A point of a table falls into slab
 *                          first + min((int)((y - ymin) * per_y), n - 1); a point outside [y-min, y-max] is outside
 *  ent_edge  int32[entries] the slab's edges: every edge whose closed y-interval touches the slab (and, conservatively, the slabs next
 *                          to those), sorted by edge number, so that the edges of a ring are neighbours and the rings of a polygon too
 *  ent_ring  int32[entries] the ring of each entry's edge
 *  edge      double[E][4]  xs, ys, xn, yn
 *  ring_info int32[R]      2 * polygon number + (1 for a hole); rings in polygon order, a polygon's exterior first
 * Every count is below 2^31 (the host raises otherwise).  The kernels allocate nothing and write only inside[p] / medoid_pos_kept[m] /
 * on_road[m]; a table number outside [0, n_tables) reads as "outside".  One wave per point.
 *
 *  xy double[n_points][2]; point_table int32[n_points] the table of each point; inside uint8[n_points] OUT 0 / 1 */
int cm3d_points_in_polygons(const double *xy, const int32_t *point_table, int32_t n_points, const double *tab_y,
                            const int32_t *tab_slab, const int32_t *slab_off, const int32_t *ent_edge, const int32_t *ent_ring,
                            const double *edge, const int32_t *ring_info, int32_t n_tables, uint8_t *inside, cm3d_stream_t stream);

/* The stage-2 filters on what a pass left in device memory.  Mask m's point is its medoid in the global frame,
 * ((double)centroid_g[3m], (double)centroid_g[3m+1]) -- the reference's float(m_x), float(m_y), not the pushed centre --, its table
 * frame_lane[mask_frame[m]]: the location index of the lane tables.  tab_y == NULL: no polygons, no road test (the other index
 * arrays and needs_road are then ignored).
 *   medoid_pos_kept[m] = medoid_pos[m], unless the mask has a centroid (medoid_pos[m] >= 0) and is dropped; then -1.  Dropped iff
 *     lane_dist[m] > lane_max_dist                                              (any class, :755), or
 *     is_vehicle[cls] && lane_dist[m] > vehicle_lane_max_dist                   (:782), or
 *     polygons given && needs_road[cls] && the point is not inside               (:775; car, truck and bus)
 *   strict > on float64, so a threshold of +inf is off.
 *   on_road[m] = 1 iff polygons are given, the mask has a centroid and its point is inside (every class); else 0. */
int cm3d_stage2_filter(const float *centroid_g, const int32_t *medoid_pos, const int32_t *mask_frame, const int32_t *frame_lane,
                       const int32_t *class_id, const double *lane_dist, int32_t n_masks, int32_t n_frames, const double *tab_y,
                       const int32_t *tab_slab, const int32_t *slab_off, const int32_t *ent_edge, const int32_t *ent_ring,
                       const double *edge, const int32_t *ring_info, int32_t n_tables, const int32_t *needs_road,
                       const int32_t *is_vehicle, int32_t n_classes, double lane_max_dist, double vehicle_lane_max_dist,
                       int32_t *medoid_pos_kept, uint8_t *on_road, cm3d_stream_t stream);

/* What the filtered pass needs beyond cm3d_lift_pass_desc.  `size` is sizeof(cm3d_stage2_filter_desc) (another value: CM3D_ERR_ARG).
 * The index arrays and needs_road as in cm3d_stage2_filter (tab_y NULL: no road test); n_poly_tables = the batch's n_tables. */
typedef struct cm3d_stage2_filter_desc {
    int64_t size;
    const double *tab_y; const int32_t *tab_slab; const int32_t *slab_off; const int32_t *ent_edge; const int32_t *ent_ring;
    const double *edge; const int32_t *ring_info; const int32_t *needs_road;
    int32_t *medoid_pos_kept; uint8_t *on_road;
    void *ev[2];                 /* optional hipEvent_t, recorded in front of and behind the filter launch */
    double lane_max_dist, vehicle_lane_max_dist;
    int32_t n_poly_tables, reserved;
} cm3d_stage2_filter_desc;

/* The opt-in filtered pass: cm3d_lift_pass_opt (below) with only `filter` set; a NULL `filter` is CM3D_ERR_ARG.  k_box_nms treats a
 * negative position as "no box", so a dropped mask neither gets a box nor suppresses one. */
int cm3d_lift_pass_filtered(const cm3d_lift_pass_desc *desc, const cm3d_stage2_filter_desc *filter, cm3d_stream_t stream);

/* ---- Depth clustering of every mask's in-mask list, and the clustered pass (opt-in) ----
 * Added within ABI v5: new symbols only, no existing call changes, so CM3D_ABI_VERSION stays.
 * Stands where the reference's clusters_hdbscan stood (src/kitti/2d_to_3d.py:159-174, src/waymo/2d_to_3d.py:102-117; its only call
 * site is commented out): background points inside a mask -- seen through windows, leaked in at the mask's edge -- are dropped before
 * the medoid and the box fit see the list.  It is a 1-D gap clustering on the range from the sensor rig, exact and independent of the
 * order of processing; host statement: cm3d_amd.cluster.depth_cluster_host.
 *
 * Per mask m: its list is positions hit_off[m] .. hit_off[m+1] of hit_xyz (and hit_idx), its origin o = origin[mask_frame[m]].
 *   key      float64, no contraction: dx = (double)x - ox, dy, dz alike; r = sqrt((dx*dx + dy*dy) + dz*dz)
 *   clusters the positions sorted by (r, position); a boundary lies between sorted neighbours iff r[k+1] - r[k] > eps (strict,
 *            float64) -- the connected components of |ri - rj| <= eps
 *   choice   a cluster qualifies iff it has >= min_points points.  pick 0 (largest): the qualifying cluster of most points, the
 *            nearer one (smaller first range) on a tie; pick 1 (nearest): the first qualifying cluster in range order
 *   result   cl_status[m] = 0: the chosen cluster's points, in the list's own (ascending) order; 1: no cluster qualifies, the list is
 *            kept whole (the reference's `return None`, :168-171); 2: empty list, empty result.  A non-empty list never becomes empty.
 *  hit_xyz    float[idx_cap][4]; hit_idx int32[idx_cap] or NULL; hit_off int32[n_masks+1]; mask_frame int32[n_masks]
 *  origin     double[n_frames][3] (a frame number outside [0, n_frames) reads as the origin 0, 0, 0)
 *  eps > 0 (+inf: one cluster), min_points >= 1, pick 0 or 1: anything else, NaN included, is CM3D_ERR_ARG and no launch
 *  cl_off      int32[n_masks+1] OUT exclusive scan of the kept counts
 *  cl_tile_off int32[n_masks+1] OUT exclusive scan of ceil(kept count / CM3D_MEDOID_TILE)
 *  cl_idx      int32[idx_cap] OUT (NULL exactly when hit_idx is), cl_xyz float[idx_cap][4] OUT: the kept entries, laid out by cl_off
 *  cl_status   int32[n_masks] OUT
 *  workspace: cm3d_depth_cluster_workspace_bytes(n_masks, idx_cap) = 13 idx_cap + 4 n_masks bytes, 8-byte aligned (sort keys and
 *             positions of the lists too long for LDS, placed by the offsets; one keep byte per position; the kept counts)
 * Three launches, no synchronisation, no allocation: one workgroup per mask sorts (in LDS up to CM3D_DEPTH_CLUSTER_LDS_POINTS points,
 * in the workspace beyond: every length gives the statement's answer), finds the clusters and marks the kept positions; one
 * workgroup scans the counts; one workgroup per mask compacts.  An offset outside [0, idx_cap] is clamped into it and a list end below
 * its start is an empty list: no position >= idx_cap is read or written whatever hit_off holds. */
int64_t cm3d_depth_cluster_workspace_bytes(int32_t n_masks, int32_t idx_cap);
int cm3d_depth_cluster(const float *hit_xyz, const int32_t *hit_idx, const int32_t *hit_off, const int32_t *mask_frame, int32_t n_masks,
                       int32_t idx_cap, const double *origin, int32_t n_frames, double eps, int32_t min_points, int32_t pick,
                       int32_t *cl_off, int32_t *cl_tile_off, int32_t *cl_idx, float *cl_xyz, int32_t *cl_status, void *workspace,
                       int64_t workspace_bytes, cm3d_stream_t stream);

/* What the clustered pass needs beyond cm3d_lift_pass_desc.  `size` is sizeof(cm3d_depth_cluster_desc) (another value: CM3D_ERR_ARG);
 * the other fields as in cm3d_depth_cluster (origin: double[desc->n_frames][3]). */
typedef struct cm3d_depth_cluster_desc {
    int64_t size;
    const double *origin;
    int32_t *cl_off; int32_t *cl_tile_off; int32_t *cl_idx; float *cl_xyz; int32_t *cl_status;
    void *ws; int64_t ws_bytes;
    void *ev[2];                 /* optional hipEvent_t, recorded in front of and behind the clustering's launches */
    double eps;
    int32_t min_points, pick;
} cm3d_depth_cluster_desc;

/* The opt-in clustered pass: cm3d_lift_pass_opt (below) with only `cluster` set; a NULL `cluster` is CM3D_ERR_ARG.  The medoid, colsum
 * and cm3d_obb see the clustered lists and medoid_pos is a position in them; the raw lists stay what they were. */
int cm3d_lift_pass_clustered(const cm3d_lift_pass_desc *desc, const cm3d_depth_cluster_desc *cluster, cm3d_stream_t stream);

/* ---- Vehicle yaw from the in-mask points: L-shape fit, and the yaw-fitted pass (opt-in) ----
 * Added within ABI v5: new symbols only, no existing call changes, so CM3D_ABI_VERSION stays.
 * On nuScenes and Waymo the reference takes a box's heading from the nearest lane point (2d_to_3d.py:295) and never from the points.
 * cm3d_bev_fit fits a heading AXIS to every list: search-based L-shape fitting with the closeness criterion (Zhang et al., IV 2017) on
 * the list's bird's-eye view, in whatever frame the list is in; host statement: cm3d_amd.bevfit.bev_fit_host.  What it does to label
 * quality has not been measured, and the defaults of its parameters (cm3d_amd.bevfit.YawFit) have not been tuned.
 *
 * Per mask m: its list is positions hit_off[m] .. hit_off[m+1] of hit_xyz, n points (xi, yi) of float32; z is not used.  All
 * arithmetic is float64, every product and sum rounded on its own (no contraction):
 *   x = (double)xi - (double)x0, y = (double)yi - (double)y0, (x0, y0) the list's first point
 *   per angle k, (c, s) = angle_cs[k]:  c1 = (x*c) + (y*s), c2 = (y*c) - (x*s); lo1, hi1, lo2, hi2 their minima and maxima over the list;
 *     d = max(min(min(hi1 - c1, c1 - lo1), min(hi2 - c2, c2 - lo2)), d0); q_k = (((+0.0 + 1.0/d_0) + 1.0/d_1) + ...) in LIST ORDER
 *   k* = the k of the greatest q_k, the smallest on a tie; at k*: a = hi1 - lo1, b = hi2 - lo2; length = max(a, b), width = min(a, b);
 *     the heading axis is the longer side, (c, s) when a >= b, else (-s, c);
 *     m1 = (lo1 + hi1) * 0.5, m2 = (lo2 + hi2) * 0.5;  cx = ((m1*c) - (m2*s)) + (double)x0,  cy = ((m1*s) + (m2*c)) + (double)y0
 *   fit_status[m]: tested in this order -- 2 empty list; 1 fewer than min_points points; 4 a non-finite x or y in the list (tested
 *     before any minimum or maximum is taken); 3 length < min_length; else 0 fitted.  For a status other than 0 the record is six
 *     zeros and fit_k[m] = -1.
 *  hit_xyz   float[idx_cap][4], 16-byte aligned; hit_off int32[n_masks+1].  An offset outside [0, idx_cap] is clamped into it and a
 *            list end below its start is an empty list: no position >= idx_cap is read whatever hit_off holds.  Every list length up
 *            to idx_cap gives the statement's answer: a list is staged through LDS CM3D_BEV_FIT_CHUNK points at a time.
 *  angle_cs  double[K][2], 16-byte aligned: cos, sin of k * pi / (2K), computed by the caller (cm3d_amd.bevfit.angle_table) so that
 *            device and host use the same bits; the kernel does no trigonometry.  K: 64, 128, 192 or 256
 *  d0 > 0, min_points >= 2, min_length >= 0, all finite: anything else is CM3D_ERR_ARG and no launch
 *  fit_k     int32[n_masks] OUT;  fit_status int32[n_masks] OUT
 *  fit_rect  double[n_masks][CM3D_MATCH_BOX_STRIDE] OUT: cx, cy, length, width, cos, sin -- the record of cm3d_bev_match; the heading
 *            is an axis, not yet resolved modulo pi
 * One launch, one workgroup of K threads per mask: lanes are angles, a lane walks the list twice (the rule's order of summation is
 * the lane's own loop).  No atomics, no allocation, no workspace: every run gives the same bytes. */
#define CM3D_BEV_FIT_CHUNK 512   /* points of a list cm3d_bev_fit stages in LDS at a time (16 bytes each) */
int cm3d_bev_fit(const float *hit_xyz, const int32_t *hit_off, int32_t n_masks, int32_t idx_cap, const double *angle_cs, int32_t K,
                 double d0, int32_t min_points, double min_length, int32_t *fit_k, double *fit_rect, int32_t *fit_status,
                 cm3d_stream_t stream);

/* The yaw each mask's box is built with, one thread per mask; host statement: cm3d_amd.bevfit.yaw_select_host.
 * A mask takes the fit iff medoid_pos[m] >= 0 && fit_status[m] == 0 && is_vehicle[class] && lane_dist[m] >= lane_min_dist
 * (lane_min_dist 0: always; a positive value trusts the lanes on the road and the fit away from it).  Then, with (c, s) the record's
 * axis:  pose_rt != NULL (Waymo: the lists are in the vehicle frame) rotates it by the float32 pose's upper-left 2x2 widened to
 * float64, cg = (R00*c) + (R01*s), sg = (R10*c) + (R11*s), else cg = c, sg = s;  yl = (double) the lane point's float32 yaw,
 * dot = (cg*cos(yl)) + (sg*sin(yl));  dot < 0: both negated -- the fit gives the axis, the map which way along it;
 * yaw = (float)atan2(sg, cg).  Every other mask with a medoid gets its lane point's yaw bit for bit -- the point cm3d_box_nms reads,
 * lane[lane_off[frame_lane[mask_frame[m]]] + lane_idx[m]] -- and a mask without a medoid gets 0.  Indices are clamped into their
 * arrays (n_frames, n_tables, n_lane_points).
 *  pose_rt  float[F][12] as in cm3d_centroid_transform, or NULL;  lane_min_dist >= 0 (NaN: CM3D_ERR_ARG)
 *  yaw_tab  float[n_masks][3] OUT: 0, 0, yaw -- a lane table of n_masks rows;  yaw_idx int32[n_masks] OUT: yaw_idx[m] = m
 *  yaw_src  int32[n_masks] OUT: 0 lane, 1 fit */
int cm3d_yaw_select(const double *fit_rect, const int32_t *fit_status, const int32_t *medoid_pos, const int32_t *mask_frame,
                    const int32_t *class_id, const int32_t *is_vehicle, int32_t n_classes, const double *lane_dist,
                    double lane_min_dist, const float *lane, const int32_t *lane_off, const int32_t *frame_lane,
                    const int32_t *lane_idx, int32_t n_tables, int32_t n_lane_points, const float *pose_rt, int32_t n_masks,
                    int32_t n_frames, float *yaw_tab, int32_t *yaw_idx, int32_t *yaw_src, cm3d_stream_t stream);

/* What the yaw-fitted pass needs beyond cm3d_lift_pass_desc.  `size` is sizeof(cm3d_yaw_fit_desc) (another value: CM3D_ERR_ARG).
 *  hit_xyz, hit_off  the lists cm3d_yaw_fit_boxes fits; NULL: the pass descriptor's
 *  medoid_pos        the positions that decide for cm3d_yaw_fit_boxes which masks have a box; NULL: the pass descriptor's
 *                    (cm3d_lift_pass_opt derives all three itself: there each is NULL or what it derives)
 *  tab_off   int32[2] = {0, n_masks};  tab_frame int32[n_frames] = zeros: filled by the caller once, they make yaw_tab the lane table
 *            of every frame
 *  the other fields as in cm3d_bev_fit and cm3d_yaw_select */
typedef struct cm3d_yaw_fit_desc {
    int64_t size;
    const double *angle_cs;
    const float *hit_xyz; const int32_t *hit_off; const int32_t *medoid_pos;
    int32_t *fit_k; double *fit_rect; int32_t *fit_status;
    float *yaw_tab; int32_t *yaw_idx; int32_t *yaw_src;
    const int32_t *tab_off; const int32_t *tab_frame;
    void *ev[2];                 /* optional hipEvent_t, recorded in front of cm3d_bev_fit and behind cm3d_yaw_select */
    double d0, min_length, lane_min_dist;
    int32_t K, min_points;
} cm3d_yaw_fit_desc;

/* The three launches behind a pass that has run (host code, csrc/pass_options.cpp).  Enqueues on `stream`, stopping at and returning
 * the first error; a wrong `size` or a null table or output: CM3D_ERR_ARG and no call:
 *
 *   record fit->ev[0]
 *   cm3d_bev_fit                          the lists -> fit_k, fit_rect, fit_status
 *   cm3d_yaw_select                       lane_idx, lane_dist, lane tables ... of desc -> yaw_tab, yaw_idx, yaw_src
 *   record fit->ev[1]
 *   cm3d_box_nms_bounded                  as in the plain pass, with lane = yaw_tab, lane_off = tab_off, frame_lane = tab_frame,
 *                                         lane_idx = yaw_idx (and fit->medoid_pos when given): `box` and `flags` written anew
 *
 * k_box_nms reads nothing of a lane point but its yaw, so it is untouched.  Column 5 of the box record ("lane yaw") then holds the yaw
 * that was USED: the fitted one where yaw_src[m] == 1.  A mask with yaw_src[m] == 0 gets the record the plain pass gave it. */
int cm3d_yaw_fit_boxes(const cm3d_lift_pass_desc *desc, const cm3d_yaw_fit_desc *fit, cm3d_stream_t stream);
/* The opt-in yaw-fitted pass: cm3d_lift_pass_opt (below) with only `yaw` set; a NULL `fit` is CM3D_ERR_ARG. */
int cm3d_lift_pass_yaw_fitted(const cm3d_lift_pass_desc *desc, const cm3d_yaw_fit_desc *fit, cm3d_stream_t stream);

/* ---- One pass with any of the opt-in stages, in one call ----
 * Added within ABI v5: new symbols only, so CM3D_ABI_VERSION stays.  Host code (csrc/pass_options.cpp): no kernel of its own;
 * cm3d_lift_pass and cm3d_pipe_submit know nothing of it. */
typedef struct cm3d_rotated_nms_desc {     /* what cm3d_box_rotated_nms takes beyond the pass descriptor */
    int64_t size;
    const double *thr; int32_t n_thr, measure, class_agnostic, reserved;
} cm3d_rotated_nms_desc;

typedef struct cm3d_lift_pass_options {    /* NULL member: that stage is off */
    int64_t size;
    const cm3d_depth_cluster_desc *cluster;
    const cm3d_stage2_filter_desc *filter;
    const cm3d_yaw_fit_desc       *yaw;
    const cm3d_rotated_nms_desc   *nms;
} cm3d_lift_pass_options;

/* Every pass with an opt-in stage: enqueues on `stream`, stopping at and returning the first error (a failed event call:
 * CM3D_ERR_LAUNCH); NULL events are skipped; no descriptor of the caller's is written.  This is the only statement of a composed
 * pass's order for the stages the options name -- cm3d_lift_pass_composed (at the end of this header; it adds the stages the options
 * have no member for) and the three single-option passes end here:
 *
 *   every present descriptor is checked first: `size` of opt, desc and each member; cluster's cl_off, cl_tile_off, cl_xyz, cl_status
 *   (and cl_idx when desc has hit_idx); filter's medoid_pos_kept, on_road; yaw's tables and outputs as in cm3d_yaw_fit_boxes, and its
 *   hit_xyz, hit_off, medoid_pos each NULL or what `yaw` below derives; nms's thr.  CM3D_ERR_ARG and NO call at all, whichever is bad
 *   cluster ?  cm3d_lift_pass_head(desc); record cluster->ev[0]; cm3d_depth_cluster (desc's lists -> the cl_* arrays); record cluster->ev[1]
 *              cm3d_lift_pass_tail(desc')            desc' = desc with hit_off, tile_off, hit_idx, hit_xyz = the cl_* arrays, tile_work = NULL
 *           :  cm3d_lift_pass(desc)                  the plain pass, boxes of every mask included
 *   filter  ?  record filter->ev[0]; cm3d_stage2_filter (centroid_g, medoid_pos, lane_dist ... of desc -> medoid_pos_kept, on_road);
 *              record filter->ev[1]
 *              cm3d_box_nms_bounded                  as in the plain pass, with medoid_pos_kept for medoid_pos: `box`, `flags` written anew
 *   yaw     ?  cm3d_yaw_fit_boxes' sequence          lists = cluster ? cl_xyz, cl_off : desc's;  positions = filter ? medoid_pos_kept : desc's
 *   nms     ?  cm3d_box_rotated_nms                  box, flags, mask_off ... of desc; waymo = pose_inv != NULL; bound as the box launch's
 *   opt == NULL or every member NULL: exactly cm3d_lift_pass(desc)
 *   behind the pass, a call of the caller's own and no member of opt: cm3d_box_velocity (below) on desc's box, flags, mask_off, class_id
 *   behind cm3d_box_velocity, a call of the caller's own as well: cm3d_box_tracks (below) on desc's box, flags and the two match arrays */
int cm3d_lift_pass_opt(const cm3d_lift_pass_desc *desc, const cm3d_lift_pass_options *opt, cm3d_stream_t stream);

/* ---- box velocity from frame-to-frame association (opt-in; nuScenes: boxes in the global frame) --------------------
 * The reference writes "velocity": [0, 0] into every box (src/nuscenes/2d_to_3d.py:808-817).  This stage fills the field: the kept
 * boxes of consecutive keyframes of a scene are associated one to one by the maximum-weight assignment of csrc/assign.h, and a box's
 * velocity is the difference of matched centres over the difference of their frames' times.  It is a call of its own BEHIND the
 * pass -- cm3d_lift_pass_opt(desc, opt, stream); cm3d_box_velocity(desc's box, flags, mask_off, class_id ..., stream) -- and so
 * behind the rotated NMS when that is on: its input is the final kept set.  cm3d_lift_pass_options has no member for it.  Host
 * statement to the bit: cm3d_amd.velocity.track_velocity_host.
 *
 *  box, flags  double[n_masks][CM3D_BOX_STRIDE], int32[n_masks] as the last box launch or the rotated NMS left them; a box is KEPT iff
 *              (flags & 3) == 3; its centre is box[0], box[1]
 *  mask_off    int32[F+1]; a frame's start is clamped to [0, n_masks] and its end to [start, n_masks] before use; a frame of more than
 *              CM3D_MAX_MASKS_PER_FRAME masks takes part in no link (status bit 1)
 *  class_id    int32[n_masks]; track_group int32[n_classes] (the entry points pass nms_group); max_speed double[n_groups], m/s.  A
 *              class outside [0, n_classes) or a group outside [0, n_groups) never matches
 *  frame_next  int32[F]: batch index of the same scene's following keyframe, or -1.  A value outside [-1, F) sets status bit 0 and
 *              is read as -1.  No two frames may name the same follower
 *  frame_time  double[F] seconds, formed on the host from the int64 microsecond timestamps minus the batch's smallest, times 1e-6
 *  max_dt      seconds, > 0 (the max_time_diff of the devkit's box_velocity; 1.5 at the entry points); NaN or <= 0: CM3D_ERR_ARG
 *
 *  Links.   f -> n = frame_next[f] is a link iff n >= 0 and 0 < dt = frame_time[n] - frame_time[f] <= max_dt.
 *  Weights. Rows are ALL masks of f, columns all masks of n, in mask order.  A pair has weight 0 unless both boxes are kept and
 *           track_group of their classes is equal (= g).  Then, every operation rounded on its own, no fma:
 *             dx = bn[0] - bf[0];  dy = bn[1] - bf[1];  d2 = (dx * dx) + (dy * dy);  gate = max_speed[g] * dt
 *             gate > 0 and d2 <= gate * gate ?  r = sqrt(d2) / gate;  weight = r <= 1 ? 1 + (int)((1.0 - r) * (double)(ASSIGN_KMAX - 1)) : 0
 *                                            :  weight = 0                  (ASSIGN_KMAX = 1000000; NaN compares false: weight 0)
 *           float64 sqrt and / are correctly rounded on the host and on the device: the integers are the same bits.
 *  Assign.  Maximum total weight, one to one, by AssignSolver's steps and tie rule (an unassigned column first, then the lowest
 *           column), rows = the smaller side as in cm3d_bev_match.  An assigned pair is a match iff its weight is positive.
 *  Velocity of mask i of frame f at time t, float64: p+, t+ the centre and frame time of next_match[i], p-, t- of prev_match[i]; the
 *           first of   central (p+ - p-) / (t+ - t-),  forward (p+ - p) / (t+ - t),  backward (p - p-) / (t - t-)
 *           whose matches exist and whose time span is <= max_dt; else (0.0, 0.0).  vel_src: 0 none, 1 forward, 2 backward, 3 central.
 *           A mask that is not kept has no match and gets zeros and 0.
 *
 *  pair_off    int64[n_links+1], n_links == n_frames: link slot f holds the pairs of f -> frame_next[f],
 *              pair_off[f+1] - pair_off[f] = M_f * M_n for a link and 0 otherwise, total_pairs = pair_off[n_links]: computed by the
 *              host from mask_off, frame_next and frame_time alone (no read-back).  A slot that disagrees with what the device derives
 *              from those arrays, or leaves [0, total_pairs], is skipped (status bit 1)
 *  next_match, prev_match  int32[n_masks] OUT: batch mask index of the match in the following / preceding frame, or -1
 *  vel double[n_masks][2], vel_src int32[n_masks] OUT.  The first launch initialises all four outputs: a rerun gives the same bytes
 *  status      int32[1], zero it before the call; bits are only ever set
 *  workspace   cm3d_box_velocity_workspace_bytes(total_pairs, n_masks): the int32 weights, the first link of every 256-pair block and
 *              every mask's frame
 *  Launches: k_track_init (outputs, every mask's frame), k_assign_block_owner, k_track_weight (one thread per pair),
 *  k_track_assign<1, 2, 4, 16> (one wave per link; weights in LDS up to 8192 pairs, from L2 above), k_track_velocity (one thread per
 *  mask).  Plain stores; the only atomic is the status word's. */
int64_t cm3d_box_velocity_workspace_bytes(int64_t total_pairs, int32_t n_masks);
int cm3d_box_velocity(const double *box, const int32_t *flags, const int32_t *mask_off, int32_t n_frames, int32_t n_masks,
                      const int32_t *class_id, const int32_t *track_group, const double *max_speed, int32_t n_classes,
                      int32_t n_groups, const int32_t *frame_next, const double *frame_time, double max_dt, const int64_t *pair_off,
                      int32_t n_links, int64_t total_pairs, int32_t *next_match, int32_t *prev_match, double *vel, int32_t *vel_src,
                      int32_t *status, void *workspace, int64_t workspace_bytes, cm3d_stream_t stream);

/* ---- box tracks from the velocity stage's matches (opt-in; a call of its own BEHIND cm3d_box_velocity) ---------------
 * Added within ABI v5: new symbols only.  cm3d_box_velocity leaves next_match / prev_match; this stage follows them: a track id,
 * position and length per kept box, four statistics per track, a least-squares velocity over a window of the track, a track score
 * and a length filter.  What it does to label quality has not been measured, and none of its defaults is tuned.  Host statement to
 * the bit: cm3d_amd.tracks.box_tracks_host.  M = n_masks, F = n_frames.
 *
 *  box, flags  double[M][CM3D_BOX_STRIDE], int32[M], IN/OUT: only box[i][7], box[i][9] and bit 1 of flags[i] are ever written
 *  mask_frame  int32[M] the batch frame of every mask;  frame_time double[F] seconds (as cm3d_box_velocity takes them)
 *  next_match, prev_match  int32[M] as cm3d_box_velocity left them; read only
 *
 *  Kept.    kept(i) = (flags[i] & 3) == 3 and 0 <= mask_frame[i] < F.  Flag bits set but a frame outside [0, F): status bit 0, not kept.
 *  Links.   For a kept i and j = next_match[i]:  j outside [-1, M): status bit 1, read as -1.  j >= 0 is a valid next link iff kept(j),
 *           prev_match[j] == i and frame_time[mask_frame[j]] > frame_time[mask_frame[i]] (NaN compares false); else status bit 2, read
 *           as -1.  prev_match symmetrically: p valid iff kept(p), next_match[p] == i and p's time < i's.  Valid links are mutual and
 *           strictly forward in time: whatever the arrays hold, the structure is a set of disjoint paths of at most F masks each,
 *           without cycles, and no index outside [0, M) or [0, F) addresses memory.  What cm3d_box_velocity writes sets none of the bits.
 *  Tracks.  A head is a kept mask without a valid previous link; its track m_0 = head, m_1 = next(m_0), ..., m_{L-1}.  Every member:
 *           track_id = m_0 (the head's batch mask index), track_pos = k, track_len = L, and track_stat[4], float64, every operation
 *           rounded on its own (no fma), s_k = box[m_k][7] as on entry, t_k = m_k's frame time:
 *             [0] (((+0.0 + s_0) + s_1) + ...) in track order        [1] the greatest s_k: s_0, replaced by every later s_k > it
 *             [2] t_{L-1} - t_0                                      [3] sqrt((dx * dx) + (dy * dy)) of the last centre minus the first
 *           A mask that is not kept: track_id -1, track_pos -1, track_len 0, zeros in track_stat and vel_smooth.
 *  Smoothed velocity, smooth_window = W >= 1 (0: off; vel_smooth may then be NULL, and holds zeros if it is given).  Member i at position p: the window
 *           is the n members at positions max(0, p - W) .. min(L - 1, p + W) in track order.  n < 2: zeros.  Else per window member j
 *             t = time(j) - time(i);  x = box[j][0] - box[i][0];  y = box[j][1] - box[i][1]
 *           six left-to-right sums from +0.0: St, Stt (of t * t), Sx, Sy, Stx (of t * x), Sty (of t * y); then
 *             den = ((double)n * Stt) - (St * St);  den > 0 ?  vx = (((double)n * Stx) - (St * Sx)) / den,  vy alike  :  zeros
 *           -- the least-squares slope through the window.  vel, vel_src and the match arrays of cm3d_box_velocity are never written.
 *  Score, score_mode: 0 own, nothing written; 1 mean, box[i][7] = track_stat[0] / (double)L; 2 max, box[i][7] = track_stat[1].  Kept
 *           masks only, from the scores as they were on entry.
 *  Filter, min_length >= 1: a kept mask with L < min_length loses bit 1 of flags[i], and box[i][9] = (double)flags[i] as
 *           cm3d_box_rotated_nms writes it; nothing else of the mask changes.  A whole track goes or stays.
 *
 *  CM3D_ERR_ARG before any launch: n_masks < 0, n_frames <= 0, min_length < 1, score_mode outside 0..2, smooth_window < 0,
 *  smooth_window > 0 with vel_smooth NULL, a NULL array that M > 0 needs.  CM3D_ERR_WORKSPACE before any launch: workspace NULL or
 *  shorter than cm3d_box_tracks_workspace_bytes(n_masks) (a double and two int32 per mask: time, validated next and previous link).
 *  The first launch initialises track_id, track_pos, track_len, track_stat and vel_smooth: a rerun on restored inputs gives the same
 *  bytes.  box and flags are IN/OUT: with min_length > 1 or score_mode != 0 a second call on the same arrays sees other scores and
 *  another kept set, so it is no rerun -- the pass writes both anew before every call of the engine's.
 *  status      int32[1], zero it before the call; bits 0..2 above are only ever set
 *  Launches: k_tracks_links, k_tracks_walk, k_tracks_apply, one thread per mask each.  The third, which changes flags, reads validity
 *  from the workspace alone.  Plain stores; the only atomic is the status word's OR; no allocation. */
int64_t cm3d_box_tracks_workspace_bytes(int32_t n_masks);
int cm3d_box_tracks(double *box, int32_t *flags, const int32_t *mask_frame, const int32_t *next_match, const int32_t *prev_match,
                    const double *frame_time, int32_t n_masks, int32_t n_frames, int32_t min_length, int32_t score_mode,
                    int32_t smooth_window, int32_t *track_id, int32_t *track_pos, int32_t *track_len, double *track_stat,
                    double *vel_smooth, int32_t *status, void *workspace, int64_t workspace_bytes, cm3d_stream_t stream);

/* ---- box centre from the fitted rectangle instead of the view-ray push (opt-in; behind the yaw fit) -------------------
 * Added within ABI v5: new symbols only, so CM3D_ABI_VERSION stays.  The box launch puts a vehicle's centre at the medoid pushed
 * along the view ray by min(|w / 2 sin|, |l / 2 cos|) (push_centroid, src/nuscenes/2d_to_3d.py:164-198): a guess that never looks
 * at where the faces are.  cm3d_bev_fit leaves the bounding rectangle of a mask's points at the fitted angle; its sensor-side corner
 * is a corner of the object and its sensor-side edges are faces.  This stage hangs the class's length and width on them.  What it
 * does to label quality has not been measured, and `thin` is not tuned.  Host statement to the bit, NMS included:
 * cm3d_amd.boxplace.box_place_host.  All float64, every product, sum and difference rounded on its own, no fma, no library call.
 *
 *  Placed.  Mask m of frame f is placed iff flags[m] & 1, yaw_src[m] == 1, and the sensor and the six record values are finite.
 *           cx, cy, a, b, hc, hs = fit_rect[m];  c = box[m][8] >= 0 && box[m][8] < n_classes ? (int)box[m][8] : 0 (as
 *           cm3d_box_rotated_nms reads it);  len = prior_wlh[3 c + 1], wid = prior_wlh[3 c + 0] (length along the heading);
 *           sensor (sx, sy) = ego_xyz[3 f], ego_xyz[3 f + 1] (nuScenes: lists, rectangles and boxes are global), or (0, 0) when
 *           waymo != 0 (all three in the vehicle frame; ego_xyz is not read and may be NULL).
 *             ex = sx - cx;  ey = sy - cy;  pu = (ex*hc) + (ey*hs);  pv = (ey*hc) - (ex*hs)
 *             su = pu >= 0 ? 1.0 : -1.0;  sv = pv >= 0 ? 1.0 : -1.0
 *             au = b >= thin   (two faces seen: the corner fixes the box along the heading);   av = a >= thin
 *             du = au ? su * ((a - len) * 0.5) : 0.0   (not anchored: centred on the face);    dv = av ? sv * ((b - wid) * 0.5) : 0.0
 *             x = ((du*hc) - (dv*hs)) + cx;  y = ((du*hs) + (dv*hc)) + cy
 *           The rule is the same under (hc, hs) -> (-hc, -hs): the axis sign cm3d_yaw_select resolved is not needed.
 *           box[m][0] = x, box[m][1] = y; columns 2..8 are untouched (z stays the medoid's).  place_src[m]: 1 both axes anchored,
 *           2 one, 3 none.  A mask that is not placed keeps columns 0..8 bit for bit and gets place_src 0.
 *  place_pushed double[n_masks][2] OUT: box[m][0], box[m][1] as they were on entry, for every mask
 *  place_src    int32[n_masks] OUT, written whole
 *  thin         finite, >= 0 (0: both axes always anchored); NaN, negative or infinite: CM3D_ERR_ARG
 *  NMS.     The circle NMS of the box launch ran on the pushed centres; it is decided again here, in the same launch, on the
 *           centres as they now are: descending score, ties by descending index, group nms_group[c], dist^2 <= nms_thr[group],
 *           only masks with flags & 1 (cm3d_box_nms's rule and code).  Bit 1 of flags and column 9 of box are rewritten for
 *           EVERY mask of the batch; bit 0 stays.  max_masks_per_frame as in cm3d_box_nms_bounded: the launch's LDS is sized by
 *           it (none up to 64), and the masks of a frame beyond it are not placed and not kept.
 *  mask_off int32[F+1]; a frame's start is clamped to [0, n_masks] and its end to [start, n_masks] before use
 * CM3D_ERR_ARG and no launch: a NULL array (ego_xyz only when waymo == 0), a non-positive n_frames, n_masks, n_classes or
 * max_masks_per_frame, a bad thin.  One launch, k_box_place<WAYMO>, one wave per frame; plain stores, no atomics, no workspace. */
int cm3d_box_place(double *box, int32_t *flags, const int32_t *mask_off, int32_t n_frames, int32_t n_masks, const double *fit_rect,
                   const int32_t *yaw_src, const double *prior_wlh, const int32_t *nms_group, const double *nms_thr, int32_t n_classes,
                   const double *ego_xyz, int32_t waymo, double thin, int32_t max_masks_per_frame, int32_t *place_src,
                   double *place_pushed, cm3d_stream_t stream);

typedef struct cm3d_box_place_desc {       /* what the placed pass needs beyond the pass descriptor and the options */
    int64_t size;                          /* sizeof(cm3d_box_place_desc); another value: CM3D_ERR_ARG */
    int32_t *place_src; double *place_pushed;
    void *ev[2];                           /* optional hipEvent_t, recorded in front of and behind cm3d_box_place */
    double thin;
} cm3d_box_place_desc;

/* The composed pass with the placement: cm3d_lift_pass_composed(desc, opt, place, NULL, NULL, stream) (below; host code,
 * csrc/pass_compose.cpp), which states the order and the checks; cm3d_lift_pass_options has no member for the placement and
 * csrc/pass_options.cpp does not know it.  Its own requirement, checked first: a NULL opt or a NULL place is CM3D_ERR_ARG and NO call
 * at all.  So every refusal of the composer's applies: desc, opt or place of a wrong `size`; opt->yaw NULL, of a wrong size or without
 * fit_rect or yaw_src; place_src or place_pushed NULL; a bad thin; opt->nms given but of a wrong size or without thr.
 * Behind the pass, calls of the caller's own as before: cm3d_box_velocity (its centres are the placed ones), cm3d_box_tracks. */
int cm3d_lift_pass_placed(const cm3d_lift_pass_desc *desc, const cm3d_lift_pass_options *opt, const cm3d_box_place_desc *place,
                          cm3d_stream_t stream);

/* ---- box size from the fitted extents, pooled over each track (opt-in; a call of its own BEHIND cm3d_box_tracks) ------
 * Added within ABI v5: new symbols only, so CM3D_ABI_VERSION stays.  Every box has the size of its class prior.  cm3d_bev_fit
 * leaves the extents of a vehicle's points at the fitted heading; one frame sees one or two faces, often cut short, so one frame's
 * extent is a lower bound with outliers, but over a track (cm3d_box_tracks) the object is seen from several sides, and an upper
 * quantile of the extents estimates the object itself.  This stage pools them per track, hangs the pooled size on the rectangle by
 * cm3d_box_place's rule, and takes the velocity again on the new centres.  The defaults q = 0.75, min_obs = 2, lo = 0.6, hi = 1.5
 * are UNTUNED, and what the stage does to label quality has not been measured (it cannot be on synthetic scenes).  Host statement to
 * the bit: cm3d_amd.boxsize.box_size_host.  All float64, every product, quotient, sum and difference rounded on its own, no fma, no
 * library call.  M = n_masks, F = n_frames.
 *
 *  box, flags  double[M][CM3D_BOX_STRIDE], int32[M], IN/OUT: only box[i][0] and box[i][1] are ever written; flags is not read
 *  mask_frame  int32[M];  frame_time double[F] seconds;  max_dt as cm3d_box_velocity takes them
 *  fit_rect    double[M][6] as cm3d_bev_fit left it (cx, cy, a, b, hc, hs);  place_src int32[M] as cm3d_box_place left it
 *  prior_wlh   double[n_classes][3];  ego_xyz double[F][3], waymo, thin: exactly as cm3d_box_place takes them
 *  next_match, prev_match int32[M] as cm3d_box_velocity left them;  track_id, track_pos, track_len int32[M] as cm3d_box_tracks did
 *
 *  Members. Mask i is a member iff track_len[i] > 0, 0 <= track_id[i] < M, 0 <= track_pos[i] < track_len[i] and
 *           0 <= mask_frame[i] < F.  Its frame time is frame_time[mask_frame[i]].
 *  Links.   The follower of a member i is j = next_match[i] iff 0 <= j < M, j is a member, track_id[j] == track_id[i] and
 *           track_pos[j] == track_pos[i] + 1.  The predecessor is p = prev_match[i] iff 0 <= p < M, p is a member of the same track_id
 *           and track_pos[p] == track_pos[i] - 1.  Any other value but -1 reads as "no link" and sets status bit 0.  A follower raises
 *           the position by one, so whatever the arrays hold there is no cycle.
 *  Tracks.  The track of a member i is walked from its head h = track_id[i] along the followers.  h must be a member with
 *           track_id[h] == h and track_pos[h] == 0, and the walk must reach i within F steps; a member without such a head or
 *           that the walk does not reach sets status bit 0, is a member WITHOUT A TRACK, observes nothing for others and gets the
 *           ratios 1.0, not pooled, with size_obs 0.  A track has at most one box per frame: no walk takes more than F steps, and one
 *           that is cut at F steps with a follower left sets status bit 1.  What cm3d_box_tracks writes sets neither bit.  No index
 *           outside [0, M) or [0, F) addresses memory.
 *  Observation of a member.  c = box[i][8] >= 0 && box[i][8] < n_classes ? (int)box[i][8] : 0 (as cm3d_box_place reads it);
 *           len0 = prior_wlh[3 c + 1], wid0 = prior_wlh[3 c];  a = fit_rect[i][2], b = fit_rect[i][3].  Member i observes the length iff
 *           place_src[i] != 0, len0 > 0 and lo <= rl <= hi with rl = a / len0 (NaN compares false), the width alike with
 *           rw = b / wid0.  Ratios are pooled, not metres: a track's members may differ in class inside one NMS group.  An extent far
 *           below the prior means the face was not seen, one far above it is background in the list; neither is an observation,
 *           so the pooled value needs no clamp.
 *  Pooling, per track and per dimension: v_0 .. v_{n-1} the observed ratios of the walk's members in track order.  n < min_obs: the
 *           ratio is exactly 1.0 and the dimension is not pooled.  Else k = (int)(q * (double)(n - 1)) and the ratio is the v_p that has
 *           exactly k of the others before it in the order (value, then track position): an order statistic, no interpolation.
 *  Size.    A member with place_src != 0:  len = r_len * len0, wid = r_wid * wid0, size_wlh[i] = (wid, len, prior_wlh[3 c + 2]) -- the
 *           height stays the prior's --, size_src[i] bit 0: the length was pooled, bit 1: the width was.  Every other mask of the batch
 *           (no member, or a member that kept the lane's yaw): its class's prior row bit for bit and size_src 0.
 *           size_ratio double[M][2] = (r_len, r_wid) and size_obs int32[M][2] = the two n for members, zeros elsewhere.
 *  Centre.  A member with place_src != 0 whose sensor and six record values are finite (cm3d_box_place places no other mask): the
 *           rule of cm3d_box_place above, bracket for bracket, with this len and wid for the prior's, the sensor of frame
 *           mask_frame[i]; box[i][0] = x, box[i][1] = y.  It is computed from fit_rect and the sensor, never from the entry centre: a
 *           second call on the same arrays gives the same centres.  size_placed double[M][2]: columns 0, 1 as on entry, every mask.
 *           Columns 2..9 and flags are never written; no NMS is decided again (the tracks stand on the kept set as it is).
 *  Velocity on the new centres, size_vel double[M][2]; zeros for masks that are no members.
 *           smooth_window == 0: cm3d_box_velocity's rule with the follower and predecessor above: the first of central, forward,
 *           backward whose links exist and whose span is <= max_dt, else zeros.
 *           smooth_window = W > 0: cm3d_box_tracks' least-squares rule.  W' = min(W, F), p = track_pos[i], L = track_len[i]; the window
 *           starts min(p, W') predecessors back (or where they end) and holds up to min(p, W') + 1 + min(L - 1 - p, W') members along
 *           the followers (more than F: F, status bit 1); n the members it found; n < 2: zeros; else the six sums and the quotient
 *           as stated there, with (double)n.
 *
 *  CM3D_ERR_ARG before any launch: n_masks < 0, n_frames <= 0, n_classes <= 0, q outside [0, 1] or NaN, min_obs < 1, not
 *  0 < lo <= hi < inf, thin not finite or < 0, max_dt not > 0, smooth_window < 0, a NULL frame_time, prior_wlh or status, a NULL ego_xyz
 *  with waymo == 0, a NULL array that M > 0 needs.  CM3D_ERR_WORKSPACE before any launch: workspace NULL or shorter than
 *  cm3d_box_size_workspace_bytes(n_masks) (five doubles and three int32 per mask).  The first launch initialises the six pure outputs.
 *  status      int32[1], zero it before the call; bits 0 and 1 above are only ever set
 *  A NaN that an operation forms (a centre of inf - inf) has the implementation's sign and payload; every other value is the host's bits.
 *  Launches: k_size_observe, k_size_pool, k_size_apply<WAYMO>, k_size_velocity, one thread per mask each.  Plain stores; the only
 *  atomic is the status word's OR; no allocation, no read-back. */
int64_t cm3d_box_size_workspace_bytes(int32_t n_masks);
int cm3d_box_size(double *box, int32_t *flags, const int32_t *mask_frame, const double *fit_rect, const int32_t *place_src,
                  const double *prior_wlh, int32_t n_classes, const double *ego_xyz, int32_t waymo, double thin,
                  const int32_t *next_match, const int32_t *prev_match, const int32_t *track_id, const int32_t *track_pos,
                  const int32_t *track_len, const double *frame_time, int32_t n_masks, int32_t n_frames, double max_dt,
                  int32_t smooth_window, double q, int32_t min_obs, double lo, double hi, double *size_wlh, int32_t *size_src,
                  double *size_ratio, int32_t *size_obs, double *size_placed, double *size_vel, int32_t *status, void *workspace,
                  int64_t workspace_bytes, cm3d_stream_t stream);

/* ---- opt-in: box height and z from the in-mask points (csrc/vertical.hip) ----------------------------------
 * box[m][2] of the pass is the medoid's z, a point somewhere on the surface the LiDAR saw, and the height of every box is its class's
 * prior.  Here two order statistics of every list's z say where the seen surface begins and ends, and the prior says whether both ends
 * of the object were seen.  Per frame, no track, no yaw fit, every class.  The defaults q_bot = 0.02, q_top = 0.98, min_points = 5,
 * lo = 0.7, hi = 1.3 are UNTUNED, and what the stage does to label quality has not been measured (it cannot be on synthetic scenes).
 * Host statement to the bit: cm3d_amd.boxvertical.box_vertical_host.  M = n_masks.
 *
 *  xyz, off    float[idx_cap][4], int32[M + 1]: the in-mask lists a pass leaves (hit_xyz / hit_off, or cl_xyz / cl_off behind the depth
 *              clustering).  The list of mask m is positions lo_m .. hi_m with lo_m = clamp(off[m], 0, idx_cap) and
 *              hi_m = clamp(off[m + 1], lo_m, idx_cap) (an end below its start: empty), as cm3d_bev_fit and cm3d_depth_cluster clamp
 *              them: whatever off holds, nothing at or beyond idx_cap is read.  n = hi_m - lo_m, z_i the float32 in column 2.  nuScenes
 *              lists and boxes are global, Waymo's both in the vehicle frame: list z and box[m][2] share a frame, there is no switch.
 *  Key.        The order of z is the order of the unsigned key(z) = bits ^ (bits >> 31 ? 0xFFFFFFFF : 0x80000000): a total order on the
 *              bit patterns, -0.0 before +0.0.  The order statistic k of a list is the value whose key has exactly k keys before it in
 *              ascending key order; equal keys are equal bits, so the value needs no tie rule.
 *  Status.     vert_status int32[M], in this order: 2 n == 0;  1 n < min_points;  4 some z_i is not finite (tested before anything is
 *              selected);  0 otherwise.
 *  Quantiles.  Status 0: kb = (int)(q_bot * (double)(n - 1)), kt = (int)(q_top * (double)(n - 1)), vert_z double[M][2] =
 *              ((double)z[kb], (double)z[kt]) = (zb, zt).  Any other status: (0, 0).  Status and vert_z are functions of the lists
 *              alone and are written for every mask, whatever flags says.
 *  Apply.      float64, every operation rounded on its own, no fma, no library call.  c = box[m][8] >= 0 && box[m][8] < n_classes ?
 *              (int)box[m][8] : 0 (as cm3d_box_place reads it), h0 = prior_wlh[3 c + 2].  vert_entry_z double[M] = box[m][2] as on entry,
 *              every mask.  Mask m is judged iff flags[m] & 1, status 0, and h0 is finite and > 0.  Then ext = zt - zb, r = ext / h0:
 *                lo <= r <= hi   both ends seen: vert_src 1, h = ext, z = zb + ext * 0.5
 *                r < lo          the lower part was not seen (a LiDAR above the object and an occluder in front leave it):
 *                                vert_src 2, h = h0, z = zt - h0 * 0.5 -- the prior's height hung on the top seen
 *                r > hi (the list holds ground or a wall), or not judged: vert_src 0, h = h0 bit for bit, box[m][2] untouched
 *              vert_src int32[M], vert_h double[M] = h;  for sources 1 and 2 box[m][2] = z.  Only column 2 of box is ever written, flags is
 *              only read, no NMS is decided again: the circle and rotated NMS and the velocity use x and y only.  z comes from the list,
 *              never from the entry value: a second call on the arrays of the first gives the same box.
 *
 *  CM3D_ERR_ARG before any launch: q_bot, q_top not 0 <= q_bot <= q_top <= 1 (NaN included), min_points < 1, not 0 < lo <= hi < inf,
 *  n_masks < 0, idx_cap < 0, n_classes < 0, and with M > 0: n_classes == 0 or a NULL array (xyz may be NULL when idx_cap == 0).
 *  M == 0: CM3D_OK, nothing is launched.
 *  One launch, k_box_vertical: workgroups of four waves, four masks each.  A list of up to CM3D_VERT_LANE_MAX (64) points sits one
 *  point per lane of its mask's wave and is selected by ballots over the key bits, both order statistics in the same 32 steps, no LDS.
 *  A longer list is selected by all four waves together: a most-significant-digit radix select, four 8-bit digits, integer LDS
 *  counters (sums of integers: the result does not depend on their order), both order statistics in the same passes; up to
 *  CM3D_VERT_LDS_KEYS (4096) keys are staged in LDS by the first pass, a longer list is read again from memory in each of the four.  Every
 *  length up to idx_cap gives the rule's answer.  The apply step is the tail of the same launch, one lane per mask.  Per point one
 *  4-byte load of column 2.  Plain stores, no global atomic, no workspace, no allocation, no read-back. */
#define CM3D_VERT_LANE_MAX 64
#define CM3D_VERT_LDS_KEYS 4096
int cm3d_box_vertical(const float *xyz, const int32_t *off, int32_t n_masks, int32_t idx_cap, double *box, const int32_t *flags,
                      const double *prior_wlh, int32_t n_classes, double q_bot, double q_top, int32_t min_points, double lo, double hi,
                      double *vert_z, double *vert_h, int32_t *vert_src, int32_t *vert_status, double *vert_entry_z,
                      cm3d_stream_t stream);

/* ---- opt-in: ground height under each box from the frame's own sweep (csrc/ground.hip) ------------------------
 * The bottom face of a box is a guess: box[m][2] of the pass is the medoid's z, and the vertical stage sees tops, not bottoms.  Objects
 * stand on the ground, and the ground around an object is what the sweep measures best.  Here every mask bins the z of the points of
 * its frame around its centre -- the first stage behind the projection that looks at a point outside a mask -- and takes a low
 * quantile of the bins as the ground.  Per frame, no track, every class.  The defaults radius R = 3.0 m, quantile Q = 0.1,
 * min_points = 20, window DOWN, UP = 5.0, 0.5 m, ratio LO, HI = 0.7, 1.3 are UNTUNED, all seven, and what the stage does to label
 * quality has not been measured (it cannot be on synthetic scenes).  Host statement to the bit: cm3d_amd.boxground.box_ground_host.
 * M = n_masks, F = n_frames.  All arithmetic of the rule is float64, every operation rounded on its own, no fma, no library call.
 *
 *  Points.     The points of frame f are the rows of its sweeps as the sweep preparation transforms them: the very float32 of
 *              cm3d_sweep_prep's `points`.  Either the cloud is given -- points float[n_rows][4] (16-byte aligned) and pt_off int32[F+1],
 *              frame f at rows [pt_off[f], pt_off[f+1]) -- or, with points or pt_off NULL, the raw rows: raw, raw_stride (4 and up: rows
 *              of that many floats; CM3D_RAW_QUADS: the quad layout), sweep_xf float[n_sweeps][24], sweep_row_off int32[n_sweeps+1],
 *              frame_sweep_off int32[F+1] and halfw as cm3d_sweep_prep takes them, read through its row addressing and fma chains: the
 *              coordinates are bit-identical to the cloud's.  A row the preparation drops (|x| < halfw && |y| < halfw on the sensor-frame
 *              x, y; halfw 0: none) is no point -- in the cloud it is NaN --, and a row with a non-finite coordinate is no point, which
 *              covers the quad layout's padding rows.  Row offsets are clamped into [0, n_rows] and sweep offsets into [0, n_sweeps]
 *              (an end below its start: empty) before use.  Lists and boxes share a frame (nuScenes global, Waymo vehicle).
 *  Masks.      mask_off int32[F+1]: frame f holds masks [mask_off[f], mask_off[f+1]), start clamped to [0, M], end to [start, M].
 *              A mask in no frame's range gets no output.
 *  zref.       zref[m] = the reference height: the array zref double[M] when given, else box[m][2] as on entry.  With a vertical stage
 *              in front the caller hands vert_entry_z, so that zref is box[m][2] as the pass left it.  Written out as ground_zref
 *              double[M]; zref may alias ground_zref, so the stage alone can be run again on what a pass left.
 *  Members.    cx = box[m][0], cy = box[m][1].  A point p (float32 px, py, pz) of the mask's frame is a member of mask m when
 *              dx = (double)px - cx, dy = (double)py - cy, dx*dx + dy*dy <= R*R  (a point on the circle is a member), and with
 *              z0 = zref - DOWN, dz = (DOWN + UP) / 128.0, t = ((double)pz - z0) / dz:  t >= 0 && t < 128.  Its bin is (int)t.
 *              Masks of other frames never see the point; the object's own points are members like any other; a NaN centre has none.
 *  Status.     ground_status int32[M], in this order: 4 cx, cy or zref not finite;  2 no member;  1 n < min_points, n = the number of
 *              members (ground_n int32[M]; 0 with status 4);  0 otherwise.
 *  Ground.     Status 0: k = (int)(Q * (double)(n - 1)), b* = the smallest bin whose cumulative count exceeds k,
 *              ground_z double[M] = z0 + ((double)b* + 0.5) * dz.  Any other status: 0.  Status, n and ground_z are functions of the
 *              cloud, the centre and zref alone and are written for every mask, whatever flags says.  The counts are integers: the
 *              result does not depend on the order in which points arrive.
 *  Apply.      c = box[m][8] >= 0 && box[m][8] < n_classes ? (int)box[m][8] : 0 and h0 = prior_wlh[3 c + 2], as cm3d_box_vertical reads
 *              them.  Mask m is judged iff flags[m] & 1, status 0, and h0 is finite and > 0.  With g = ground_z[m]:
 *                source 1, ground and top: vert_status / vert_z / vert_h are given (the engine has a vertical stage; all three or none),
 *                          vert_status[m] == 0, t = vert_z[m][1], and LO <= (t - g) / h0 <= HI.  Then h = t - g, z = g + h * 0.5.
 *                source 2, the prior stood on the ground: otherwise, if zref - g <= h0 + UP: h = h0, z = g + h0 * 0.5 (the medoid is
 *                          no higher above the ground than the object is tall plus the window's margin; g - zref <= UP holds by the window).
 *                source 0: otherwise, or not judged: box[m][2] untouched -- the vertical stage's value where it wrote one --, and h is
 *                          what it was: vert_h[m] when given, else h0, bit for bit.
 *              ground_src int32[M], ground_h double[M] = h;  for sources 1 and 2 box[m][2] = z.  Only column 2 of box is ever written;
 *              flags is only read and no NMS is decided again (both use x and y only).
 *
 *  CM3D_ERR_ARG before any launch: R not finite and > 0, Q not in [0, 1] (NaN included), min_points < 1, DOWN or UP not finite,
 *  DOWN <= 0, UP < 0, not 0 < LO <= HI < inf, a negative count, neither a cloud (points and pt_off) nor raw rows (raw, sweep_xf,
 *  sweep_row_off, frame_sweep_off; raw_stride 4 and up or CM3D_RAW_QUADS), points not 16-byte aligned, and with M > 0: n_classes == 0,
 *  F == 0, a NULL array (zref and the three vertical arrays may be NULL; those three only together).  M == 0: CM3D_OK, nothing launched.
 *  max_masks_per_frame: the caller's knowledge of mask_off (it sizes the grid; a frame with more masks is still computed, by its
 *  workgroups in turn).
 *  One launch, k_box_ground: one workgroup of sixteen waves per (frame, chunk of the frame's masks).  A chunk holds at most
 *  CM3D_GROUND_CHUNK = 64 masks; the launch takes smaller ones, down to 8, while that gives the chip more workgroups
 *  (cm3d_box_ground_chunk says how many masks for a batch's shape; the result does not depend on it).  The chunk's centres and z0 sit
 *  in LDS beside a 64 x CM3D_GROUND_BINS table of int32 counters (32 KB); the rectangle around the chunk's circles sits in registers,
 *  and a point outside it skips the mask loop.  The workgroup streams the frame's rows once, sweep by sweep with the sweep's transform
 *  uniform; a member does one integer LDS add.  Behind a barrier one wave per mask scans the 128 counters with a wave prefix sum, and the lane that
 *  holds the ground applies the rule.  Per row 12 bytes (quads), 4 raw_stride, or 16 (the cloud), once per chunk of its frame.  Plain
 *  stores, no global atomic, no workspace, no allocation, no read-back. */
#define CM3D_GROUND_BINS 128
#define CM3D_GROUND_CHUNK 64
int32_t cm3d_box_ground_chunk(int32_t n_frames, int32_t max_masks_per_frame);
int cm3d_box_ground(const float *points, const int32_t *pt_off, const float *raw, int32_t raw_stride, const float *sweep_xf,
                    const int32_t *sweep_row_off, const int32_t *frame_sweep_off, int32_t n_sweeps, float halfw, int32_t n_rows,
                    const int32_t *mask_off, int32_t n_frames, int32_t n_masks, int32_t max_masks_per_frame, double *box,
                    const int32_t *flags, const double *prior_wlh, int32_t n_classes, const double *zref, const int32_t *vert_status,
                    const double *vert_z, const double *vert_h, double radius, double quantile, int32_t min_points, double down, double up,
                    double lo, double hi, double *ground_z, int32_t *ground_n, double *ground_h, int32_t *ground_src,
                    int32_t *ground_status, double *ground_zref, cm3d_stream_t stream);

/* ---- opt-in: ground points stripped from the in-mask lists; a per-frame ground grid (csrc/groundstrip.hip) -----
 * Added within ABI v5: new symbols only, so CM3D_ABI_VERSION stays.  A mask drawn around an object covers a strip of road at its foot;
 * the erosion does not remove it and the depth clustering cannot (the road beside the wheels lies at the object's own range).  Here a
 * frame's own sweep gives a grid of ground heights around the frame's origin, and every in-mask list loses the points that lie below
 * its cell's ground plus a margin, between the compaction and the depth clustering: everything behind reads the stripped lists.  The
 * reference has nothing of the kind.  The defaults C = 2.0 m, DOWN, UP = 4.0, 4.0 m, Q = 0.1, N = 8, MARGIN = 0.3 m, MIN_KEEP = 5 are
 * UNTUNED, all seven, and what the stage does to label quality has not been measured (it cannot be on synthetic scenes).  Host
 * statements to the bit: cm3d_amd.groundstrip.ground_grid_host and ground_strip_host.  F = n_frames, M = n_masks.  All arithmetic of
 * the rule is float64, every operation rounded on its own, no fma; counts are integers, so nothing depends on the order in which
 * points arrive.
 *
 *  Grid of frame f.  o = origin[f] (double[F][3]; the engine hands ego_xyz, as the clustering does: zeros on Waymo).  The points are
 *              the rows of the frame's sweeps exactly as cm3d_box_ground defines them (above, "Points."): the very float32 of the
 *              cloud, given as the cloud or as raw rows, without the rows the sweep preparation drops and without rows that have a
 *              non-finite coordinate; every offset clamped as there.  The grid has CM3D_GROUND_GRID_CELLS = 64 cells of side C per
 *              side, centred on o, and every cell a window of CM3D_GROUND_GRID_BINS = 64 bins from oz - DOWN to oz + UP.
 *              For a point p (float32 px, py, pz):  u = ((double)px - ox) / C, iu = floor(u), and iv from py, oy alike.  The point is
 *              inside the grid iff -32 <= iu < 32 && -32 <= iv < 32; its cell is (iv + 32) * 64 + (iu + 32).  With dz = (DOWN + UP) / 64.0
 *              and t = ((double)pz - (oz - DOWN)) / dz, the point is a member of its cell iff 0 <= t < 64; its bin is (int)t.
 *              grid_n int32[F][64*64] = the cell's member count n.  n >= N: k = (int)(Q * (double)(n - 1)), b* = the smallest bin
 *              whose cumulative count exceeds k (cm3d_box_ground's selection), grid_z double[F][64*64] = (oz - DOWN) + ((double)b* + 0.5) * dz.
 *              n < N: grid_z = NaN, "no estimate".  A frame with a non-finite origin has no estimate in any cell and every grid_n 0.
 *  Strip of mask m.  f = mask_frame[m]; the list is positions hit_off[m] .. hit_off[m+1] of hit_xyz (and hit_idx), the offsets clamped
 *              as cm3d_depth_cluster clamps them.  A list point is GROUND iff it lies inside the grid of frame f (iu, iv as above, from
 *              origin[f] and C), its cell has an estimate g, its z is finite and (double)z < g + MARGIN (strict).  A point outside the
 *              grid, in a cell without an estimate, or with a non-finite coordinate is never ground; a frame number outside [0, F) is
 *              a frame without estimates.  kept = the number of non-ground points, dropped = the number of ground points:
 *                gs_status 2: empty list, empty result, gs_dropped 0
 *                gs_status 1: kept < MIN_KEEP: the list is kept whole, gs_dropped 0
 *                gs_status 0: the non-ground points in the list's own order, gs_dropped = dropped (which may be 0)
 *              A non-empty list never becomes empty, so the set of masks with a box cannot change.
 *  gs_off, gs_tile_off int32[M+1], gs_idx int32[idx_cap] (NULL exactly when hit_idx is), gs_xyz float[idx_cap][4], gs_status int32[M]:
 *              the formats of cm3d_depth_cluster's cl_off, cl_tile_off, cl_idx, cl_xyz, cl_status;  gs_dropped int32[M].
 *  workspace   cm3d_ground_strip_workspace_bytes(M, idx_cap) = 4 M + idx_cap bytes, 4-byte aligned (the kept counts; one keep byte per
 *              position).
 *
 *  cm3d_ground_strip_check: CM3D_OK iff C is finite and > 0, DOWN and UP finite and > 0, 0 <= Q <= 1, N >= 1, MARGIN finite,
 *  MIN_KEEP >= 1; anything else, NaN included, is CM3D_ERR_ARG.  Both calls below apply it to the parameters they take, before any
 *  launch; CM3D_ERR_ARG before any launch as well: a negative count, idx_cap <= 0, neither a cloud nor raw rows (as cm3d_box_ground),
 *  points, hit_xyz or gs_xyz not 16-byte aligned, hit_idx and gs_idx not NULL together, and with F > 0 (grid) or M > 0 (strip) a NULL
 *  array (origin and grid_z may be NULL for the strip when F == 0); a workspace too small is CM3D_ERR_WORKSPACE.  cm3d_ground_grid with
 *  F == 0 and cm3d_ground_strip with M == 0: CM3D_OK, nothing launched, nothing written.
 *  cm3d_ground_grid is one launch, k_ground_grid: one workgroup of sixteen waves per (frame, tile of 16 x 16 cells); the tile's
 *  256 x 64 int32 counters are 64 KiB of LDS.  The workgroup streams the whole frame's rows (so a frame's rows are read 16 times, from
 *  L2 after the first), a point outside the tile's rectangle costs two comparisons, a member does one integer LDS add; behind a barrier one
 *  wave per cell scans the 64 counters with a wave prefix sum and the lane that owns rank k writes the cell.  The tile seams are cells
 *  15/16, 31/32 and 47/48 in x and in y.  cm3d_ground_strip is three launches: k_ground_strip, one workgroup per mask (keep bytes, the
 *  count, the MIN_KEEP rule), then the scan and the stable compaction cm3d_depth_cluster uses (csrc/list_compact.h).  No position
 *  >= idx_cap is read or written whatever hit_off holds.  Plain stores, no global atomic, no allocation, no read-back: every run gives
 *  the same bytes, and both calls can be captured in a graph. */
#define CM3D_GROUND_GRID_CELLS 64
#define CM3D_GROUND_GRID_BINS 64
int cm3d_ground_strip_check(double cell, double down, double up, double quantile, int32_t min_points, double margin, int32_t min_keep);
int cm3d_ground_grid(const float *points, const int32_t *pt_off, const float *raw, int32_t raw_stride, const float *sweep_xf,
                     const int32_t *sweep_row_off, const int32_t *frame_sweep_off, int32_t n_sweeps, float halfw, int32_t n_rows,
                     const double *origin, int32_t n_frames, double cell, double down, double up, double quantile, int32_t min_points,
                     double *grid_z, int32_t *grid_n, cm3d_stream_t stream);
int64_t cm3d_ground_strip_workspace_bytes(int32_t n_masks, int32_t idx_cap);
int cm3d_ground_strip(const float *hit_xyz, const int32_t *hit_idx, const int32_t *hit_off, const int32_t *mask_frame, int32_t n_masks,
                      int32_t idx_cap, const double *origin, const double *grid_z, int32_t n_frames, double cell, double margin,
                      int32_t min_keep, int32_t *gs_off, int32_t *gs_tile_off, int32_t *gs_idx, float *gs_xyz, int32_t *gs_status,
                      int32_t *gs_dropped, void *workspace, int64_t workspace_bytes, cm3d_stream_t stream);

/* What the stripped pass needs beyond cm3d_lift_pass_desc.  `size` is sizeof(cm3d_ground_strip_desc) (another value: CM3D_ERR_ARG);
 * the other fields as in cm3d_ground_grid and cm3d_ground_strip (origin: double[desc->n_frames][3]). */
typedef struct cm3d_ground_strip_desc {
    int64_t size;
    const double *origin;
    double *grid_z; int32_t *grid_n;
    int32_t *gs_off; int32_t *gs_tile_off; int32_t *gs_idx; float *gs_xyz; int32_t *gs_status; int32_t *gs_dropped;
    void *ws; int64_t ws_bytes;
    void *ev[2];                 /* optional hipEvent_t, recorded in front of cm3d_ground_grid and behind cm3d_ground_strip */
    double cell, down, up, quantile, margin;
    int32_t min_points, min_keep;
} cm3d_ground_strip_desc;

/* The composed pass with the ground strip: cm3d_lift_pass_composed(desc, opt, place, strip, NULL, stream) (below; host code,
 * csrc/pass_compose.cpp), which states the order and the checks.  No member of cm3d_lift_pass_options: the strip stands in front of
 * every stage the options name, and csrc/pass_options.cpp does not know it.  opt may be NULL (no other stage), place may be NULL.  Its
 * own requirement, checked first: a NULL strip is CM3D_ERR_ARG and NO call at all: it does not fall back to the plain pass. */
int cm3d_lift_pass_stripped(const cm3d_lift_pass_desc *desc, const cm3d_lift_pass_options *opt, const cm3d_box_place_desc *place,
                            const cm3d_ground_strip_desc *strip, cm3d_stream_t stream);

/* ---- opt-in: virtual points from each mask, nearest-depth lifting (csrc/virtual.hip) ---------------------------
 * Added within ABI v5: new symbols only, so CM3D_ABI_VERSION stays.  Every stage behind the compaction refines the one box a mask
 * gets; this one yields the other product of a 2D -> 3D lifter: for every instance mask, pixels sampled inside the eroded mask take the
 * depth of the nearest LiDAR return that projects into the same mask and are unprojected to 3D.  It writes no box, flag or record.  The
 * reference's authors left a beginning of it dead (src/kitti/2d_to_3d.py:613-724, never called); the rule below is this project's own.
 * The defaults K = 50, SEED = 0, MAX_PX = 0 are UNTUNED, and what the points do to a detector has not been measured.  Host statement
 * to the bit: cm3d_amd.virtualpoints.virtual_points_host (steps 2 to 5; step 1 is held against the oracle's project_points).
 * F = n_frames, M = n_masks.
 *
 * Inputs per mask m of frame f = mask_frame[m], with camera c = mask_cam[m] and kk = m - mask_off[f]: the mask's eroded bits -- the
 * bits of `packed` inside the eroded bounds bbox[0..3], read through the stored-rectangle layout bbox[4..7] (cm3d_erode_pack above;
 * both stored forms, the workgroup-per-mask RLE form at the image's row stride included: only words of the eroded bounds are read); the
 * camera record cams[f][c]; the list the medoid saw, positions off[m] .. off[m+1] of `xyz` (the clustered list, else the stripped
 * list, else hit_*), n positions, the offsets clamped into [0, idx_cap] as cm3d_box_vertical clamps them.
 * Parameters: K virtual points per mask, 1 <= K <= CM3D_VP_MAX_K = 1024; SEED uint32; MAX_PX double >= 0, 0 = no limit; KEPT_ONLY:
 * only masks with (flags & 3) == 3 get points; frame_seed uint32[F], one word per frame (the entry points pass the frame's ordinal in
 * the whole job, so that a frame's points do not depend on how the job was cut into batches).
 *
 *  1. Re-projection (cm3d_hit_project).  For every list position, (u, v, depth) by the exact float32 chain of the mask's own camera
 *     applied to that position's x, y, z: the stages with optional t_pre / t_post, k-sequential fmaf, then the K' rows with the
 *     trailing fmaf(0, 1, acc), then IEEE division -- the arithmetic orc_project_points states and the projection kernels implement;
 *     depth is the z behind the last stage.  hit_uvd float[idx_cap][4] = (u, v, depth, 0).  A position of a mask whose frame or camera
 *     number is out of range, and every position outside the lists, is not written.
 *  2. Sampling without replacement, integers only.  A = set pixels of the eroded mask, k = min(K, A).  Pixels are ranked by ascending
 *     y, then ascending x.  For j in [0, k), with uint64 products: lo = j*A / k, hi = (j+1)*A / k, w = hi - lo (always >= 1),
 *     r_j = lo + (h_j mod w), with h_j = mix(SEED ^ frame_seed[f]*0x9E3779B1 ^ kk*0x85EBCA77 ^ j*0xC2B2AE3D), all uint32 with
 *     wraparound, and mix(x): x ^= x>>16; x *= 0x7FEB352D; x ^= x>>15; x *= 0x846CA68B; x ^= x>>16.  The sample is the r_j-th set pixel
 *     (px, py), 0-based; its centre is cx = (float)px + 0.5f, cy = (float)py + 0.5f.  When A <= K every set pixel is drawn exactly once.
 *  3. Nearest return in the image.  Over list positions i in ascending order: du = u_i - cx; dv = v_i - cy; d2 = fmaf(dv, dv, du*du)
 *     in float32.  The winner is the first i with the least d2 under strict <; a NaN never wins.  If no position wins, the sample is
 *     dropped.  If MAX_PX > 0 and (double)d2 > MAX_PX*MAX_PX, the sample is dropped.
 *  4. Unprojection.  Float64 throughout, every operation rounded on its own, no contraction, brackets as written.  d = (double)depth_i;
 *     yc = ((cy - K12) * d) / K11;  xc = (((cx - K02) * d) - K01 * yc) / K00;  zc = d.  Then, for stages from the last to the first:
 *     p -= t_post where the flag says so; p = R^T p with o[r] = (R[0][r]*x + R[1][r]*y) + R[2][r]*z; p -= t_pre where the flag says
 *     so.  The stages are rotations in all three entry points; the rule uses the transpose whatever they hold.  A camera whose K' has a
 *     last row other than (0, 0, 1), K10 != 0, or a zero or non-finite K00 / K11 gives the mask status 4 and no points; so does a
 *     frame or camera number out of range or a stage count outside [0, 3].
 *  5. Output.  Mask m owns rows [m*K, m*K + vp_count[m]).  Kept samples are in ascending j with no holes.  Rows behind the count are
 *     never written.
 *       vp_count  int32[M]       points written for mask m
 *       vp_status int32[M]       0 ok; 1 skipped by KEPT_ONLY; 2 empty list or empty mask (bounds or a stored rectangle that do not
 *                                lie inside the image and the mask's slot count as empty); 4 camera not invertible.  Where several
 *                                hold: 1 before 4 before 2.
 *       vp_xyz    double[M*K][3] point in the frame of the pass's cloud: global on nuScenes, vehicle on Waymo
 *       vp_pix    int32[M*K][2]  the sampled pixel
 *       vp_src    int32[M*K]     the winner's position in the mask's list
 *       vp_depth  float[M*K]     the winner's depth
 *       vp_d2     float[M*K]     the winner's squared pixel distance
 *
 *  cm3d_virtual_points_check: CM3D_OK iff 1 <= K <= CM3D_VP_MAX_K and MAX_PX is finite and >= 0; anything else, NaN included, is
 *  CM3D_ERR_ARG.  cm3d_virtual_points applies it before any launch.  CM3D_ERR_ARG before any launch as well, for both calls: a
 *  negative count, n_cams > CM3D_MAX_CAMS, xyz or hit_uvd not 16-byte aligned, with M > 0 a NULL array (flags may be NULL without
 *  KEPT_ONLY; xyz and hit_uvd with idx_cap == 0) or F == 0 or n_cams == 0; for cm3d_virtual_points W or H < 1, H > CM3D_VP_MAX_ROWS =
 *  4096, or M*H*Wp beyond 2^31 - 1.  M == 0: CM3D_OK, nothing launched, nothing written.
 *  cm3d_hit_project is one launch, k_hit_project: one thread per list position below the last offset, its mask by a search of the
 *  offsets (which ascend); the grid is bounded (2048 workgroups), so a thread takes several positions where the lists are long.
 *  cm3d_virtual_points is one launch, k_virtual_points: one workgroup of four waves per mask -- (a) row popcounts of the eroded
 *  bounds, scanned into LDS, give A; (b) a wave per sample selects rank -> pixel by a search of the row prefix, a wave scan over the
 *  row's words and the bit within the word; (c) the same wave takes the argmin over the list, the lexicographic (d2, position)
 *  minimum, (u, v) staged in LDS for lists of up to CM3D_VP_LDS_LIST = 256 positions and read from memory otherwise; then the keep
 *  flags are scanned in ascending j and the kept samples unprojected, one lane each.  No position >= idx_cap and no word outside a
 *  mask's slot is read whatever the offsets and bbox hold.  Plain stores, no global atomic, no allocation, no read-back: every run
 *  gives the same bytes, and both calls can be captured in a graph. */
#define CM3D_VP_MAX_K 1024
#define CM3D_VP_MAX_ROWS 4096
#define CM3D_VP_LDS_LIST 256
int cm3d_virtual_points_check(int32_t per_mask, double max_px);
int cm3d_hit_project(const float *xyz, const int32_t *off, const int32_t *mask_frame, const int32_t *mask_cam, const float *cams,
                     int32_t n_cams, int32_t n_frames, int32_t n_masks, int32_t idx_cap, float *hit_uvd, cm3d_stream_t stream);
int cm3d_virtual_points(const uint32_t *packed, const int32_t *bbox, int32_t W, int32_t H, const float *cams, int32_t n_cams,
                        const int32_t *mask_off, const int32_t *mask_frame, const int32_t *mask_cam, const int32_t *flags,
                        int32_t n_frames, int32_t n_masks, const float *hit_uvd, const int32_t *off, int32_t idx_cap,
                        int32_t per_mask, uint32_t seed, double max_px, int32_t kept_only, const uint32_t *frame_seed,
                        int32_t *vp_count, int32_t *vp_status, double *vp_xyz, int32_t *vp_pix, int32_t *vp_src, float *vp_depth,
                        float *vp_d2, cm3d_stream_t stream);

/* ---- opt-in: one owner per contested point, exclusive in-mask lists (csrc/pointowner.hip) ----------------------
 * Added within ABI v5: new symbols only, so CM3D_ABI_VERSION stays.  Every stage behind the compaction assumes that an in-mask list
 * holds the points of its own object, and nothing makes that true where masks overlap: the 2D NMS is per class, a pedestrian's mask
 * lies inside the mask of the bus behind them, adjacent cameras see one object twice.  Here every point that several masks of a frame
 * list gets one owner, and every list keeps the positions it owns, between the compaction and the ground strip: everything behind
 * reads the exclusive lists.  ow_owner is also the table of a painted cloud (one instance per LiDAR point).  The reference has
 * nothing of the kind.  The defaults rule = 0 (score), MIN_KEEP = 5 are UNTUNED, both, and what the stage does to label quality has
 * not been measured (it cannot be on synthetic scenes).  Host statement to the bit: cm3d_amd.pointowner.point_owner_host.
 * F = n_frames, M = n_masks, P = max_pts_per_frame.
 *
 *  Lists.      The masks of frame f are [mask_off[f], mask_off[f+1]) (mask_off ascends from 0 to M; every value is clamped into [0, M]
 *              before it is used, and a mask that no frame holds contests nothing: it owns all its positions).  The raw list of mask m
 *              is positions lo_m .. hi_m of hit_idx / hit_xyz, the offsets clamped into [0, idx_cap] exactly as cm3d_depth_cluster
 *              clamps them (hit_off ascends; lists that share positions are not an input); n_m = hi_m - lo_m.  s_m = score[m]
 *              (double).  A NaN score is lower than every number, and two NaNs are equal.
 *  Beats.      For two different masks a, b of one frame:
 *                rule 0 (score):    a beats b iff s_a > s_b; or equal and n_a < n_b; or both equal and a < b
 *                rule 1 (smallest): a beats b iff n_a < n_b; or equal and s_a > s_b; or both equal and a < b
 *              Both are strict total orders within a frame.
 *  Owner.      Position i of mask m (frame f) holds point p = hit_idx[i].  If 0 <= p < P its claimants are the masks of frame f whose
 *              list holds p, and the owner is the claimant that beats all the others.  If p is outside [0, P) the owner is m.  Masks
 *              of different frames never contest.  ow_owner int32[idx_cap] = the owner's batch mask index at every position of every
 *              list; positions beyond the clamped end of the last list are not written.
 *  Result.     kept_m = the number of positions of m whose owner is m:
 *                ow_status 2: empty list, empty result, ow_lost 0
 *                ow_status 1: kept_m < MIN_KEEP: the list is kept whole, ow_lost 0 (ow_owner still names the owners)
 *                ow_status 0: the positions the list owns, in its own order, ow_lost = n_m - kept_m (which may be 0)
 *              A non-empty list never becomes empty, so the set of masks with a box cannot change.
 *  ow_off, ow_tile_off int32[M+1], ow_idx int32[idx_cap], ow_xyz float[idx_cap][4], ow_status int32[M]: the formats of
 *              cm3d_depth_cluster's cl_off, cl_tile_off, cl_idx, cl_xyz, cl_status;  ow_lost int32[M].
 *  workspace   cm3d_point_owner_workspace_bytes(F, P, M, idx_cap) = 16 M + 4 F P + idx_cap bytes, 4-byte aligned (the kept counts,
 *              the ranks, the frames and the masks by rank; the owner table int32[F][P]; one keep byte per position).  Nothing
 *              depends on what it held before the call.
 *
 *  cm3d_point_owner_check: CM3D_OK iff rule is 0 or 1 and MIN_KEEP >= 1; anything else is CM3D_ERR_ARG.  cm3d_point_owner applies it
 *  before any launch; CM3D_ERR_ARG before any launch as well: a negative count, idx_cap <= 0, a NULL hit_idx (the stage cannot do
 *  without it), with M > 0 a NULL array, hit_xyz or ow_xyz not 16-byte aligned; a workspace too small is CM3D_ERR_WORKSPACE.  M == 0:
 *  CM3D_OK, nothing launched, nothing written.
 *  Six launches: k_owner_rank, one thread per mask (its frame by a search of mask_off; its rank = the number of the frame's masks it
 *  beats, and the inverse table); k_owner_claim twice, one workgroup per mask: first 0 into the table entry of every listed point --
 *  only entries that are read are cleared, not the 4 F P bytes of the table --, then an integer maximum of rank + 1 on it (a maximum
 *  does not depend on the order of arrival); k_owner_resolve, one workgroup per mask (entry -> owner, ow_owner, keep bytes, the count,
 *  the MIN_KEEP rule); then the scan and the stable compaction cm3d_depth_cluster uses (csrc/list_compact.h).  No position >= idx_cap
 *  and no table entry outside [0, F P) is read or written whatever hit_off and hit_idx hold.  Integer atomics only, no float atomic,
 *  no allocation, no read-back: every run gives the same bytes, and the call can be captured in a graph. */
int cm3d_point_owner_check(int32_t rule, int32_t min_keep);
int64_t cm3d_point_owner_workspace_bytes(int32_t n_frames, int32_t max_pts_per_frame, int32_t n_masks, int32_t idx_cap);
int cm3d_point_owner(const float *hit_xyz, const int32_t *hit_idx, const int32_t *hit_off, const int32_t *mask_off, int32_t n_frames,
                     int32_t n_masks, int32_t idx_cap, int32_t max_pts_per_frame, const double *score, int32_t rule, int32_t min_keep,
                     int32_t *ow_owner, int32_t *ow_off, int32_t *ow_tile_off, int32_t *ow_idx, float *ow_xyz, int32_t *ow_status,
                     int32_t *ow_lost, void *workspace, int64_t workspace_bytes, cm3d_stream_t stream);

/* What the owned pass needs beyond cm3d_lift_pass_desc.  `size` is sizeof(cm3d_point_owner_desc) (another value: CM3D_ERR_ARG); the
 * other fields as in cm3d_point_owner. */
typedef struct cm3d_point_owner_desc {
    int64_t size;
    int32_t *ow_owner; int32_t *ow_off; int32_t *ow_tile_off; int32_t *ow_idx; float *ow_xyz; int32_t *ow_status; int32_t *ow_lost;
    void *ws; int64_t ws_bytes;
    void *ev[2];                 /* optional hipEvent_t, recorded in front of and behind cm3d_point_owner */
    int32_t rule, min_keep;
} cm3d_point_owner_desc;

/* ---- One pass with any opt-in stage, those without a member in cm3d_lift_pass_options included ----
 * Added within ABI v5: a new symbol only, so CM3D_ABI_VERSION stays.  Host code (csrc/pass_compose.cpp; behind the ownership and the
 * strip it enters csrc/pass_options.cpp, which does not know these stages, on the lists that are left).  This is the one statement of
 * the order of a pass with a placement, a ground strip or a point ownership: cm3d_lift_pass_placed, _stripped and _owned and
 * cm3d_amd.lifting.LiftEngine.run end here.  Enqueues on `stream`, stopping at and returning the first error (a failed event call:
 * CM3D_ERR_LAUNCH); NULL events are skipped; no descriptor of the caller's is written.  opt, place, strip and owner may each be NULL.
 *
 *   every descriptor is checked first, CM3D_ERR_ARG and NO call at all, whichever is bad:
 *     desc     NULL or of a wrong `size`
 *     owner    desc without hit_idx; owner's `size`, a NULL ow_* array, a NULL workspace pointer, cm3d_point_owner_check of its parameters
 *     strip    its `size`, a NULL array (gs_idx only when desc has hit_idx), a NULL workspace pointer, cm3d_ground_strip_check of its
 *              parameters
 *     opt      its `size` and its members as in cm3d_lift_pass_opt, for the lists the pass goes on with: yaw's hit_xyz, hit_off,
 *              medoid_pos each NULL or what is derived below; cluster's cl_idx when those lists have a hit_idx
 *     place    its `size`; place_src or place_pushed NULL; thin not in [0, DBL_MAX]; opt NULL, opt->yaw NULL or without fit_rect or
 *              yaw_src (a placement needs the yaw fit)
 *   owner or strip ?  cm3d_lift_pass_head(desc)
 *   owner   ?  record owner->ev[0]; cm3d_point_owner (desc's lists, mask_off, score -> the ow_* arrays); record owner->ev[1]
 *   strip   ?  record strip->ev[0]; cm3d_ground_grid (desc's sweep rows: the cloud where desc has points, else the raw rows; origin ->
 *              grid_z, grid_n); cm3d_ground_strip (the ow_* lists, else desc's lists -> the gs_* arrays); record strip->ev[1]
 *   the lists the pass goes on with: the gs_* arrays, else the ow_* arrays, else desc's
 *   owner or strip ?  cluster ?  record cluster->ev[0]; cm3d_depth_cluster (the lists -> the cl_* arrays); record cluster->ev[1]
 *                     cm3d_lift_pass_tail(desc')     desc' = desc with hit_off, tile_off, hit_idx, hit_xyz = the cl_* arrays, else the
 *                                                    lists; tile_work = NULL
 *                  :  cluster and the plain pass as in cm3d_lift_pass_opt (the head runs there, in front of the clustering)
 *   filter  ?  as in cm3d_lift_pass_opt
 *   yaw     ?  cm3d_yaw_fit_boxes' sequence          lists = cluster ? cl_xyz, cl_off : the lists the pass goes on with
 *   place   ?  record place->ev[0]
 *              cm3d_box_place                        box, flags, mask_off, prior_wlh, nms_group, nms_thr, ego_xyz ... of desc; fit_rect,
 *                                                    yaw_src of opt->yaw; waymo = pose_inv != NULL; bound as the box launch's
 *              record place->ev[1]
 *   nms     ?  cm3d_box_rotated_nms                  as in cm3d_lift_pass_opt; with a placement it judges the placed boxes and overwrites
 *                                                    the circle NMS's verdict (the stages in front run on a copy of opt with nms = NULL)
 *   place, strip and owner all NULL: exactly cm3d_lift_pass_opt(desc, opt) for a desc of the right size
 *   medoid_pos is then a position in the lists the medoid saw: cl_*, else gs_*, else ow_*, else desc's.  Behind the pass the caller's own
 *   calls as before; cm3d_box_vertical reads the lists the yaw fit reads.  cm3d_box_ground stays what it is: it streams the sweep and
 *   does not read the grid. */
int cm3d_lift_pass_composed(const cm3d_lift_pass_desc *desc, const cm3d_lift_pass_options *opt, const cm3d_box_place_desc *place,
                            const cm3d_ground_strip_desc *strip, const cm3d_point_owner_desc *owner, cm3d_stream_t stream);

/* The composed pass with the point ownership: cm3d_lift_pass_composed with the same arguments (above).  opt, place and strip may be
 * NULL.  Its own requirement, checked first: a NULL owner is CM3D_ERR_ARG and NO call at all: it does not fall back to another pass. */
int cm3d_lift_pass_owned(const cm3d_lift_pass_desc *desc, const cm3d_lift_pass_options *opt, const cm3d_box_place_desc *place,
                         const cm3d_ground_strip_desc *strip, const cm3d_point_owner_desc *owner, cm3d_stream_t stream);

#ifdef __cplusplus
}
#endif
#endif /* CM3D_HIP_H */
