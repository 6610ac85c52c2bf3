// The two run-length -> erode -> pack kernels of masks.hip.  masks.hip includes this file twice: once as they have always been
// (k_rle_erode_pack, k_rle_erode_pack_wave: every run list covers the W x H image) and once SIZED (k_rle_erode_pack_sized,
// k_rle_erode_pack_wave_sized, behind cm3d_rle_erode_pack_sized): there a mask's run list describes an image of its own size
// (w, h) = mask_wh[m] <= (W, H), pasted top-left into the W x H canvas (rule R, include/cm3d_hip.h).  (gw, gh) is the geometry of
// the run list -- pixel index -> (x, y), the set pixels' rectangle, where the list ends --; W, H, Wp stay what they are for storage
// and for what counts as outside: canvas pixels beyond the mask's own image are never painted, hence zeros, and the canvas's
// border rule applies where the two coincide.  Textual inclusion, not a template: the code of the plain pair stays the very code
// it was (profiles/mixed_sizes_resources.txt).
//   RLE_SIZED 0 / 1, RLE_KERNEL_BLOCK, RLE_KERNEL_WAVE: the kernels' names, RLE_SIZE_PARAM: empty / the mask_wh parameter

// f1: run lengths -> packed tile in LDS -> erode -> store.  ONE workgroup per mask, one launch:
//   pass 1 streams the run lengths (block scan, 2048 runs per step) and finds the rectangle of the set pixels;
//   then, tile by tile over that rectangle (the tile is as wide as the rectangle + halo and as tall as LDS
//   allows, so nearly every mask is a single tile): clear, paint the 1-runs, erode, store, reduce the bbox.
// A mask of up to 2048 runs keeps its runs in registers between the passes; longer lists are streamed again
// per tile.  Nothing outside the rectangle is written; the workgroup owns the mask's bbox (no global atomics).
__global__ __launch_bounds__(EP_THREADS) void RLE_KERNEL_BLOCK(const uint32_t *__restrict__ cnts_all,
                                                                const int32_t *__restrict__ rle_off, int W, int H, int Wp,
                                                                int lds_words, uint32_t *__restrict__ packed,
                                                                int32_t *__restrict__ bbox RLE_SIZE_PARAM)
{
    extern __shared__ __align__(16) uint32_t s_rows[];
    __shared__ int s_w[EP_THREADS / 64];
    __shared__ int s_rect[4];                   // ylo, xlo, yhi, xhi of the set pixels
    __shared__ int s_bb[4];                     // bbox of the eroded pixels
    const int m = blockIdx.x;
    const int o = rle_off[m], n = rle_off[m + 1] - o;
    const uint32_t *cnts = cnts_all + o;
#if RLE_SIZED       // (clamped into the canvas: no table content can move a write outside the mask's slot)
    const int gw = min(max(mask_wh[2 * m], 1), W), gh = min(max(mask_wh[2 * m + 1], 1), H);
#else
    const int gw = W, gh = H;
#endif
    if (threadIdx.x == 0) {
        s_rect[0] = 0x7FFFFFFF; s_rect[1] = 0x7FFFFFFF; s_rect[2] = -1; s_rect[3] = -1;
        s_bb[0] = 0x7FFFFFFF; s_bb[1] = 0x7FFFFFFF; s_bb[2] = -1; s_bb[3] = -1;
    }
    // ---- pass 1: rectangle
    int v0[RS_PER], start0 = 0;                 // the first chunk stays in registers
    {
        int carry = 0;
        int ylo = 0x7FFFFFFF, yhi = -1, xlo = 0x7FFFFFFF, xhi = -1;
        for (int base = 0; base < n; base += RS_CHUNK) {
            int v[RS_PER];
            int run = rle_chunk_scan(cnts, n, base, v, s_w, carry);
            if (base == 0) {
                start0 = run;
#pragma unroll
                for (int q = 0; q < RS_PER; ++q) v0[q] = v[q];
            }
            const int i0 = base + (int)threadIdx.x * RS_PER;
#pragma unroll
            for (int q = 0; q < RS_PER; ++q) {
                if (((i0 + q) & 1) && v[q] > 0) {                     // a 1-run [s, e)
                    const int s = run, e = run + v[q];
                    const int ys = s / gw, ye = (e - 1) / gw;
                    ylo = min(ylo, ys); yhi = max(yhi, ye);
                    if (ys == ye) { xlo = min(xlo, s - ys * gw); xhi = max(xhi, e - 1 - ys * gw); }
                    else { xlo = 0; xhi = gw - 1; }
                }
                run += v[q];
            }
        }
        ylo = cm3d_wave_min(ylo); xlo = cm3d_wave_min(xlo); yhi = cm3d_wave_max(yhi); xhi = cm3d_wave_max(xhi);
        __syncthreads();                        // s_rect initialised
        if (cm3d_lane() == 0 && yhi >= 0) {
            atomicMin(&s_rect[0], ylo); atomicMin(&s_rect[1], xlo); atomicMax(&s_rect[2], yhi); atomicMax(&s_rect[3], xhi);
        }
        __syncthreads();
    }
    const int ry0 = s_rect[0], ry1 = min(s_rect[2], gh - 1);
    if (s_rect[2] < 0) {                        // empty mask
        if (threadIdx.x == 0) { bbox[CM3D_BBOX_STRIDE * m + 0] = 0x7FFFFFFF; bbox[CM3D_BBOX_STRIDE * m + 1] = 0x7FFFFFFF; bbox[CM3D_BBOX_STRIDE * m + 2] = -1; bbox[CM3D_BBOX_STRIDE * m + 3] = -1; }
        if (threadIdx.x >= 4 && threadIdx.x < 8) bbox[CM3D_BBOX_STRIDE * m + threadIdx.x] = 0;
        return;
    }
    const int xw0 = s_rect[1] >> 5, wc = (min(s_rect[3], gw - 1) >> 5) - xw0 + 1, lw = wc + 2;
    int br = lds_words / lw - 2;                // output rows per tile
    br = min(br, ry1 - ry0 + 1);
    const uint32_t pad = (W & 31) ? ~((1u << (W & 31)) - 1u) : 0u;
    // ---- tiles
    for (int y0 = ry0; y0 <= ry1; y0 += br) {
        __syncthreads();                        // the previous tile's readers are done
        const int rows = min(br, ry1 - y0 + 1);
        const int lrows = rows + 2;
        const int ya = y0 - 1;                  // image row of LDS row 0
        // initial tile: ones outside the image, zeros inside; pad bits of a row's last word are ones
        {
            int r = (int)threadIdx.x / lw, c = (int)threadIdx.x - r * lw;
            const int dr_step = EP_THREADS / lw, dc_step = EP_THREADS - dr_step * lw;
            for (int q = threadIdx.x; q < lrows * lw; q += EP_THREADS, r += dr_step, c += dc_step) {
                if (c >= lw) { c -= lw; ++r; }
                const int y = ya + r, xw = xw0 - 1 + c;
                uint32_t v = 0u;
                if (y < 0 || y >= H || xw < 0 || xw >= Wp) v = 0xFFFFFFFFu;
                else if (xw == Wp - 1) v = pad;
                s_rows[q] = v;
            }
        }
        __syncthreads();
        const int yc0 = max(ya, 0), yc1 = min(ya + lrows - 1, gh - 1);           // image rows held in LDS
        const uint32_t px0 = (uint32_t)yc0 * gw, px1 = (uint32_t)(yc1 + 1) * gw;   // pixel range [px0, px1)
        // every 1-run (odd index) overlapping the tile sets its bits (all of them lie inside the word range)
        if (n <= RS_CHUNK) {
            int run = start0;
            const int i0 = (int)threadIdx.x * RS_PER;
#pragma unroll
            for (int q = 0; q < RS_PER; ++q) {
                if (((i0 + q) & 1) && v0[q] > 0) {
                    const uint32_t s = max((uint32_t)run, px0), e = min((uint32_t)(run + v0[q]), px1);
                    rle_paint(s_rows, lw, xw0, ya, gw, s, e);
                }
                run += v0[q];
            }
        } else {
            int carry = 0;
            for (int base = 0; base < n; base += RS_CHUNK) {
                int v[RS_PER];
                int run = rle_chunk_scan(cnts, n, base, v, s_w, carry);
                const int i0 = base + (int)threadIdx.x * RS_PER;
#pragma unroll
                for (int q = 0; q < RS_PER; ++q) {
                    if (((i0 + q) & 1) && v[q] > 0) {
                        const uint32_t s = max((uint32_t)run, px0), e = min((uint32_t)(run + v[q]), px1);
                        rle_paint(s_rows, lw, xw0, ya, gw, s, e);
                    }
                    run += v[q];
                }
                if ((uint32_t)carry >= px1) break;          // uniform: the rest lies below the tile
            }
        }
        __syncthreads();
        erode_tile_store(s_rows, lw, wc, xw0, ya, rows, W, Wp, packed + (size_t)m * H * Wp, s_bb);
    }
    __syncthreads();
    if (threadIdx.x < 4) bbox[CM3D_BBOX_STRIDE * m + threadIdx.x] = s_bb[threadIdx.x];
    // this form stores image rows as they are: the stored rectangle is the whole image
    if (threadIdx.x >= 4 && threadIdx.x < 8) bbox[CM3D_BBOX_STRIDE * m + threadIdx.x] = threadIdx.x == 6 ? Wp : (threadIdx.x == 7 ? H : 0);
}

// ---------------------------------------------------------------------------
// the one-wave-per-mask form (described in masks.hip, above its helpers)
__global__ __launch_bounds__(RW_THREADS, 5) void RLE_KERNEL_WAVE(const uint32_t *__restrict__ cnts_all, const int32_t *__restrict__ rle_off,
                                                                  int n_masks, int W, int H, int Wp, int lds_words,
                                                                  uint32_t *__restrict__ packed, int32_t *__restrict__ bbox, int max_bands,
                                                                  const RwBegin begin RLE_SIZE_PARAM)
{
    // cm3d_rle_erode_pack_begin: the per-pass reset (cm3d_batch_begin's: status word, hit counts, removed-row bits) rides on this launch -- the
    // first of a pass -- instead of a launch of its own.  Nothing in this kernel reads or writes those arrays; whatever does runs behind it.
    if (begin.status) {
        const long long i0 = (long long)blockIdx.x * blockDim.x + threadIdx.x, step = (long long)gridDim.x * blockDim.x;
        if (i0 < CM3D_STATUS_WORDS) begin.status[i0] = 0;
        for (long long i = i0; i < begin.n_masks; i += step) begin.hit_count[i] = 0;
        for (long long i = i0; i < begin.removed_words; i += step) begin.removed_bits[i] = 0u;
    }
    extern __shared__ __align__(16) uint32_t s_all[];
    __shared__ int s_part[RW_WAVES][4];                         // the bands' shares of the bounding box
    const int lane = cm3d_lane(), wave = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    // max_bands > 1: one workgroup per mask, wave w its band w; 1: one wave per mask.  The launch's grid covers the masks in both forms,
    // so the loop below runs once: its stride is kept only so that the kernel's code stays what it was when a smaller grid could be forced.
    const int m_first = max_bands > 1 ? (int)blockIdx.x : (int)blockIdx.x * RW_WAVES + wave;
    const int m_stride = max_bands > 1 ? (int)gridDim.x : (int)gridDim.x * RW_WAVES;
    for (int m = m_first; m < n_masks; m += m_stride) {         // (max_bands > 1: the grid covers the masks, one round, uniform over the workgroup)
    const int band = max_bands > 1 ? wave : 0;
    uint32_t *s_rows = s_all + (size_t)wave * lds_words;
    const int o = rle_off[m], n = rle_off[m + 1] - o;
    const uint32_t *cnts = cnts_all + o;
    const int nb = max(1, min(max_bands, (n + RW_BAND_RUNS - 1) / RW_BAND_RUNS));     // bands = waves at work on this mask
    int bminx = 0x7FFFFFFF, bminy = 0x7FFFFFFF, bmaxx = -1, bmaxy = -1;               // bounding box of the band's eroded pixels
    int rect_x = 0, rect_y = 0, rect_w = 0, rect_h = 0;                               // the stored rectangle (uniform; every band finds the same)
#if RLE_SIZED       // uniform over the wave: scalar registers (clamped into the canvas: no table content can move a write outside the mask's slot)
    const int gw = __builtin_amdgcn_readfirstlane(min(max(mask_wh[2 * m], 1), W));
    const int gh = __builtin_amdgcn_readfirstlane(min(max(mask_wh[2 * m + 1], 1), H));
#else
    const int gw = W, gh = H;
#endif
    if (band < nb) {
    const float rcpW = 1.0f / (float)gw;
    // ---- pass 1: rectangle of the set pixels (the 1-runs of the first chunk stay in registers)
    int s0[RW_PER / 2], l0[RW_PER / 2];
    int ylo = 0x7FFFFFFF, yhi = -1, xlo = 0x7FFFFFFF, xhi = -1;
    int carry0 = 0;                             // pixels covered by the first chunk of runs
    {
        int carry = 0;
#pragma unroll 1
        for (int base = 0; base < n; base += RW_CHUNK) {
            int v[RW_PER], s1[RW_PER / 2], l1[RW_PER / 2];
            const int run = rw_chunk_scan(cnts, n, base, lane, v, carry);
            rw_one_runs(run, v, s1, l1);
            if (base == 0) {
                carry0 = carry;
#pragma unroll
                for (int q = 0; q < RW_PER / 2; ++q) { s0[q] = s1[q]; l0[q] = l1[q]; }
            }
#pragma unroll 1
            for (int q = 0; q < RW_PER / 2; ++q) {
                const int s = s1[0], len = l1[0];
#pragma unroll
                for (int r = 0; r + 1 < RW_PER / 2; ++r) { s1[r] = s1[r + 1]; l1[r] = l1[r + 1]; }
                if (len > 0) {                                          // a 1-run [s, s + len)
                    const int ys = rw_row_of((uint32_t)s, gw, rcpW), ye = rw_row_of((uint32_t)(s + len - 1), gw, rcpW);
                    ylo = min(ylo, ys); yhi = max(yhi, ye);
                    if (ys == ye) { xlo = min(xlo, s - ys * gw); xhi = max(xhi, s + len - 1 - ys * gw); }
                    else { xlo = 0; xhi = gw - 1; }
                }
            }
        }
        ylo = __builtin_amdgcn_readfirstlane(cm3d_wave_min(ylo)); xlo = __builtin_amdgcn_readfirstlane(cm3d_wave_min(xlo));
        yhi = __builtin_amdgcn_readfirstlane(cm3d_wave_max(yhi)); xhi = __builtin_amdgcn_readfirstlane(cm3d_wave_max(xhi));
    }
    if (!(yhi < 0)) {                        // (an empty mask: nothing to paint, the box stays empty)
    const int my0 = ylo, my1 = min(yhi, gh - 1);                        // rows of the mask's set pixels; this wave's band of them:
    const int bandr = (my1 - my0 + nb) / nb;
    const int ry0 = my0 + band * bandr, ry1 = min(my1, ry0 + bandr - 1);
    const int xw0 = xlo >> 5, wc = (min(xhi, gw - 1) >> 5) - xw0 + 1, lw = wc + 2;
    rect_x = xw0; rect_y = my0; rect_w = max(wc, 0); rect_h = max(my1 - my0 + 1, 0);     // (never negative: run lengths that overshoot W*H must not poison the table entries)
    int br = lds_words / lw - 2;                // output rows per tile
    br = min(br, ry1 - ry0 + 1);
    const uint32_t pad = (W & 31) ? ~((1u << (W & 31)) - 1u) : 0u;
    const uint32_t tail_mask = ~pad;
    uint32_t *out_mask = packed + (size_t)m * H * Wp;
    // (bounding box of the eroded pixels: per lane the OR of its column's words and its first / last non-empty row)
    const int nseg = max(1, 64 / wc);           // stretches of rows a tile is cut into (one lane per stretch and word column)
    for (int y0 = ry0; y0 <= ry1; y0 += br) {
        const int rows = min(br, ry1 - y0 + 1);
        const int lrows = rows + 2;
        const int ya = y0 - 1;                  // image row of LDS row 0
        rw_lds_sync();                          // the previous tile's readers are done
        // initial tile: zeros inside the image (16 bytes per lane and step), then the few places that are ones
        {
            const int nq = (lrows * lw + 3) >> 2;
            for (int q = lane; q < nq; q += 64) reinterpret_cast<uint4 *>(s_rows)[q] = make_uint4(0u, 0u, 0u, 0u);
            if (xw0 == 0 || xw0 + wc == Wp || ya < 0 || ya + lrows - 1 >= H) {          // the rectangle touches the image's border (uniform)
                rw_lds_sync();
                if (xw0 == 0) for (int r = lane; r < lrows; r += 64) s_rows[r * lw] = 0xFFFFFFFFu;                       // left of the image
                if (xw0 + wc == Wp) {
                    for (int r = lane; r < lrows; r += 64) { s_rows[r * lw + lw - 1] = 0xFFFFFFFFu; if (pad) s_rows[r * lw + lw - 2] = pad; }
                }
                rw_lds_sync();
                if (ya < 0) for (int c = lane; c < lw; c += 64) s_rows[c] = 0xFFFFFFFFu;                                  // above the image
                if (ya + lrows - 1 >= H) for (int c = lane; c < lw; c += 64) s_rows[(lrows - 1) * lw + c] = 0xFFFFFFFFu;  // below it
            }
        }
        rw_lds_sync();
        const int yc0 = max(ya, 0), yc1 = min(ya + lrows - 1, gh - 1);           // image rows held in LDS
        const uint32_t px0 = (uint32_t)yc0 * gw, px1 = (uint32_t)(yc1 + 1) * gw;   // pixel range [px0, px1)
        {
            int carry = 0;
#pragma unroll 1
            for (int base = 0; base < n; base += RW_CHUNK) {
                int s1[RW_PER / 2], l1[RW_PER / 2];
                if (base == 0) {                                    // uniform
#pragma unroll
                    for (int q = 0; q < RW_PER / 2; ++q) { s1[q] = s0[q]; l1[q] = l0[q]; }
                } else {
                    int v[RW_PER];
                    const int run = rw_chunk_scan(cnts, n, base, lane, v, carry);
                    rw_one_runs(run, v, s1, l1);
                }
#pragma unroll 1
                for (int q = 0; q < RW_PER / 2; ++q) {
                    const uint32_t rs = (uint32_t)s1[0], re = rs + (uint32_t)l1[0];
#pragma unroll
                    for (int r = 0; r + 1 < RW_PER / 2; ++r) { s1[r] = s1[r + 1]; l1[r] = l1[r + 1]; }
                    uint32_t ps = max(rs, px0);
                    const uint32_t pe = min(re, px1);
                    while (ps < pe) {                               // (one round per image row the run touches)
                        const int y = rw_row_of(ps, gw, rcpW);
                        const uint32_t x = ps - (uint32_t)y * gw;
                        const uint32_t xe = min((uint32_t)gw, x + (pe - ps));   // exclusive end within this row
                        uint32_t *row = s_rows + (y - ya) * lw + 1 - xw0;      // row[xw] = packed word xw
                        const uint32_t w0 = x >> 5, w1 = (xe - 1) >> 5;
                        const uint32_t m0 = 0xFFFFFFFFu << (x & 31);
                        const uint32_t m1 = 0xFFFFFFFFu >> (31 - ((xe - 1) & 31));
                        if (w0 == w1) atomicOr(&row[w0], m0 & m1);
                        else {
                            atomicOr(&row[w0], m0);
                            for (uint32_t w = w0 + 1; w < w1; ++w) atomicOr(&row[w], 0xFFFFFFFFu);
                            atomicOr(&row[w1], m1);
                        }
                        ps += xe - x;
                    }
                }
                if (base == 0) carry = carry0;                      // pixels covered by the first chunk (pass 1)
                if ((uint32_t)carry >= px1) break;                  // uniform: the rest lies below the tile
            }
        }
        rw_lds_sync();
        // erosion, sliding window down a word column: h(r) = centre & left & right of LDS row r; out(r) = h(r-1) & h(r) & h(r+1)
        const int rps = (rows + nseg - 1) / nseg;           // output rows per band
        for (int cb = 0; cb < wc; cb += 64) {
            const int seg = wc >= 64 ? 0 : lane / wc, c = wc >= 64 ? cb + lane : lane - seg * wc;
            const int r0 = seg * rps, r1 = min(rows, r0 + rps);                  // output rows [r0, r1) of the tile (LDS rows r0+1 .. r1)
            if (c < wc && seg < nseg && r0 < r1) {
                const uint32_t *row = s_rows + r0 * lw + c;
                auto hrow = [&](const uint32_t *rw) {
                    const uint32_t ce = rw[1];
                    return ce & ((ce << 1) | (rw[0] >> 31)) & ((ce >> 1) | (rw[2] << 31));
                };
                uint32_t h0 = hrow(row), h1 = hrow(row + lw);
                row += 2 * lw;
                const int xw = xw0 + c;
                const uint32_t keep = xw == Wp - 1 ? tail_mask : 0xFFFFFFFFu;
                // the eroded words go out as PACKED ROWS OF THE RECTANGLE of the mask's set pixels (word columns xw0 .. xw0 + wc - 1, rows
                // my0 .. my1), one row behind the other: consecutive stores fill whole cache lines.  At the image's row stride a mask's
                // 40-byte row pieces were 1.5 M partial-line writes per batch, and with three batches in flight they cost every kernel
                // that streams from HBM beside them: 20 of 142 us per pass, 4 in this form.
                uint32_t *dst = out_mask + (size_t)(ya + 1 + r0 - my0) * wc + (xw - xw0);
                uint32_t colany = 0u;
                int first = 0x7FFFFFFF, last = -1;
                for (int r = r0; r < r1; ++r, row += lw, dst += wc) {
                    const uint32_t h2 = hrow(row);
                    const uint32_t e = h0 & h1 & h2 & keep;
                    h0 = h1; h1 = h2;
                    *dst = e;
                    colany |= e;
                    if (e) { first = min(first, r); last = r; }
                }
                if (colany) {
                    bminx = min(bminx, xw * 32 + __builtin_ctz(colany));
                    bmaxx = max(bmaxx, xw * 32 + 31 - __builtin_clz(colany));
                    bminy = min(bminy, ya + 1 + first);
                    bmaxy = max(bmaxy, ya + 1 + last);
                }
            }
        }
    }
    }
    }
    bminx = cm3d_wave_min(bminx); bminy = cm3d_wave_min(bminy); bmaxx = cm3d_wave_max(bmaxx); bmaxy = cm3d_wave_max(bmaxy);
    if (nb == 1) {                              // uniform over the workgroup (or max_bands == 1): one band, no hand-over
        if (band == 0 && lane < 8)
            bbox[CM3D_BBOX_STRIDE * m + lane] = lane == 0 ? bminx : lane == 1 ? bminy : lane == 2 ? bmaxx : lane == 3 ? bmaxy
                                                : lane == 4 ? rect_x : lane == 5 ? rect_y : lane == 6 ? rect_w : rect_h;
        continue;
    }
    if (lane < 4) s_part[wave][lane] = lane == 0 ? bminx : lane == 1 ? bminy : lane == 2 ? bmaxx : bmaxy;
    __syncthreads();
    if (wave == 0 && lane < 4) {
        int v = s_part[0][lane];
        for (int w = 1; w < RW_WAVES; ++w) v = lane < 2 ? min(v, s_part[w][lane]) : max(v, s_part[w][lane]);
        bbox[CM3D_BBOX_STRIDE * m + lane] = v;
    }
    if (wave == 0 && lane >= 4 && lane < 8) bbox[CM3D_BBOX_STRIDE * m + lane] = lane == 4 ? rect_x : lane == 5 ? rect_y : lane == 6 ? rect_w : rect_h;
    }
}
