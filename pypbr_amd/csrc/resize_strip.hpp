// resize_strip.hpp -- the general form of the resize: ONE kernel (resize_strip_kernel), tile by tile through an LDS strip, HEIGHT pass first.
// The forward (resize.hip) runs it with tap tables derived from the filter, the gradient (resize_backward.hip) with the transposed tables.
//
// The tap pattern down the rows is the same for every column, so the height pass needs no exchange between lanes: it runs on registers straight from global memory,
// and only the height-reduced strip of a tile goes through LDS for the width pass.  Tap weights are normalised once per
// tile (as ATen does) instead of per output.  4096^2 -> 2048^2, 3 planes, antialiased: 450 MB of HBM traffic for two
// passes through a workspace -> 252 MB.
// History of the schedule (resize_sweep.py (a probe of its round, removed with its knob: git 9ce0718:tools/), 3 x 4096^2 -> 2048^2 | 1024^2 | 6144^2 up-scale, us): two kernels through the
// workspace 89 | 94 | 412; the whole raw window of a tile in LDS, width pass LDS -> LDS, height pass LDS -> output
// 81.5 | 95.8 | 232 -- counters: LDS pipe 65-80 % busy (13.5 cycles per LDS instruction, ~28 bytes per clock: the width pass
// reads dwords `scale` floats apart, a bank conflict for even scales), VALUs 40 %, global loads fully hidden; this form
// with one piece per lane and step 77 | 64 | 181 (LDS pipe 24 % busy, but 83 % of the wave cycles waiting on memory), with
// 2-4 pieces = 8-16 loads in flight per lane 55 | 44 | 164 = 4.6 | 4.8 | 4.0 TB/s.  Tried and measured level or worse:
// persistent workgroups with the next window prefetched through registers, unmasked tap loops for interior tiles, four
// output columns per lane with 16-byte stores (more conflicts: 86 | 72 | 195).
#pragma once
#include <climits>

#include "resize_taps.hpp"

namespace pbr {

constexpr int kTileW = 64;

// A workgroup owns a toh x 64 tile of the output:
//   0. tap tables in LDS: per output column / row of the tile its first tap and its taps' weights, NORMALISED once (ATen
//      normalises the weights, then accumulates sum w_j x_j: _compute_indices_weights_aa) -- the inner loops are pure fma
//      streams, no weight arithmetic, no division;
//   1. height pass: a lane owns a 16-byte piece (4 columns) of one output row, loads that piece of each of the row's K
//      input rows straight from global memory (coalesced along x; an input row serves ~K / scale output rows and is re-read
//      from L2, not from HBM) and accumulates in registers -> strip mid[toh][in_cols] in LDS, one ds_write_b128 per piece;
//   2. width pass mid -> output: a lane keeps its column and its K weights, reads its taps from LDS, stores coalesced.
// Only taps inside a window are ever used (0 x inf must not become NaN).  The sums are formed height-first, ATen's
// width-first: the same products added in another order, a few ulp apart (tests: <= 2e-6 from ATen).
// LDS: wx[K][64] wy[K][toh] | xo[64] xn[64] yo[toh] yn[toh] | mid[toh][pitch] + 16 floats of slack.
//
// StripGeom (the host fills it: strip_launch below).  xcd_chunk, xcd_tiles: the XCD-contiguous order -- tiles per chunk (0 = identity), tiles covered by whole blocks of 8 chunks.
// reserved: a word nobody reads (it held `quads`, which the kernel takes as its template parameter).  It stays for the layout of the kernel's argument
// block: without it the compiler merges the scalar loads of the arguments differently and renumbers the registers of the two forward instantiations
// (5 611 -> 5 610 and 5 746 -> 5 737 instructions; timed level within 0.5 %, which is also what two runs of one binary differ by).
struct StripGeom { int toh, tiles_x, tiles_y, kx, ky, pitch, vec_ok, xcd_chunk, xcd_tiles, reserved; };

template <int K, bool VEC>
__device__ __forceinline__ void height_from_global(const float *__restrict__ sp, float *mid, const float *wy, const int *yo, const int *yn,
                                                   int toh, int oh, int in_cols, int pitch, int w_in, int cols_left, int tid) {
    const int cn = VEC ? (in_cols + 3) >> 2 : in_cols, total = oh * cn;
    const float inv = 1.0f / (float)cn;
    if (VEC) {
        // U pieces per lane and step, their U x K loads all in flight before the first fma: the kernel waits on memory
        // (counters: 83 % of the wave cycles), and every load in flight shortens the phase.
        constexpr int U = K <= 4 ? 4 : (K <= 8 ? 2 : 1);
        for (int e0 = tid; e0 < total; e0 += U * 256) {
            float4 v[U][K];
            int o[U], n[U], at[U];
#pragma unroll
            for (int u = 0; u < U; ++u) {
                const int e = e0 + u * 256;
                const bool live = e < total;
                o[u] = live ? (int)(((float)e + 0.5f) * inv) : 0;          // (e + 0.5) / cn is never within rounding of an integer
                const int c = e - o[u] * cn;
                n[u] = live && 4 * c < cols_left ? yn[o[u]] : 0;              // the window's last piece may start past the row's end
                at[u] = live ? o[u] * pitch + 4 * c : -1;
                const float *q = sp + (int64_t)yo[o[u]] * w_in + 4 * c;
#pragma unroll
                for (int j = 0; j < K; ++j) {
                    v[u][j] = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
                    if (j < n[u]) v[u][j] = *reinterpret_cast<const float4 *>(q + (int64_t)j * w_in);
                }
            }
#pragma unroll
            for (int u = 0; u < U; ++u) {
                float4 acc = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
#pragma unroll
                for (int j = 0; j < K; ++j) {
                    const float w = j < n[u] ? wy[j * toh + o[u]] : 0.0f;
                    acc.x = fmaf(w, v[u][j].x, acc.x); acc.y = fmaf(w, v[u][j].y, acc.y);
                    acc.z = fmaf(w, v[u][j].z, acc.z); acc.w = fmaf(w, v[u][j].w, acc.w);
                }
                if (at[u] >= 0) *reinterpret_cast<float4 *>(mid + at[u]) = acc;
            }
        }
        return;
    }
    for (int e = tid; e < total; e += 256) {
        const int o = (int)(((float)e + 0.5f) * inv), c = e - o * cn;
        const int n = c < cols_left ? yn[o] : 0;
        const float *q = sp + (int64_t)yo[o] * w_in + c;
        float acc = 0.0f;
#pragma unroll
        for (int j = 0; j < K; ++j)
            if (j < n) acc = fmaf(wy[j * toh + o], q[(int64_t)j * w_in], acc);
        mid[o * pitch + c] = acc;
    }
}

template <int K>
__device__ __forceinline__ void width_to_global(const float *mid, float *dp, const float *wx, const int *xo, const int *xn, int pitch,
                                                int oh, int ow, int oy0, int ox0, int w_out, int tid) {
    const int i = tid & (kTileW - 1), off = xo[i], n = xn[i];
    if (i >= ow) return;
    float w[K];
#pragma unroll
    for (int j = 0; j < K; ++j) w[j] = j < n ? wx[j * kTileW + i] : 0.0f;
    for (int r = tid / kTileW; r < oh; r += 2 * (256 / kTileW)) {            // a lane keeps its column; two rows per step for ILP
        const int r2 = r + 256 / kTileW;
        const bool second = r2 < oh;
        const float *q0 = mid + r * pitch + off, *q1 = mid + (second ? r2 : r) * pitch + off;
        float a0 = 0.0f, a1 = 0.0f;
#pragma unroll
        for (int j = 0; j < K; ++j) { a0 = fmaf(w[j], j < n ? q0[j] : 0.0f, a0); a1 = fmaf(w[j], j < n ? q1[j] : 0.0f, a1); }
        dp[(int64_t)(oy0 + r) * w_out + ox0 + i] = a0;
        if (second) dp[(int64_t)(oy0 + r2) * w_out + ox0 + i] = a1;
    }
}

// The same pass with FOUR consecutive columns per lane and 16-byte stores (rows of the result 16-byte aligned, whole quads): the
// launches that write more than they read -- the gradient of a down-scale, 4 output bytes per input byte at 2x -- are bound by
// their stores, and a wave's 4-byte stores fill a 256-byte piece of a row where its 16-byte stores fill four rows of the tile.
// Same taps, same order per column: bit-identical to the one-column form.
template <int K>
__device__ __forceinline__ void width_to_global_quads(const float *mid, float *dp, const float *wx, const int *xo, const int *xn, int pitch,
                                                      int oh, int ow, int oy0, int ox0, int w_out, int tid) {
    constexpr int kLanes = kTileW / 4;                                       // lanes per tile row
    const int i4 = (tid & (kLanes - 1)) * 4;
    if (i4 >= ow) return;
    int off[4], n[4];
    float w[4][K];
#pragma unroll
    for (int c = 0; c < 4; ++c) {
        off[c] = xo[i4 + c]; n[c] = xn[i4 + c];
#pragma unroll
        for (int j = 0; j < K; ++j) w[c][j] = j < n[c] ? wx[j * kTileW + i4 + c] : 0.0f;
    }
    for (int r = tid / kLanes; r < oh; r += 256 / kLanes) {
        const float *q = mid + r * pitch;
        float a[4] = {0.0f, 0.0f, 0.0f, 0.0f};
#pragma unroll
        for (int c = 0; c < 4; ++c)
#pragma unroll
            for (int j = 0; j < K; ++j) a[c] = fmaf(w[c][j], j < n[c] ? q[off[c] + j] : 0.0f, a[c]);
        *reinterpret_cast<float4 *>(dp + (int64_t)(oy0 + r) * w_out + ox0 + i4) = make_float4(a[0], a[1], a[2], a[3]);
    }
}

// TABLES (the gradient, pbr_resize_bilinear_backward): the same two phases with the tap tables TRANSPOSED -- per gradient-input
// index k the first upstream index that reads it, their number and the normalised weights, as resize_backward_tables_kernel
// wrote them to global memory -- instead of derived from the filter: "dst" is the gradient of the resize's input, "src" the
// upstream gradient.  Phase 0 copies the tile's slices of the tables into the same LDS arrays; phases 1 and 2 do not change.
struct StripTables { const int *lo_x, *cnt_x, *lo_y, *cnt_y; const float *w_x, *w_y; int nx, ny, h_src; const float *band; const int *col_base; const float *col_w; };

// WIDE: the instantiation for 17 ... 36 taps per axis (down-scales of 7x ... 17x: (int)(2 s) + 3 taps; round 5) -- its own kernel, so that its registers (36 pieces of a column in
// flight: 190 VGPRs) are not the occupancy of the common one (89).
template <bool TABLES, bool QUADS, bool WIDE = false>
__global__ __launch_bounds__(256) void resize_strip_kernel(const float *__restrict__ src, float *__restrict__ dst, int h_out,
                                                           int w_out, int w_in, StripGeom tg, AxisFilter fw, AxisFilter fh, StripTables tb) {
    extern __shared__ float lds[];
    float *wx = lds, *wy = wx + tg.kx * kTileW;
    int *xo = reinterpret_cast<int *>(wy + tg.ky * tg.toh), *xn = xo + kTileW, *yo = xn + kTileW, *yn = yo + tg.toh;
    float *mid = reinterpret_cast<float *>(yn + tg.toh);            // [toh][pitch] + 16 floats of slack (taps past a window are loaded, never used)
    __shared__ int tap_max[2];
    // Workgroups are dealt to the 8 XCDs round-robin; each XCD has its own L2.  With the identity order the left / right / upper /
    // lower neighbours of a tile -- which share its halo rows and the 128-byte lines its window starts and ends in -- run on
    // OTHER XCDs, and every shared line leaves HBM once per XCD that touches it (PMC: 1.3-1.4 x the algorithmic bytes, 2 x the input
    // when up-scaling).  Here XCD x takes the x-th CHUNK of consecutive tiles out of every block of 8 chunks, so the left / right
    // neighbours (and, with chunks of two tile rows, half of the upper / lower ones) meet in one L2.
    int tile = blockIdx.x;
    if (tg.xcd_chunk > 0 && tile < tg.xcd_tiles) {          // blocks of 8 chunks: XCD x takes chunk x of every block
        const int span = 8 * tg.xcd_chunk, blk = tile / span, r = tile - blk * span;
        tile = blk * span + (r & 7) * tg.xcd_chunk + (r >> 3);
    }
    const int per_plane = tg.tiles_x * tg.tiles_y;
    const int plane = tile / per_plane, t2 = tile - plane * per_plane;
    const int ty = t2 / tg.tiles_x, tx = t2 - ty * tg.tiles_x;
    const int ox0 = tx * kTileW, oy0 = ty * tg.toh;
    const int ow = min(kTileW, w_out - ox0), oh = min(tg.toh, h_out - oy0);
    const int tid = threadIdx.x;
    int xlo = 0, n0, xl = 0, nl = 0; float c0;                       // tap windows are monotone in the output index
    __shared__ int win[2];
    if (TABLES) {
        // the upstream columns the tile reads: first and one-past-last over its columns WITH contributors (without antialiasing a
        // down-scale leaves columns that no output reads: cnt = 0)
        if (tid < kTileW) {
            int lo = INT32_MAX, hi = 0;
            if (tid < ow) {
                const int n = tb.cnt_x[ox0 + tid];
                if (n > 0) { lo = tb.lo_x[ox0 + tid]; hi = lo + n; }
            }
            for (int o = 32; o > 0; o >>= 1) { lo = min(lo, __shfl_xor(lo, o, 64)); hi = max(hi, __shfl_xor(hi, o, 64)); }
            if (tid == 0) { win[0] = lo == INT32_MAX ? 0 : lo; win[1] = lo == INT32_MAX ? 0 : hi; }
        }
    } else {
        tap_window(fw, ox0, xlo, n0, c0);
        tap_window(fw, ox0 + ow - 1, xl, nl, c0);
    }
    // ---- phase 0: tap tables (wave 0: columns; waves 1-3: rows, with their ABSOLUTE first input row) and the largest tap counts
    if (tid < 2) tap_max[tid] = 0;
    __syncthreads();
    if (TABLES) { xlo = win[0]; xl = win[1]; }
    const int xbase = tg.vec_ok ? (xlo & ~3) : xlo;
    const int in_cols = xl + nl - xbase;
    if (tid < kTileW) {
        int xmin = 0, n = 0; float center = 0.0f, wsum = 0.0f;
        if (TABLES) {
            if (tid < ow) { xmin = tb.lo_x[ox0 + tid]; n = min(tb.cnt_x[ox0 + tid], tg.kx); }
            for (int j = 0; j < tg.kx; ++j) wx[j * kTileW + tid] = j < n ? tb.w_x[(size_t)j * tb.nx + ox0 + tid] : 0.0f;
        } else {
            if (tid < ow) {
                tap_window(fw, ox0 + tid, xmin, n, center);
                for (int j = 0; j < n; ++j) wsum += tap_weight(fw, j, xmin, center);
            }
            const float inv = wsum != 0.0f ? 1.0f / wsum : 0.0f;      // (window_norm, written out: through the helper the compiler orders this kernel differently)
            for (int j = 0; j < tg.kx; ++j) wx[j * kTileW + tid] = j < n ? tap_weight(fw, j, xmin, center) * inv : 0.0f;
        }
        xo[tid] = tid < ow && n > 0 ? xmin - xbase : 0;
        xn[tid] = n;
        int m = n;
        for (int o = 32; o > 0; o >>= 1) m = max(m, __shfl_xor(m, o, 64));
        if (tid == 0) atomicMax(&tap_max[0], m);
    } else {
        int m = 0;
        for (int o = tid - kTileW; o < tg.toh; o += 256 - kTileW) {
            int ymin = 0, n = 0; float center = 0.0f, wsum = 0.0f;
            if (TABLES) {
                if (o < oh) { ymin = tb.lo_y[oy0 + o]; n = min(tb.cnt_y[oy0 + o], tg.ky); }
                for (int j = 0; j < tg.ky; ++j) wy[j * tg.toh + o] = j < n ? tb.w_y[(size_t)j * tb.ny + oy0 + o] : 0.0f;
            } else {
                if (o < oh) {
                    tap_window(fh, oy0 + o, ymin, n, center);
                    for (int j = 0; j < n; ++j) wsum += tap_weight(fh, j, ymin, center);
                }
                const float inv = wsum != 0.0f ? 1.0f / wsum : 0.0f;
                for (int j = 0; j < tg.ky; ++j) wy[j * tg.toh + o] = j < n ? tap_weight(fh, j, ymin, center) * inv : 0.0f;
            }
            yo[o] = ymin;
            yn[o] = n;
            m = max(m, n);
        }
        for (int k = 32; k > 0; k >>= 1) m = max(m, __shfl_xor(m, k, 64));
        if ((tid & 63) == 0) atomicMax(&tap_max[1], m);
    }
    __syncthreads();
    const int kx = tap_max[0], ky = tap_max[1];
    // ---- phase 1: height pass, global -> mid
    const float *sp = src + (int64_t)plane * (TABLES ? tb.h_src : fh.n_in) * w_in + xbase;
    const int cols_left = w_in - xbase;
#define PBR_HEIGHT(KK) (tg.vec_ok ? height_from_global<KK, true>(sp, mid, wy, yo, yn, tg.toh, oh, in_cols, tg.pitch, w_in, cols_left, tid) \
                                  : height_from_global<KK, false>(sp, mid, wy, yo, yn, tg.toh, oh, in_cols, tg.pitch, w_in, cols_left, tid))
    if (WIDE) {
        if (ky <= 24) PBR_HEIGHT(24);
        else PBR_HEIGHT(36);
    } else if (ky <= 4) PBR_HEIGHT(4);
    else if (ky <= 6) PBR_HEIGHT(6);
    else if (ky <= 8) PBR_HEIGHT(8);
    else if (ky <= 12) PBR_HEIGHT(12);
    else PBR_HEIGHT(16);
#undef PBR_HEIGHT
    __syncthreads();
    // ---- phase 2: width pass, mid -> output
    float *dp = dst + (int64_t)plane * h_out * w_out;
    const bool quads = QUADS && (ow & 3) == 0;
#define PBR_WIDTH(KK) (quads ? width_to_global_quads<KK>(mid, dp, wx, xo, xn, tg.pitch, oh, ow, oy0, ox0, w_out, tid) \
                             : width_to_global<KK>(mid, dp, wx, xo, xn, tg.pitch, oh, ow, oy0, ox0, w_out, tid))
    if (WIDE) {
        if (kx <= 24) width_to_global<24>(mid, dp, wx, xo, xn, tg.pitch, oh, ow, oy0, ox0, w_out, tid);
        else width_to_global<36>(mid, dp, wx, xo, xn, tg.pitch, oh, ow, oy0, ox0, w_out, tid);
    } else if (kx <= 4) PBR_WIDTH(4);
    else if (kx <= 6) PBR_WIDTH(6);
    else if (kx <= 8) PBR_WIDTH(8);
    else if (kx <= 12) PBR_WIDTH(12);
    else width_to_global<16>(mid, dp, wx, xo, xn, tg.pitch, oh, ow, oy0, ox0, w_out, tid);
#undef PBR_WIDTH
}

// Host side, for either direction: the launch of a strip kernel over planes x h_dst x w_dst results with kx | ky taps per axis and
// tiles that read at most cols_max source columns.  Rows per tile: the most of 128 ... 16 that keep the workgroup's LDS within
// `budget` (the callers have the measurements behind theirs), else 8; `slack` words behind the strip (a window's taps are read up to
// the template's K, never used).  False when the launch does not fit 64 KiB of LDS or a 32-bit grid.
struct StripLaunch { StripGeom tg; size_t lds; unsigned tiles; };
inline bool strip_launch(StripLaunch &l, int64_t planes, int h_dst, int w_dst, int kx, int ky, int cols_max, bool vec_ok, int slack, size_t budget) {
    const int pitch = ((cols_max + 3) & ~3) + 4;                                              // + 4 floats: rows land on different banks
    auto lds_for = [&](int rows) {
        return sizeof(float) * ((size_t)kx * kTileW + (size_t)ky * rows + 2 * (kTileW + rows) + (size_t)rows * pitch + slack);
    };
    int toh = 8;
    for (int rows : {128, 64, 32, 16})
        if (lds_for(rows) <= budget) { toh = rows; break; }
    const int64_t tx = (w_dst + kTileW - 1) / kTileW, ty = (h_dst + toh - 1) / toh, n_tiles = planes * tx * ty;
    if (lds_for(toh) > 64 * 1024 || n_tiles > INT32_MAX) return false;
    // XCD-contiguous order (resize_strip_kernel) in chunks of 64 tiles.  Identity order -> chunks of 64, 3 x 4096^2 (us):
    // -> 2048^2 55.1 -> 48.0, -> 1024^2 44.4 -> 36.8, -> 1365^2 46.3 -> 41.0, -> 3000^2 74.7 -> 72.7, -> 5000^2 127.6 -> 114.3,
    // -> 6144^2 163.5 -> 158.1, -> 8192^2 269.1 -> 271.5; HBM reads 301.5 -> 201.7 MB for the 2x down-scale (the input is
    // 201.3 MB), 399.7 -> 201.7 MB for the 1.5x up-scale.  One chunk per XCD (an eighth of all tiles each) is as good for
    // down-scales but 4 % slower for large up-scales (eight write fronts far apart); 32 ... 1024 tiles are within 2 %.
    int64_t chunk = 64;
    if (chunk > n_tiles / 8) chunk = n_tiles / 8;
    l.tg = {toh, (int)tx, (int)ty, kx, ky, pitch, vec_ok ? 1 : 0, (int)chunk, (int)(chunk ? (n_tiles / (8 * chunk)) * 8 * chunk : 0), 0};
    l.lds = lds_for(toh);
    l.tiles = (unsigned)n_tiles;
    return true;
}

}  // namespace pbr
