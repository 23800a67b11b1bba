// resize_backward.hip -- gradient of the bilinear resize (the forward: resize.hip; the tap rule: resize_taps.hpp).
//
// The kernel families, in the order pbr_resize_bilinear_backward tries them: the band walk of resize_down.hpp with the transposed two-tap
// weights (whole power-of-two up-scales), the two-tap transpose (other up-scales), the register gather over transposed tap tables, the
// strip kernel of resize_strip.hpp with those tables, and the two generic passes through the workspace.  The two register kernels stand in
// the lane frame of resize_lane.hpp; here: where their column and row weights come from, and the host's window scan (worst_span).
#include <hip/hip_runtime.h>

#include <cstdint>

#include "../../include/pbr_hip.h"
#include "resize_down.hpp"
#include "resize_lane.hpp"
#include "resize_strip.hpp"
#include "resize_taps.hpp"
#include "stream_shape.hpp"
#include "tuning.hpp"

namespace pbr {

// ---- the generic passes (what autograd derives from F.interpolate(mode="bilinear", antialias=...)) -------------------------
// The forward is out = Wy in Wx^T with the banded tap matrices of the rule; the gradient is g_in = Wy^T g_out Wx.  Two passes through a
// workspace, each a GATHER by input index (no atomics, fixed summation order): tap windows are monotone in the output index, so the
// outputs whose window holds input k are a contiguous range; it is bracketed from the window geometry and every candidate's exact
// window is re-derived with the forward's own arithmetic (tap_window / tap_weight), the per-output normalisation 1 / sum_j w_j
// coming from a small table computed first.
__global__ __launch_bounds__(256) void resize_norm_kernel(float *__restrict__ inv, int n_out, AxisFilter f) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n_out) return;
    int xmin, n; float center;
    inv[i] = window_norm(f, i, xmin, n, center);
}

// first / last output index whose window can hold input k: |k + 0.5 - scale (i + 0.5)| <= support + 1, one more on each side
__device__ __forceinline__ void candidates(const AxisFilter &f, int k, int n_out, int &lo, int &hi) {
    const float inv = 1.0f / f.scale;
    lo = max(0, (int)floorf(((float)k - f.support - 1.0f) * inv - 0.5f) - 1);
    hi = min(n_out - 1, (int)ceilf(((float)k + f.support + 2.0f) * inv - 0.5f) + 1);
}

// pass A: tmp[plane][k][x] = sum_i Wy[i][k] g_out[plane][i][x]      (k over input rows, x over OUTPUT columns)
__global__ __launch_bounds__(256) void resize_backward_rows_kernel(const float *__restrict__ gout, float *__restrict__ tmp, const float *__restrict__ inv,
                                                                   int64_t planes, int n_out, int width, AxisFilter f) {
    const int64_t total = planes * f.n_in * width, stride = (int64_t)gridDim.x * blockDim.x;
    for (int64_t idx = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; idx < total; idx += stride) {
        const int x = (int)(idx % width);
        const int64_t t = idx / width;
        const int k = (int)(t % f.n_in);
        const int64_t plane = t / f.n_in;
        int lo, hi;
        candidates(f, k, n_out, lo, hi);
        const float *g = gout + plane * n_out * width + x;
        float acc = 0.0f;
        for (int i = lo; i <= hi; ++i) {
            int ymin, n; float center;
            tap_window(f, i, ymin, n, center);
            if (k >= ymin && k < ymin + n) acc = fmaf(tap_weight(f, k - ymin, ymin, center) * inv[i], g[(int64_t)i * width], acc);
        }
        tmp[idx] = acc;
    }
}

// pass B: g_in[row][k] = sum_i Wx[i][k] tmp[row][i]                 (rows = planes * h_in, k over input columns)
__global__ __launch_bounds__(256) void resize_backward_cols_kernel(const float *__restrict__ tmp, float *__restrict__ gin, const float *__restrict__ inv,
                                                                   int64_t rows, int n_out, AxisFilter f) {
    const int64_t total = rows * f.n_in, stride = (int64_t)gridDim.x * blockDim.x;
    for (int64_t idx = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; idx < total; idx += stride) {
        const int64_t row = idx / f.n_in;
        const int k = (int)(idx - row * f.n_in);
        int lo, hi;
        candidates(f, k, n_out, lo, hi);
        const float *g = tmp + row * n_out;
        float acc = 0.0f;
        for (int i = lo; i <= hi; ++i) {
            int xmin, n; float center;
            tap_window(f, i, xmin, n, center);
            if (k >= xmin && k < xmin + n) acc = fmaf(tap_weight(f, k - xmin, xmin, center) * inv[i], g[i], acc);
        }
        gin[idx] = acc;
    }
}

// ---- transposed tap tables (after the counters: the generic kernels above re-derive every candidate's
// window per element and are VALU-bound -- 132 + 221 us for a 2048^2 -> 4096^2 gradient, VALUs saturated, 0.15 of HBM).
// A small kernel writes, per INPUT index k of an axis, the first contributing output `lo[k]`, their number `cnt[k]` and the
// normalised weights w[j][k] (j-major: lanes that walk k read them coalesced); the kernels that read them are then pure fma streams.
// More than kBwdMaxTaps contributors per input (up-scales from ~3x on) keep the generic kernels: the launcher decides from the
// scale (contributors <= (2 support + 2) / scale + 2).
constexpr int kBwdMaxTaps = 12;
__device__ __forceinline__ void backward_table_entry(int *__restrict__ lo_out, int *__restrict__ cnt_out, float *__restrict__ w, int n_out,
                                                     const AxisFilter &f, int k) {
    if (k >= f.n_in) return;
    int lo, hi, first = -1, n = 0;
    candidates(f, k, n_out, lo, hi);
    for (int i = lo; i <= hi; ++i) {
        int xmin, sz; float center;
        tap_window(f, i, xmin, sz, center);
        if (k < xmin || k >= xmin + sz) continue;
        if (first < 0) first = i;
        const int j = i - first;                            // contributors are contiguous (windows are monotone in i)
        float wsum = 0.0f;                                  // the output's normalisation, as resize_norm_kernel forms it (window_norm behind the window's test)
        for (int q = 0; q < sz; ++q) wsum += tap_weight(f, q, xmin, center);
        if (j < kBwdMaxTaps) w[(size_t)j * f.n_in + k] = tap_weight(f, k - xmin, xmin, center) * (wsum != 0.0f ? 1.0f / wsum : 0.0f);
        n = j + 1;
    }
    n = min(n, kBwdMaxTaps);                                // (the launcher only comes here when the bound on n fits)
    for (int j = n; j < kBwdMaxTaps; ++j) w[(size_t)j * f.n_in + k] = 0.0f;
    lo_out[k] = first < 0 ? 0 : first;
    cnt_out[k] = n;
}

// both axes in one launch: workgroups [0, groups_y) write the row tables, the others the column tables
// `band` != nullptr: besides, per BAND of kBandRows consecutive gradient rows (what one wave of resize_backward_gather_kernel owns), the
// rows' weights as a dense matrix over the band's union of upstream rows -- record of kBandWords words: [0] first upstream row,
// [1] number of upstream rows (<= kBandMaxRows), [8 + 8 j + r] weight of upstream row first + j in gradient row r -- so that the
// gather kernel reads eight wave-uniform weights with one scalar load instead of looking each up through lo / cnt (the look-ups made
// it scalar-bound: 953 scalar against 752 vector instructions per wave).  A lane reads back only the entries of its own row k; the
// band's first / last upstream row come from its eight lanes by shuffles.
constexpr int kBandRows = 8, kBandMaxRows = 16, kBandWords = 8 + kBandRows * kBandMaxRows;
__global__ __launch_bounds__(256) void resize_backward_tables_kernel(int *__restrict__ lo_y, int *__restrict__ cnt_y, float *__restrict__ wy, int h_out,
                                                                     AxisFilter fh, int *__restrict__ lo_x, int *__restrict__ cnt_x,
                                                                     float *__restrict__ wx, int w_out, AxisFilter fw, int groups_y,
                                                                     float *__restrict__ band, int *__restrict__ col_base, float *__restrict__ col_w,
                                                                     int col_window) {
    if ((int)blockIdx.x >= groups_y) {
        // ... and per GROUP of four consecutive gradient columns (what one lane of the gather kernel owns): the first upstream column of
        // the group's window, col_base[group], and the 4 x col_window matrix of column weights over that window, col_w[(c W + j) groups +
        // group] -- group-minor, so that the gather kernel's lanes read each entry coalesced, with no look-up through lo / cnt in between.
        const int k = (blockIdx.x - groups_y) * 256 + threadIdx.x;
        backward_table_entry(lo_x, cnt_x, wx, w_out, fw, k);
        if (col_w == nullptr) return;
        const bool live = k < fw.n_in;
        const int first = live ? lo_x[k] : 0, n = live ? cnt_x[k] : 0;
        int lo = n > 0 ? first : INT32_MAX;
        lo = min(lo, __shfl_xor(lo, 1, 64)); lo = min(lo, __shfl_xor(lo, 2, 64));
        if (lo == INT32_MAX) lo = 0;
        const int base = lo < w_out - col_window ? lo : w_out - col_window, group = k >> 2, c = k & 3, groups = (fw.n_in + 3) >> 2;
        if (group >= groups) return;
        if (c == 0) col_base[group] = base;
        for (int j = 0; j < col_window; ++j) {
            const int d = base + j - first;
            col_w[(size_t)(c * col_window + j) * groups + group] = d >= 0 && d < n ? wx[(size_t)d * fw.n_in + k] : 0.0f;
        }
        return;
    }
    const int k = blockIdx.x * 256 + threadIdx.x;
    backward_table_entry(lo_y, cnt_y, wy, h_out, fh, k);
    if (band == nullptr) return;
    const bool live = k < fh.n_in;
    const int first = live ? lo_y[k] : 0, n = live ? cnt_y[k] : 0;
    int lo = n > 0 ? first : INT32_MAX, hi = n > 0 ? first + n : 0;
    for (int o = 1; o < kBandRows; o <<= 1) { lo = min(lo, __shfl_xor(lo, o, 64)); hi = max(hi, __shfl_xor(hi, o, 64)); }
    if (lo == INT32_MAX) lo = 0;
    const int rows = min(max(hi - lo, 0), kBandMaxRows);
    if (k - (int)(threadIdx.x & (kBandRows - 1)) >= fh.n_in) return;        // a band past the last row
    float *rec = band + (size_t)(k / kBandRows) * kBandWords;
    const int r = threadIdx.x & (kBandRows - 1);
    if (r == 0) { reinterpret_cast<int *>(rec)[0] = lo; reinterpret_cast<int *>(rec)[1] = rows; }
    for (int j = 0; j < kBandMaxRows; ++j) {
        const int d = lo + j - first;
        rec[8 + kBandRows * j + r] = d >= 0 && d < n ? wy[(size_t)d * fh.n_in + k] : 0.0f;
    }
}
// ---- gradient of an up-scale: the transpose of resize_up2_kernel, registers only -------------------------------------------------
// out[y][x] = sum over two rows and two columns of wy wx in[..]; the gradient g_in[ky][kx] gathers g_out over the outputs whose
// two-tap windows hold (ky, kx).  Windows start at first_tap(i), which is monotone in i, so the outputs that touch gradient columns
// k0 .. k0 + 3 are the contiguous range first_tap(i) in [k0 - 1, k0 + 3]: at most 5 / scale + 1 of them.  A lane (resize_lane.hpp) finds
// the start of its range once (first_reaching), builds the 4 x W matrix of column weights in registers (W = 8 | 12 | 16 upstream columns;
// zero where an output does not touch a column), then gathers the upstream rows that touch its R gradient rows with their (wave-uniform)
// weights.  No tables, no LDS, no barriers -- the strip kernel with transposed tables (resize_strip_kernel<true>) spends most of its time
// in per-tile set-up and between its barriers on these shapes (0.52 of HBM).  A gather by gradient element with a fixed summation order:
// deterministic, no atomics.  The launcher checks on the host (the same float arithmetic) that W holds for every lane; other shapes keep
// the table-driven passes.
template <int W, int R>
__global__ __launch_bounds__(64) void resize_up2_backward_kernel(const float *__restrict__ gout, float *__restrict__ gin, int h_in, int w_in, int h_out,
                                                                 int w_out, int groups_x, int groups_y, uint32_t xcd_groups, AxisFilter fw, AxisFilter fh) {
    const LanePos p = lane_position<R>(groups_x, groups_y, xcd_groups);      // as the forward
    const int k0 = p.k0, r0 = p.r0;
    if (k0 >= w_in) return;
    // ---- columns: from the first output whose window reaches column k0 - 1 or beyond
    const int i_lo = first_reaching(fw, k0, w_out);
    const int i_base = i_lo < w_out - W ? i_lo : w_out - W;            // W upstream columns from here, inside the row (w_out >= W: the launcher)
    float wx[4][W];
#pragma unroll
    for (int j = 0; j < W; ++j) {
        int first; float wa, wb;
        two_taps(fw, i_base + j, first, wa, wb);
#pragma unroll
        for (int c = 0; c < 4; ++c) wx[c][j] = (first == k0 + c ? wa : 0.0f) + (first + 1 == k0 + c ? wb : 0.0f);
    }
    // ---- rows: the upstream rows whose windows reach gradient rows r0 .. r0 + R - 1 (wave-uniform)
    float acc[R][4];
    for (auto &row : acc) for (float &a : row) a = 0.0f;
    const float *gp = gout + (int64_t)p.plane * h_out * w_out + i_base;
    for (int y = first_reaching(fh, r0, h_out); y < h_out; ++y) {
        int yf; float wy0, wy1;
        two_taps(fh, y, yf, wy0, wy1);
        if (yf > r0 + R - 1) break;
        const int y1 = min(yf + 1, h_in - 1);               // the forward's second row (weight 0 when the window holds one tap)
        gather_row<W, R>(gp + (int64_t)y * w_out, wx, acc, [&](int r) { return (yf == r0 + r ? wy0 : 0.0f) + (y1 == r0 + r ? wy1 : 0.0f); });
    }
    store_rows<R>(gin, p, h_in, w_in, acc);
}

// Host side of the register kernels: the most outputs any `step` consecutive gradient indices (from a multiple of `step` on) gather from --
// the kernel's W (or a band's rows) must cover it.  Those of the indices from k0 on are [lo, hi): neither before(i, k0) nor past(i, k0),
// both ends monotone in k0.  The predicates use the kernels' own first_tap / tap_window: host and device agree bit for bit.
template <typename Before, typename Past>
static int worst_span(const AxisFilter &f, int n_out, int step, Before before, Past past) {
    int worst = 0, lo = 0, hi = 0;
    for (int k0 = 0; k0 < f.n_in; k0 += step) {
        while (lo < n_out && before(lo, k0)) ++lo;
        if (hi < lo) hi = lo;
        while (hi < n_out && !past(hi, k0)) ++hi;
        worst = hi - lo > worst ? hi - lo : worst;
    }
    return worst;
}
// resize_up2_backward_kernel: the outputs whose two-tap windows start in [k0 - 1, k0 + 3], over all lanes' k0
static int up2_backward_window(const AxisFilter &f, int n_out) {
    return worst_span(f, n_out, 4, [&](int i, int k0) { return first_tap(f, i) < k0 - 1; }, [&](int i, int k0) { return first_tap(f, i) > k0 + 3; });
}
// resize_backward_gather_kernel: the outputs whose window [xmin, xmin + size) meets [k0, k0 + rows - 1]; rows = 4: a lane's columns, kBandRows: a wave's rows
static int band_window(const AxisFilter &f, int n_out, int rows) {
    auto before = [&](int i, int k0) { int xmin, n; float c; tap_window(f, i, xmin, n, c); return xmin + n <= k0; };
    return worst_span(f, n_out, rows, before, [&](int i, int k0) { return first_tap(f, i) > k0 + rows - 1; });
}

// ---- gradient of a down-scale, registers only: the two table-driven passes in one kernel without the LDS strip -------------------
// With the transposed tap tables in global memory (resize_backward_tables_kernel: per gradient index k the first upstream index
// lo[k] that read it, their number cnt[k] and the normalised weights w[j][k]) the gradient is a gather with short, contiguous ranges
// on both axes.  A lane's four columns' upstream ranges overlap and are monotone, so their union is W <= 16 consecutive upstream columns:
// the lane builds the 4 x W matrix of column weights once (4 W table reads, coalesced over the lanes), then gathers the union of its rows'
// upstream rows, per gradient row one wave-uniform weight (scalar loads).  resize_strip_kernel<true> does the same work through a tile of
// LDS with three barrier-separated phases and reaches 0.52 of HBM on 4096^2 <- 2048^2; this form has no set-up to amortise.
// Gather by gradient element, fixed order: deterministic.  The launcher checks W on the host (same float arithmetic).
template <int W, int R, bool BAND>
__global__ __launch_bounds__(64) void resize_backward_gather_kernel(const float *__restrict__ gout, float *__restrict__ gin, int h_in, int w_in, int h_out,
                                                                    int w_out, int groups_x, int groups_y, uint32_t xcd_groups, StripTables tb) {
    const LanePos p = lane_position<R>(groups_x, groups_y, xcd_groups);
    const int k0 = p.k0, r0 = p.r0;
    if (k0 >= w_in) return;
    // ---- columns
    float wx[4][W];
    int i_base;
    if (BAND) {                                 // the group's record (resize_backward_tables_kernel): 1 + 4 W coalesced loads, none waits for another
        const int group = k0 >> 2, groups = (w_in + 3) >> 2;
        i_base = tb.col_base[group];
#pragma unroll
        for (int c = 0; c < 4; ++c)
#pragma unroll
            for (int j = 0; j < W; ++j) wx[c][j] = tb.col_w[(size_t)(c * W + j) * groups + group];
    } else {
        int lo[4], n[4], i_lo = INT32_MAX;
#pragma unroll
        for (int c = 0; c < 4; ++c) {
            const int k = min(k0 + c, w_in - 1);
            lo[c] = tb.lo_x[k]; n[c] = k0 + c < w_in ? min(tb.cnt_x[k], kBwdMaxTaps) : 0;
            if (n[c] > 0) i_lo = min(i_lo, lo[c]);
        }
        if (i_lo == INT32_MAX) i_lo = 0;
        i_base = i_lo < w_out - W ? i_lo : w_out - W;
#pragma unroll
        for (int c = 0; c < 4; ++c) {
            const int k = min(k0 + c, w_in - 1);
#pragma unroll
            for (int j = 0; j < W; ++j) {
                const int d = i_base + j - lo[c];
                wx[c][j] = d >= 0 && d < n[c] ? tb.w_x[(size_t)d * tb.nx + k] : 0.0f;
            }
        }
    }
    // ---- rows (wave-uniform: scalar loads)
    float acc[R][4];
    for (auto &row : acc) for (float &a : row) a = 0.0f;
    const float *gp = gout + (int64_t)p.plane * h_out * w_out + i_base;
    if (BAND) {
        // the band's record (resize_backward_tables_kernel): first upstream row, their number, eight weights per upstream row
        static_assert(!BAND || R == kBandRows, "a band is what one wave owns");
        const float *rec = tb.band + (size_t)(r0 / R) * kBandWords;
        const int y_lo = reinterpret_cast<const int *>(rec)[0], y_n = reinterpret_cast<const int *>(rec)[1];
        for (int j = 0; j < y_n; ++j) gather_row<W, R>(gp + (int64_t)(y_lo + j) * w_out, wx, acc, [&](int r) { return rec[8 + kBandRows * j + r]; });
    } else {
        int ylo[R], yn[R], y_lo = INT32_MAX, y_hi = 0;
#pragma unroll
        for (int r = 0; r < R; ++r) {
            const int k = min(r0 + r, h_in - 1);
            ylo[r] = tb.lo_y[k]; yn[r] = r0 + r < h_in ? min(tb.cnt_y[k], kBwdMaxTaps) : 0;
            if (yn[r] > 0) { y_lo = min(y_lo, ylo[r]); y_hi = max(y_hi, ylo[r] + yn[r]); }
        }
        for (int y = y_lo; y < y_hi; ++y)
            gather_row<W, R>(gp + (int64_t)y * w_out, wx, acc, [&](int r) {
                const int d = y - ylo[r];
                return d >= 0 && d < yn[r] ? tb.w_y[(size_t)d * tb.ny + min(r0 + r, h_in - 1)] : 0.0f;
            });
    }
    store_rows<R>(gin, p, h_in, w_in, acc);
}

// The TRANSPOSE of an up-scale by the whole factor S has the same shape: gradient element k gathers the 2 S upstream elements S k - S/2 ... S k + 3 S/2 - 1
// (the outputs whose two-tap windows hold input k), with one weight vector for every interior k and clipped ones for the first and the last --
// resize_down_kernel with other numbers in its three vectors.  Weights from the forward's own two-tap rule (two_taps, with its division on the host).
static DownTaps up_transpose_taps(int S) {
    const AxisFilter f = make_filter(16, 16 * S, false);     // 16 gradient elements, 16 S upstream; up-scales: antialiasing changes nothing
    return make_down_taps([&](int k, float *w) {
        for (int j = 0; j < 2 * S; ++j) {
            const int i = S * k - S / 2 + j;
            if (i < 0 || i >= 16 * S) continue;
            int first, n; float center;
            tap_window(f, i, first, n, center);
            const float a = tap_weight(f, 0, first, center), b = n > 1 ? tap_weight(f, 1, first, center) : 0.0f, inv = 1.0f / (a + b);
            w[j] = (first == k ? a * inv : 0.0f) + (first + 1 == k ? b * inv : 0.0f);
        }
    });
}

// ---- the forms, in the order pbr_resize_bilinear_backward tries them: each decides on the host and launches, or returns false -------------
// One call: its arguments and its workspace (carve_workspace)
struct BackwardCall {
    const float *g; float *gi; int64_t planes; int h_in, w_in, h_out, w_out; AxisFilter fw, fh; hipStream_t s;
    float *tmp, *inv_y, *inv_x, *wy, *wx; int *lo_y, *cnt_y, *lo_x, *cnt_x;
};
// The workspace's layout, in 4-byte words from `base`: tmp [planes][h_in][w_out] | inv_y [h_out] | inv_x [w_out] | wy [kBwdMaxTaps][h_in] |
// wx [kBwdMaxTaps][w_in] | then ints: lo_y, cnt_y [h_in] | lo_x, cnt_x [w_in] | 4 words of slack.  Sets the call's pointers (`base` = NULL: none,
// the size query) and returns the words of the whole.
static size_t carve_workspace(BackwardCall &c, float *base) {
    size_t at = 0;
    auto take = [&](auto *&p, size_t words) { p = base ? reinterpret_cast<std::remove_reference_t<decltype(p)>>(base + at) : nullptr; at += words; };
    take(c.tmp, (size_t)c.planes * (size_t)c.h_in * (size_t)c.w_out); take(c.inv_y, (size_t)c.h_out); take(c.inv_x, (size_t)c.w_out);
    take(c.wy, (size_t)kBwdMaxTaps * (size_t)c.h_in); take(c.wx, (size_t)kBwdMaxTaps * (size_t)c.w_in);
    take(c.lo_y, (size_t)c.h_in); take(c.cnt_y, (size_t)c.h_in); take(c.lo_x, (size_t)c.w_in); take(c.cnt_x, (size_t)c.w_in);
    return at + 4;
}
static StripTables tables_of(const BackwardCall &c, const float *band = nullptr, const int *col_base = nullptr, const float *col_w = nullptr) {      // (the gather kernel's records: optional)
    return {c.lo_x, c.cnt_x, c.lo_y, c.cnt_y, c.wx, c.wy, c.w_in, c.h_in, c.h_out, band, col_base, col_w};
}

// Gradient of an up-scale by 2 | 4 | 8 | 16: the band walk of resize_down.hpp over the upstream gradient, with the transposed two-tap weights.  (Powers of two only:
// the forward's scale 1 / S is then exact and its two weights are the same for every S-th output; with 1/3, 1/5 ... the forward's fp32 tap positions drift
// by ~6e-8 of the index, and the exact transpose of THAT is what the two-tap transpose below forms.)
// 3 x 4096^2 upstream -> 2048^2: see DESIGN.md section 3 (the two-tap transpose below: 44.4 us, 1.17 x the bytes -- its lanes' windows overlap past L2)
static bool backward_band_walk(const BackwardCall &c) {
    const int up = c.h_out % c.h_in == 0 && c.w_out % c.w_in == 0 && c.h_out / c.h_in == c.w_out / c.w_in ? c.h_out / c.h_in : 0;
    return (up == 2 || up == 4 || up == 8 || up == 16) && launch_down(c.g, c.gi, c.planes, c.h_in, c.w_in, up, up_transpose_taps(up), c.s);
}

// Gradient of an up-scale (up to 3x across, 4x down the rows): the register-only transpose of the two-tap forward (resize_bwd_probe.py).
// W from the exact window count of THIS shape; rows per lane 4.
static bool backward_two_tap(const BackwardCall &c) {
    if (c.fw.scale > 1.0f || c.fh.scale > 1.0f || c.fw.scale < 0.34f || c.fh.scale < 0.25f || c.w_out < 16) return false;
    const int need = up2_backward_window(c.fw, c.w_out);
    constexpr int R = 4;
    const LaneGrid grid = lane_grid(c.w_in, c.h_in, R, c.planes);
    if (need > 16 || !grid.fits) return false;
    with_window(need, [&](auto w) {
        launch_lanes(resize_up2_backward_kernel<decltype(w)::value, R>, grid, c.s, c.g, c.gi, c.h_in, c.w_in, c.h_out, c.w_out, c.fw, c.fh);
    });
    return true;
}

// the transposed tables hold every contributor of an input index (contributors <= (2 support + 2) / scale + 2)
static bool tables_fit(const AxisFilter &f) { return (int)((2.0f * f.support + 2.0f) / f.scale) + 2 <= kBwdMaxTaps; }
static void launch_tables(const BackwardCall &c, float *band, int *col_base, float *col_w, int window) {
    const int groups_y = (c.h_in + 255) / 256, groups_x = (c.w_in + 255) / 256;
    hipLaunchKernelGGL(resize_backward_tables_kernel, dim3(groups_y + groups_x), dim3(256), 0, c.s, c.lo_y, c.cnt_y, c.wy, c.h_out, c.fh, c.lo_x, c.cnt_x, c.wx,
                       c.w_out, c.fw, groups_y, band, col_base, col_w, window);
}

// Register-only gather over the tables (resize_backward_gather_kernel): 4 gradient columns x 8 rows per lane; the rows' weights from the
// per-band matrices the tables kernel leaves in the (otherwise unused) pass-to-pass area of the workspace when they fit there (else the kernel looks the rows up).
static bool backward_gather(const BackwardCall &c) {
    if (!tables_fit(c.fw) || !tables_fit(c.fh) || c.w_out < 16) return false;
    const int need = band_window(c.fw, c.w_out, 4);
    constexpr int R = 8;                                          // gradient rows per lane
    const LaneGrid grid = lane_grid(c.w_in, c.h_in, R, c.planes);
    if (need > 16 || !grid.fits) return false;
    with_window(need, [&](auto w) {
        constexpr int W = decltype(w)::value;                     // the gather kernel's W
        const size_t band_words = (size_t)((c.h_in + kBandRows - 1) / kBandRows) * kBandWords, col_groups = (size_t)(c.w_in + 3) / 4;
        const bool banded = R == kBandRows && band_window(c.fh, c.h_out, kBandRows) <= kBandMaxRows &&
                            band_words + col_groups * (1 + 4 * (size_t)W) <= (size_t)c.planes * c.h_in * c.w_out;
        float *band = banded ? c.tmp : nullptr, *col_w = banded ? c.tmp + band_words + col_groups : nullptr;
        int *col_base = banded ? reinterpret_cast<int *>(c.tmp + band_words) : nullptr;
        launch_tables(c, band, col_base, col_w, W);
        auto fn = banded ? resize_backward_gather_kernel<W, R, true> : resize_backward_gather_kernel<W, R, false>;
        launch_lanes(fn, grid, c.s, c.g, c.gi, c.h_in, c.w_in, c.h_out, c.w_out, tables_of(c, band, col_base, col_w));
    });
    return true;
}

// One pass: the strip kernel with the transposed tables (resize_strip_kernel<true>): a toh x 64 tile of the gradient, the
// rows pass from global memory into the LDS strip, the columns pass out of it.  3 x 2048^2 gradient -> 4096^2: see DESIGN.md 3.8.
static bool backward_strip(const BackwardCall &c) {
    if (!tables_fit(c.fw) || !tables_fit(c.fh)) return false;
    const int kx = (int)((2.0f * c.fw.support + 2.0f) / c.fw.scale) + 2, ky = (int)((2.0f * c.fh.support + 2.0f) / c.fh.scale) + 2;     // <= kBwdMaxTaps
    const int cols_max = (int)((float)(kTileW - 1 + 2.0f * c.fw.support) / c.fw.scale) + 8;     // upstream columns a tile of 64 reads, + alignment
    // Rows per tile: here more rows win up to ~48 KiB of LDS (resize_bwd_probe.py, us at 32 / 64 / 128 rows: 2048^2 -> 4096^2
    // 123 / 79 / 67, 3000^2 -> 4096^2 138 / 98 / 84, 6144^2 -> 4096^2 184 / 150 / -, 4096^2 -> 2048^2 59 / 60 / 115): the strip's
    // halo rows are re-read per tile, and a gradient tile reads few bytes for what it writes.
    // A refusal falls here, before the tables are written, and leaves the call to the generic passes -- no form stands in between, because next to nothing
    // is refused.  LDS never: tables_fit gives kx, ky <= 12 and (2 support + 2) / scale < 11, hence 1 / scale < 2.75 (support >= 1), cols_max < 61 x 2.75 +
    // 11 + 8 = 187, pitch <= 192, and 8 rows are 10 KiB.  The 32-bit grid only with more tiles than the planes x h_in <= 2^31 rows the entry point lets
    // in, i.e. tiles one row high, two or more to a row: at least 2^30 planes of one row and 65 columns, a gradient of 279 GB.
    StripLaunch l;
    if (!strip_launch(l, c.planes, c.h_in, c.w_in, kx, ky, cols_max, c.w_out % 4 == 0 && is_aligned(c.g, 16), 16, 48 * 1024)) return false;
    launch_tables(c, nullptr, nullptr, nullptr, 0);
    // 16-byte stores where the gradient is at least twice its upstream (2048^2 -> 4096^2: 66.7 against 69.3 us; the other way,
    // 4096^2 -> 2048^2, 70.6 against 59.4: a quarter of the lanes then walk the LDS strip)
    const bool quads = (int64_t)c.h_in * c.w_in >= 2 * (int64_t)c.h_out * c.w_out && c.w_in % 4 == 0 && is_aligned(c.gi, 16);
    auto strip = quads ? resize_strip_kernel<true, true> : resize_strip_kernel<true, false>;
    hipLaunchKernelGGL(strip, dim3(l.tiles), dim3(256), l.lds, c.s, c.g, c.gi, c.h_in, c.w_in, c.w_out, l.tg, c.fw, c.fh, tables_of(c));
    return true;
}

// many contributors per input (up-scales from ~3x on), or a shape no other form takes: the generic passes, any size
static void backward_generic(const BackwardCall &c) {
    hipLaunchKernelGGL(resize_norm_kernel, dim3((c.h_out + 255) / 256), dim3(256), 0, c.s, c.inv_y, c.h_out, c.fh);
    hipLaunchKernelGGL(resize_norm_kernel, dim3((c.w_out + 255) / 256), dim3(256), 0, c.s, c.inv_x, c.w_out, c.fw);
    hipLaunchKernelGGL(resize_backward_rows_kernel, dim3(stream_grid(c.planes * c.h_in * c.w_out, 16)), dim3(256), 0, c.s, c.g, c.tmp, c.inv_y, c.planes, c.h_out, c.w_out, c.fh);
    hipLaunchKernelGGL(resize_backward_cols_kernel, dim3(stream_grid(c.planes * c.h_in * c.w_in, 16)), dim3(256), 0, c.s, c.tmp, c.gi, c.inv_x, c.planes * c.h_in, c.w_out, c.fw);
}

}  // namespace pbr

extern "C" {

// (the layout: carve_workspace)
size_t pbr_resize_backward_workspace_bytes(int64_t planes, int32_t h_in, int32_t w_in, int32_t h_out, int32_t w_out) {
    if (planes < 1 || h_in < 1 || w_in < 1 || h_out < 1 || w_out < 1) return 0;
    pbr::BackwardCall c = {nullptr, nullptr, planes, h_in, w_in, h_out, w_out};
    return pbr::carve_workspace(c, nullptr) * sizeof(float);
}

int pbr_resize_bilinear_backward(const void *grad_out, void *grad_in, int64_t planes, int32_t h_in, int32_t w_in, int32_t h_out,
                                 int32_t w_out, int antialias, void *workspace, void *stream) {
    using namespace pbr;
    if (!grad_out || !grad_in || !workspace) return PBR_ERR_NULL_MAP;
    if (planes < 1 || h_in < 1 || w_in < 1 || h_out < 1 || w_out < 1) return PBR_ERR_SHAPE;
    if (planes * h_in > INT32_MAX) return PBR_ERR_SHAPE;
    BackwardCall c = {static_cast<const float *>(grad_out), static_cast<float *>(grad_in), planes, h_in, w_in, h_out, w_out,
                      make_filter(w_in, w_out, antialias != 0), make_filter(h_in, h_out, antialias != 0), static_cast<hipStream_t>(stream)};
    carve_workspace(c, static_cast<float *>(workspace));
    const bool tuned = g_resize_up2 != 0;      // the register-only forms of an up-scale's gradient
    const bool done = (tuned && (backward_band_walk(c) || backward_two_tap(c))) || backward_gather(c) || backward_strip(c);
    if (!done) backward_generic(c);
    return launch_status();
}

}  // extern "C"
