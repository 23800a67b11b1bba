// resize.hip -- antialiased bilinear resize of planar maps: the forward.
//
// Replaces MaterialBase.resize (/root/reference/pypbr/materials/base.py:490-504); the tap rule: resize_taps.hpp.  The gradient:
// resize_backward.hip.  The kernel families and which shapes each takes: pbr_resize_form in include/pbr_hip.h.  Here: the two-tap
// up-scale and the two generic passes; the general one-kernel form lives in resize_strip.hpp, the register-only band walk in
// resize_down.hpp, the row walk in resize_stream.hpp, the lane frame the two-tap kernel shares with the gradient's in resize_lane.hpp.
#include <hip/hip_runtime.h>

#include <cstdint>

#include "../../include/pbr_hip.h"
#include "resize_down.hpp"
#include "resize_lane.hpp"
#include "resize_stream.hpp"
#include "resize_strip.hpp"
#include "resize_taps.hpp"
#include "stream_shape.hpp"
#include "tuning.hpp"

namespace pbr {

// rows x n_in -> rows x n_out along the contiguous axis
__global__ __launch_bounds__(256) void resize_width_kernel(const float *__restrict__ src, float *__restrict__ dst,
                                                           int64_t rows, int n_out, AxisFilter f) {
    const int64_t total = rows * n_out;
    const int64_t stride = (int64_t)gridDim.x * blockDim.x;
    for (int64_t idx = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; idx < total; idx += stride) {
        const int64_t row = idx / n_out;
        const int i = (int)(idx - row * n_out);
        int xmin, xsize; float center;
        tap_window(f, i, xmin, xsize, center);
        const float *p = src + row * f.n_in + xmin;
        float acc = 0.0f, wsum = 0.0f;
        for (int j = 0; j < xsize; ++j) {
            const float w = tap_weight(f, j, xmin, center);
            acc = fmaf(w, p[j], acc);
            wsum += w;
        }
        dst[idx] = wsum != 0.0f ? acc / wsum : 0.0f;
    }
}

// planes x n_in x width -> planes x n_out x width down the rows
__global__ __launch_bounds__(256) void resize_height_kernel(const float *__restrict__ src, float *__restrict__ dst,
                                                            int64_t planes, int n_out, int width, AxisFilter f) {
    const int64_t total = planes * n_out * width;
    const int64_t stride = (int64_t)gridDim.x * blockDim.x;
    for (int64_t idx = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; idx < total; idx += stride) {
        const int x = (int)(idx % width);
        const int64_t t = idx / width;
        const int i = (int)(t % n_out);
        const int64_t plane = t / n_out;
        int ymin, ysize; float center;
        tap_window(f, i, ymin, ysize, center);
        const float *p = src + (plane * f.n_in + ymin) * width + x;
        float acc = 0.0f, wsum = 0.0f;
        for (int j = 0; j < ysize; ++j) {
            const float w = tap_weight(f, j, ymin, center);
            acc = fmaf(w, p[(int64_t)j * width], acc);
            wsum += w;
        }
        dst[idx] = wsum != 0.0f ? acc / wsum : 0.0f;
    }
}

// ---- up-scaling on both axes: two taps per axis, registers only ------------------------------------------------------------
// With scale <= 1 on both axes an output pixel has at most two taps per axis (support = 1), so neither the tap tables nor the
// LDS strip of resize_strip_kernel are needed: a lane owns FOUR consecutive output pixels of a row.  Their taps lie in at most five
// consecutive input columns; the lane loads six from each of the row's two input rows (one 16-byte and one 8-byte load per row,
// element-aligned), blends the rows first (the same order as the strip kernel: height, then width), and picks each output's two
// columns out of the six with selects.  Five vector-memory instructions per four output pixels instead of tables + LDS + barriers;
// the launch is bound by its writes (2.25 output pixels per input pixel at 1.5x).  One-wave workgroups = 256 output pixels of a
// row; workgroups are dealt to the XCDs in runs (xcd_run_order: every XCD keeps whole bands of output rows, so the input rows two
// output rows share meet in one L2).
// kUpRows: output rows per lane -- the column taps are formed once for all of them
template <int kUpRows>
__global__ __launch_bounds__(64) void resize_up2_kernel(const float *__restrict__ src, float *__restrict__ dst, int h_in, int w_in, int h_out,
                                                        int w_out, int groups_x, int groups_y, uint32_t xcd_groups, AxisFilter fw, AxisFilter fh) {
    const LanePos p = lane_position<kUpRows>(groups_x, groups_y, xcd_groups);
    const int plane = p.plane, yb = p.r0;
    // Lanes past the row's end stay in the wave (they work on column 0 and store nothing): the rows' taps below are read ACROSS lanes,
    // and a lane that has left has no defined values (the compiler is free to form them after the exit).
    const bool live = p.k0 < w_out;
    const int x0 = live ? p.k0 : 0;
    // The rows' taps are wave-uniform (every lane of the workgroup works on rows yb .. yb + kUpRows - 1) but floating-point: the scalar unit
    // cannot form them, and formed per lane they were ~30 vector instructions per row and lane (VALU busy 0.69 in a launch that should wait
    // for its stores).  Lane r forms row r's taps ONCE; the others read them through v_readlane (same arithmetic, same bits).
    int ty0; float tw0, tw1;
    two_taps(fh, min(yb + (int)(threadIdx.x & (kUpRows - 1)), h_out - 1), ty0, tw0, tw1);
    int first[4]; float wa[4], wb[4];
#pragma unroll
    for (int k = 0; k < 4; ++k) two_taps(fw, min(x0 + k, w_out - 1), first[k], wa[k], wb[k]);
    const int xb = min(first[0], w_in - 6);                 // six columns from xb on, inside the row
    int o[4];
#pragma unroll
    for (int k = 0; k < 4; ++k) o[k] = first[k] - xb;       // 0 .. 5 (5 only at the right edge, where the second tap's weight is 0)
    const float *sp = src + (int64_t)plane * h_in * w_in + xb;
    float *dp = dst + ((int64_t)plane * h_out) * w_out + x0;
    const bool whole = x0 + 4 <= w_out;
#pragma unroll
    for (int r = 0; r < kUpRows; ++r) {
        const int y = yb + r;
        if (y >= h_out) break;
        const int y0 = __builtin_amdgcn_readlane(ty0, r);
        const float wy0 = __builtin_bit_cast(float, __builtin_amdgcn_readlane(__builtin_bit_cast(int, tw0), r));
        const float wy1 = __builtin_bit_cast(float, __builtin_amdgcn_readlane(__builtin_bit_cast(int, tw1), r));
        const int y1 = min(y0 + 1, h_in - 1);               // a one-tap window at the last row: weight 0 on a valid row
        const float *r0 = sp + (int64_t)y0 * w_in, *r1 = sp + (int64_t)y1 * w_in;
        const rf4 a4 = *reinterpret_cast<const rf4 *>(r0), b4 = *reinterpret_cast<const rf4 *>(r1);
        const rf2 a2 = *reinterpret_cast<const rf2 *>(r0 + 4), b2 = *reinterpret_cast<const rf2 *>(r1 + 4);
        float mid[6];                                       // height pass first, as the strip kernel: acc = w0 v0, then fma(w1, v1, acc)
        mid[0] = fmaf(wy1, b4.x, wy0 * a4.x); mid[1] = fmaf(wy1, b4.y, wy0 * a4.y); mid[2] = fmaf(wy1, b4.z, wy0 * a4.z);
        mid[3] = fmaf(wy1, b4.w, wy0 * a4.w); mid[4] = fmaf(wy1, b2.x, wy0 * a2.x); mid[5] = fmaf(wy1, b2.y, wy0 * a2.y);
        float out[4];
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            const int ok = o[k];
            const float va = ok == 0 ? mid[0] : (ok == 1 ? mid[1] : (ok == 2 ? mid[2] : (ok == 3 ? mid[3] : (ok == 4 ? mid[4] : mid[5]))));
            const float vb = ok == 0 ? mid[1] : (ok == 1 ? mid[2] : (ok == 2 ? mid[3] : (ok == 3 ? mid[4] : mid[5])));
            out[k] = fmaf(wb[k], vb, wa[k] * va);
        }
        float *q = dp + (int64_t)y * w_out;
        if (!live) continue;
        store_quad(q, out, whole, w_out - x0);
    }
}

// The three weight vectors of resize_down_kernel for the whole factor S (antialiased): an axis of 16 outputs has them all -- output 0 (window clipped
// on the left), output 5 (whole window) and output 15 (clipped on the right) -- and they do not depend on the axis' length: with n_in = S n_out the
// tap positions relative to the window are small whole and half numbers, exact in float, whatever the output's index.  Formed with the strip kernel's statements (phase 0 of resize_strip_kernel).
static DownTaps down_taps(int S) {
    const AxisFilter f = make_filter(16 * S, 16, true);
    return make_down_taps([&](int i, float *w) {
        int xmin, n; float center;
        const float inv = window_norm(f, i, xmin, n, center);
        const int shift = xmin - (S * i - S / 2);            // the window's first tap among the K = 2 S of an unclipped one
        for (int j = 0; j < n; ++j)
            if (shift + j >= 0 && shift + j < 32) w[shift + j] = tap_weight(f, j, xmin, center) * inv;
    });
}
// Launch of resize_down_kernel: `small` = the side with 1 / S^2 of the elements (the down-scale's result, the up-scale's gradient).  False when the
// shape is not the kernel's (the caller goes on to its other forms).
bool launch_down(const float *large, float *small, int64_t planes, int h_small, int w_small, int S, const DownTaps &taps, hipStream_t s, bool dry) {
    // A lane owns 32 bytes of every row of the large side (8 / S columns of the small one) and walks down a band of rows, R rows of the small side per turn
    // of its loop, the next large row in flight.  Bands are cut so that the launch has ~1 536 waves -- six per CU, which then run side by side from
    // the first to the last row: 3 x 4096^2 -> 2048^2 | 1024^2 | 512^2 (us) with 1 280 / 1 536 / 1 792 / 2 048 / 2 560 / 3 072 / 4 096 / 6 144 waves:
    // 37.6 / 37.2 / 39.3 / 39.4 / 42.1 / 40.0 / 40.1 / 42.7 | 34.2 / 32.4 / 32.3 / 32.3 / 34.2 / 34.4 / 34.3 / 39.2 | 35.1 / 33.8 / 33.9 / 33.9 / 35.6 / 37.8 / 37.8 / 46.1
    // (tools/resize_down_probe.py; the strip kernel: 45.6 | 36.4, and 185 for the two passes the 19 taps of an 8 x down-scale fell to).  64 bytes per
    // lane (16 lines per load instruction instead of 8), 3 or 7 rows in flight, 4 or 8 rows per turn: level or 2-8 % slower; non-temporal loads:
    // 1.4-1.8 x slower (a lane's two 16-byte loads of a row are two instructions on the same lines).
    // These shapes -- one 3-plane 4096^2 map, 201 MB -- sit in the 256 MB memory-side cache between launches, and only cached (plain) loads find them there.
    // A large side that cannot (EIGHT planes, 537 MB: nothing survives a launch) reads 122.4 / 117.6 us at 1 536 / 2 048 waves for 2x (strip kernel 128), 123.0 / 112.3
    // for 4x (118), 99 / 96 for 8x (two passes: 516) -- 0.64-0.71 of HBM, what cached loads stream at on this part (tools/membench.hip: read-only plain 5.6 TB/s,
    // non-temporal 6.2).  There the lanes own 16 bytes of a row instead (4 / S columns: every line is touched by ONE instruction), loaded non-temporally,
    // three rows in flight: 111.8 (0.75) | 108.4 (0.66); on the 3-plane shapes that form costs 36.8 -> 50 | 32.0 -> 46 (it streams past the memory-side cache).
    if (S < 2 || (S > 8 && S != 16) || w_small % 4 != 0 || w_small < 8 || h_small < 2) return false;
    if (!is_aligned(large, 16) || !is_aligned(small, 16)) return false;
    const bool streams = (int64_t)planes * h_small * w_small * S * S * 4 > (256ll << 20);      // the large side does not fit the memory-side cache
    const bool narrow = streams && (S == 2 || S == 4);           // 16 bytes of a row per lane, non-temporal loads
    // columns of the small side per lane: 32 bytes of the large side's row where S divides 8, else the fewest whose S-fold is a whole number of 16-byte pieces
    const int cols = narrow ? 4 / S : (S == 16 ? 1 : (8 % S == 0 ? 8 / S : (S == 6 ? 2 : 4))), R = S == 2 ? 4 : 2;      // ... and its rows per turn of the kernel's loop (16 x: 64 bytes per lane)
    const int64_t groups_x = (w_small + 64 * cols - 1) / (64 * cols);
    int64_t bands = (streams ? 2048 : 1536) / (planes * groups_x);
    bands = bands < 1 ? 1 : bands;
    int64_t band_rows = (h_small + bands - 1) / bands;
    band_rows = (band_rows + R - 1) / R * R;
    bands = (h_small + band_rows - 1) / band_rows;               // every band holds at least one row
    const int64_t pairs = planes * bands, n_groups = pairs * groups_x;
    if (n_groups > INT32_MAX) return false;
    const uint32_t mapped = (uint32_t)((pairs / 8) * 8 * groups_x);      // the (plane, band) pairs dealt to the XCDs by eights
    void (*fn)(const float *, float *, int, int, int, int, int, uint32_t, const DownTaps) = nullptr;
    switch (S) {
        case 2: fn = resize_down_kernel<2, 4, 4, 1>; break;
        case 3: fn = resize_down_kernel<3, 2, 4, 1>; break;
        case 4: fn = resize_down_kernel<4, 2, 2, 1>; break;
        case 5: fn = resize_down_kernel<5, 2, 4, 1>; break;
        case 6: fn = resize_down_kernel<6, 2, 2, 1>; break;
        case 7: fn = resize_down_kernel<7, 2, 4, 1>; break;
        case 8: fn = resize_down_kernel<8, 2, 1, 1>; break;
        default: fn = resize_down_kernel<16, 2, 1, 1>; break;
    }
    if (narrow) fn = S == 2 ? resize_down_kernel<2, 4, 2, 3, true> : resize_down_kernel<4, 2, 1, 3, true>;
    if (dry) return true;                                   // (pbr_resize_form: the shape is this kernel's)
    hipLaunchKernelGGL(fn, dim3((unsigned)n_groups), dim3(64), 0, s, large, small, h_small, w_small, (int)groups_x, (int)bands, (int)band_rows, mapped, taps);
    return true;
}

// Launch of resize_stream_kernel (resize_stream.hpp): antialiased down-scales by any factor 1.01 <= s < 17 on both axes.  False when the shape is
// not the kernel's (the caller goes on to the strip form).  `workspace` holds the tables: pbr_resize_workspace_bytes is planes x h_in x w_out floats,
// the tables need 5 h_in + 2 h_out + (kt + 2) w_out.
static bool launch_stream(const float *src, float *dst, int64_t planes, int h_in, int w_in, int h_out, int w_out, const AxisFilter &fw, const AxisFilter &fh,
                          float *workspace, hipStream_t s, bool dry = false) {
    if (fw.scale < 1.01f || fh.scale < 1.01f || fw.support != fw.scale || fh.support != fh.scale) return false;      // (support = scale: antialiased)
    if ((int)(2.0f * fw.support) + 3 > 36 || (int)(2.0f * fh.support) + 3 > 36 || w_in % 4 != 0 || w_out < 16 || h_out < 4) return false;      // (the strip form's range of taps)
    if (!is_aligned(src, 16) || !is_aligned(workspace, 16)) return false;
    const int kt = (int)(2.0f * fw.support) + 2, kw = (kt + 3) & ~3;    // rows of the column table (a window holds at most ceil(2 s) taps: hi - lo < 2 s + 1); taps the width pass walks: whole groups of four
    const size_t words = 4 * (size_t)h_in + (size_t)h_in + 2 * (size_t)h_out + (size_t)(kt + 2) * (size_t)w_out;
    if (words > (size_t)planes * (size_t)h_in * (size_t)w_out) return false;
    // One 16-byte piece of a row per lane (a strip spans 256 input columns), four rows in flight, ~2 048 workgroups, whatever the factor and the number of
    // planes (tools/resize_stream_probe.py on 3 | 8 x 4096^2 -> 3000^2 ... 300^2, every repetition on freshly allocated buffers, with boost clocks AND after 150 ms
    // of launches: two pieces per lane level to 20 % slower; 1 024 | 1 536 | 3 072 | 4 096 workgroups 20 | 3 | 2-20 | 5-20 % slower; eight rows in flight 3-6 % slower;
    // 6 144 ... 24 576 short bands dispatched in memory order: 5-25 % slower from 2 x up).
    constexpr int P = 1, D = 4;
    const bool nt = (int64_t)planes * h_in * w_in * 4 > (256ll << 20);      // the input does not fit the memory-side cache: it streams (8 x 4096^2: 110 -> 101 us at 10 x)
    // output columns per strip: as many as keep every strip's window (its start aligned down to 16 bytes) within 256 P input columns
    auto window_fits = [&](int oc) {
        for (int xb = 0; xb < w_out; xb += oc) {
            const int last = (xb + oc < w_out ? xb + oc : w_out) - 1;
            int lo, n, lo2, n2; float c;
            tap_window(fw, xb, lo, n, c);
            tap_window(fw, last, lo2, n2, c);
            if (lo2 + n2 - (lo & ~3) > 256 * P) return false;
        }
        return true;
    };
    int oc = (int)(((float)(256 * P - 5) - 2.0f * fw.support) / fw.scale);
    if (oc > w_out) oc = w_out;
    while (oc >= 8 && !window_fits(oc)) --oc;
    if (oc < 8) return false;
    const int64_t strips = (w_out + oc - 1) / oc;
    int64_t bands = 2048 / (planes * strips);
    bands = bands < 1 ? 1 : bands;
    int64_t band_rows = (h_out + bands - 1) / bands;
    band_rows = band_rows < 4 ? 4 : band_rows;
    bands = (h_out + band_rows - 1) / band_rows;
    const int64_t pairs = planes * bands, n_groups = pairs * strips;
    if (n_groups > INT32_MAX) return false;
    const size_t lds = sizeof(float) * ((size_t)2 * (4 / P) * (256 * P + 40) + (size_t)(kw + 2) * oc + 8);      // two buffers of finished rows | the strip's column table | two notes
    if (lds > 32 * 1024) return false;
    if (dry) return true;
    float4 *rec = reinterpret_cast<float4 *>(workspace);
    int *orow = reinterpret_cast<int *>(rec + h_in), *ylo = orow + h_in, *yhi = ylo + h_out, *xlo = yhi + h_out, *xn = xlo + w_out;
    float *wx = reinterpret_cast<float *>(xn + w_out);
    const int groups_y = (h_in + 255) / 256, groups_x = (w_out + 255) / 256;
    hipLaunchKernelGGL(resize_stream_tables_kernel, dim3(groups_y + groups_x), dim3(256), 0, s, rec, orow, ylo, yhi, xlo, xn, wx, kt, h_out, w_out, fh, fw, groups_y);
    const StreamGeom g = {h_out, w_out, h_in, w_in, kw, kt, oc, (int)strips, (int)bands, (int)band_rows, (uint32_t)((pairs / 8) * 8 * strips)};
    auto fn = nt ? resize_stream_kernel<P, D, true> : resize_stream_kernel<P, D, false>;
    hipLaunchKernelGGL(fn, dim3((unsigned)n_groups), dim3(128), lds, s, src, dst, g, rec, orow, ylo, yhi, xlo, xn, wx);
    return true;
}

}  // namespace pbr

extern "C" {

size_t pbr_resize_workspace_bytes(int64_t planes, int32_t h_in, int32_t w_out) {
    return planes < 1 || h_in < 1 || w_out < 1 ? 0 : (size_t)planes * (size_t)h_in * (size_t)w_out * sizeof(float);
}

// pbr_resize_bilinear and pbr_resize_form: `form` receives the kernel family; `dry` = decide, launch nothing
static int resize_forward(const void *src, void *dst, int64_t planes, int32_t h_in, int32_t w_in, int32_t h_out,
                          int32_t w_out, int antialias, void *workspace, void *stream, bool dry, int *form) {
    using namespace pbr;
    if (!src || !dst || !workspace) return PBR_ERR_NULL_MAP;
    if (planes < 1 || h_in < 1 || w_in < 1 || h_out < 1 || w_out < 1) return PBR_ERR_SHAPE;
    hipStream_t s = static_cast<hipStream_t>(stream);
    float *tmp = static_cast<float *>(workspace);
    const AxisFilter fw = make_filter(w_in, w_out, antialias != 0), fh = make_filter(h_in, h_out, antialias != 0);
    if (g_resize_up2 && fw.scale <= 1.0f && fh.scale <= 1.0f && w_in >= 6) {
        // up-scaling (or 1:1) on both axes: the two-tap register form.  3 x 4096^2 -> 6144^2 (resize_sweep.py).
        // Output rows per lane.  Measured (resize_up_ab.py, 3 planes, us, rows 2 / 4 / 8; strip kernel for scale):
        //   4096^2 -> 6144^2  131.4 / 121.6 / 110.8 (157)    -> 8192^2  215.3 / 195.5 / 184.7 (270)    2048^2 -> 4096^2  59.0 / 53.6 / 53.0 (64)
        //   4096^2 -> 4608^2   79.1 /  70.0 /  73.1 (101)    -> 4096^2   63.7 /  61.2 /  66.0 (95)
        // 8 from 1.25x up (the column taps' share shrinks as the rows grow), 4 below.
        const int rows = fh.scale <= 0.8f ? 8 : 4;
        const LaneGrid grid = lane_grid(w_out, h_out, rows, planes);
        if (grid.fits) {
            auto fn = rows == 8 ? resize_up2_kernel<8> : resize_up2_kernel<4>;
            *form = PBR_RESIZE_TWO_TAP;
            if (dry) return PBR_OK;
            launch_lanes(fn, grid, s, static_cast<const float *>(src), static_cast<float *>(dst), h_in, w_in, h_out, w_out, fw, fh);
            return launch_status();
        }
    }
    if (g_resize_up2 && antialias && h_in % h_out == 0 && w_in % w_out == 0 && h_in / h_out == w_in / w_out && h_in / h_out >= 2 && h_in / h_out <= 16 &&
        launch_down(static_cast<const float *>(src), static_cast<float *>(dst), planes, h_out, w_out, h_in / h_out, down_taps(h_in / h_out), s, dry)) {
        // a whole factor 2 ... 8 | 16 on both axes: the register form (resize_down.hpp)
        *form = PBR_RESIZE_BAND_WALK;
        if (dry) return PBR_OK;
        return launch_status();
    }
    // Antialiased down-scales from 7 x up that are not a whole factor (17 ... 36 taps per axis, (int)(2 s) + 3: the strip form's WIDE instantiation): every input row once
    // (resize_stream.hpp).  tools/resize_stream_probe.py, us, walk | strip, after 150 ms of launches (settled clocks), every repetition on freshly allocated buffers:
    //   8 x 4096^2 -> 400^2  100 | 126     -> 300^2  97 | 128     3 x 4096^2 -> 400^2  35-40 | 44     -> 300^2  42 | 60
    // The walk is built and bit-identical for every factor from 1.01 x (knob value 2 takes it wherever the shape allows) but NOT the rule below 7 x, where
    // its STORES decide: the walking wave alone streams 8 x 4096^2 at its read-only pattern (87-95 us) at every factor and clock, the width pass's arithmetic is free from
    // 2 x up, and the result's stores cost 0.45-0.9 us per MB where the strip form pays 0.26 (not understood: DESIGN.md section 9).  At boost clocks (the first ~20 launches
    // after an idle moment) 8 x 4096^2 -> 2000^2 | 1365^2 | 1000^2 read 120 | 107 | 102 against the strip form's 140 | 119 | 108; after 150 ms of launches 139 | 125-132 | 107
    // against 140 | 117-122 | 108, and below 2 x 187-243 against 154-174 -- on three boxes of four: on the fourth the stores drain fast enough for the walk to win from 1.5 x up
    // (106 against 117 at 1365^2, equally settled); the strip form's figures do not move.  A cache-resident input (3 planes) between 2.2 x and 7 x is 2-6 % faster
    // through the strip form.  Every step: profiles/EXPERIMENTS.md.
    const bool walk = (int)(2.0f * fw.support) + 3 > 16 || (int)(2.0f * fh.support) + 3 > 16;
    if (g_resize_up2 && antialias && (walk || g_resize_up2 == 2) &&
        launch_stream(static_cast<const float *>(src), static_cast<float *>(dst), planes, h_in, w_in, h_out, w_out, fw, fh, tmp, s, dry)) {
        *form = PBR_RESIZE_ROW_WALK;
        if (dry) return PBR_OK;
        return launch_status();
    }
    {   // strip form: tap tables + the height-reduced strip [toh][pitch] of a toh x 64 output tile in LDS, up to 36 taps per axis
        // (16 -> 36 taps, i.e. down-scales below 17x keep the one-kernel form)
        const int kx = (int)(2.0f * fw.support) + 3, ky = (int)(2.0f * fh.support) + 3;      // taps per output: xsize <= 2 support + 2
        const int cols_max = (int)(kTileW * fw.scale + 2.0f * fw.support) + 4 + 3;           // + 3: window start aligned down to 16 bytes
        // Output rows per workgroup: as many as keep the workgroup's LDS within 24 KiB (6 workgroups per CU).  More rows
        // amortise the tables and re-read fewer input rows; more resident workgroups overlap the phases
        // (resize_sweep.py: 2x down 32-64 rows, 3-4x down 16, up-scales 64-128).
        // 16-byte stores in the forward width pass (QUADS): 62.7 against 54.0 us with them (4096^2 -> 2048^2): never.
        StripLaunch l;
        if (kx <= 36 && ky <= 36 && strip_launch(l, planes, h_out, w_out, kx, ky, cols_max, w_in % 4 == 0 && is_aligned(src, 16), 40, 24 * 1024)) {
            auto strip = kx <= 16 && ky <= 16 ? resize_strip_kernel<false, false> : resize_strip_kernel<false, false, true>;
            *form = PBR_RESIZE_STRIP;
            if (dry) return PBR_OK;
            hipLaunchKernelGGL(strip, dim3(l.tiles), dim3(256), l.lds, s,
                               static_cast<const float *>(src), static_cast<float *>(dst), (int)h_out, (int)w_out, (int)w_in, l.tg, fw, fh, StripTables{});
            return launch_status();
        }
    }
    // more than 36 taps per axis (down-scales from 17x): two passes through `workspace`
    *form = PBR_RESIZE_TWO_PASS;
    if (dry) return PBR_OK;
    hipLaunchKernelGGL(resize_width_kernel, dim3(stream_grid(planes * h_in * w_out, 16)), dim3(256), 0, s,
                       static_cast<const float *>(src), tmp, planes * h_in, (int)w_out, fw);
    hipLaunchKernelGGL(resize_height_kernel, dim3(stream_grid(planes * h_out * w_out, 16)), dim3(256), 0, s,
                       tmp, static_cast<float *>(dst), planes, (int)h_out, (int)w_out, fh);
    return launch_status();
}

int pbr_resize_bilinear(const void *src, void *dst, int64_t planes, int32_t h_in, int32_t w_in, int32_t h_out,
                        int32_t w_out, int antialias, void *workspace, void *stream) {
    int form = 0;
    return resize_forward(src, dst, planes, h_in, w_in, h_out, w_out, antialias, workspace, stream, false, &form);
}

int pbr_resize_form(const void *src, const void *dst, int64_t planes, int32_t h_in, int32_t w_in, int32_t h_out,
                    int32_t w_out, int antialias, const void *workspace) {
    int form = -1;
    const int rc = resize_forward(src, const_cast<void *>(dst), planes, h_in, w_in, h_out, w_out, antialias, const_cast<void *>(workspace), nullptr, true, &form);
    return rc == PBR_OK ? form : -1;
}

}  // extern "C"
