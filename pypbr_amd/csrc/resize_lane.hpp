// resize_lane.hpp -- the lane frame of the one-wave register kernels of the bilinear resize (resize_up2_kernel in resize.hip,
// resize_up2_backward_kernel and resize_backward_gather_kernel in resize_backward.hip): a lane owns FOUR consecutive columns of R
// rows.  Where it stands, how its quad goes out, the gradient kernels' gather of one upstream row, and -- host side -- the launch
// geometry and the dispatch of the gather's window W.  The tap rule and the workgroup order: resize_taps.hpp.
#pragma once
#include <type_traits>

#include "resize_taps.hpp"

namespace pbr {

// A workgroup is one wave = 256 columns of a band of R rows (band = plane * groups_y + row / R), dealt to the XCDs in runs
// (xcd_run_order).  k0 is RAW, it may lie past the row's end: the forward keeps such lanes (its rows' taps are read across lanes),
// the gradient kernels return -- that stays with the caller.
struct LanePos { int plane, r0, k0; };
template <int R>
__device__ __forceinline__ LanePos lane_position(int groups_x, int groups_y, uint32_t xcd_groups) {
    const uint32_t wg = xcd_run_order(blockIdx.x, xcd_groups);
    const uint32_t band = wg / (uint32_t)groups_x, gx = wg - band * (uint32_t)groups_x;
    const int plane = (int)(band / (uint32_t)groups_y), r0 = (int)(band - (uint32_t)plane * (uint32_t)groups_y) * R;
    return {plane, r0, ((int)gx * 64 + (int)threadIdx.x) * 4};
}

// four values at q (element-aligned): one non-temporal 16-byte store, or -- the row's last, partial quad -- the first n
typedef float sf4 __attribute__((ext_vector_type(4), aligned(4)));
__device__ __forceinline__ void store_quad(float *q, const float v[4], bool whole, int n) {
    if (whole) {
        const sf4 t = {v[0], v[1], v[2], v[3]};
        __builtin_nontemporal_store(t, reinterpret_cast<sf4 *>(q));
    } else {
        for (int c = 0; c < n; ++c) q[c] = v[c];
    }
}

// The gradient kernels' accumulators, R rows of the lane's quad, fed from one upstream row: W / 4 16-byte loads, 4 W fma for the width
// sums t[c] = sum_j wx[c][j] g[j], 4 R fma with the row's weight cy(r) in each of the R gradient rows.  (They are cleared in the kernels:
// cleared in a function here, or by `= {}`, the tail store compiles to other code at other occupancies -- not measured, not taken.)
template <int W>
__device__ __forceinline__ void load_row(const float *row, float g[W]) {
#pragma unroll
    for (int q = 0; q < W / 4; ++q) {
        const rf4 v = *reinterpret_cast<const rf4 *>(row + 4 * q);       // cached: neighbouring lanes' and rows' windows overlap
        g[4 * q] = v.x; g[4 * q + 1] = v.y; g[4 * q + 2] = v.z; g[4 * q + 3] = v.w;
    }
}
template <int W>
__device__ __forceinline__ void width_sums(const float wx[4][W], const float g[W], float t[4]) {
#pragma unroll
    for (int c = 0; c < 4; ++c) {
        float a = wx[c][0] * g[0];
#pragma unroll
        for (int j = 1; j < W; ++j) a = fmaf(wx[c][j], g[j], a);
        t[c] = a;
    }
}
template <int W, int R, typename F>
__device__ __forceinline__ void gather_row(const float *row, const float wx[4][W], float acc[R][4], F &&cy) {
    float g[W], t[4];
    load_row<W>(row, g);
    width_sums<W>(wx, g, t);
#pragma unroll
    for (int r = 0; r < R; ++r) {
        const float w = cy(r);
#pragma unroll
        for (int c = 0; c < 4; ++c) acc[r][c] = fmaf(w, t[c], acc[r][c]);
    }
}
template <int R>
__device__ __forceinline__ void store_rows(float *gin, const LanePos &p, int h, int w, const float acc[R][4]) {
    float *dp = gin + (int64_t)p.plane * h * w + p.k0;
    const bool whole = p.k0 + 4 <= w;
#pragma unroll
    for (int r = 0; r < R; ++r) {
        if (p.r0 + r >= h) break;
        store_quad(dp + (int64_t)(p.r0 + r) * w, acc[r], whole, w - p.k0);
    }
}

// The first output of an up-scale whose two-tap window starts at input k - 1 or beyond (first_tap is monotone in the output index):
// a short search around the closed-form estimate, with the forward's own arithmetic.
__device__ __forceinline__ int first_reaching(const AxisFilter &f, int k, int n_out) {
    if (k <= 1) return 0;
    int i = (int)(((float)k - 0.5f) / f.scale - 0.5f) - 1;
    i = i < 0 ? 0 : (i > n_out - 1 ? n_out - 1 : i);
    while (i > 0 && first_tap(f, i - 1) >= k - 1) --i;
    while (i < n_out - 1 && first_tap(f, i) < k - 1) ++i;
    return i;
}

// Host: the grid of a one-wave kernel over cols x rows x planes with R rows per lane (`fits`: a 32-bit grid, else the caller's next
// form) and its launch -- the three kernels share their arguments up to the grid's; `tail`: the filters, or the tables.
struct LaneGrid { int groups_x, groups_y; unsigned n_groups; uint32_t xcd_groups; bool fits; };
inline LaneGrid lane_grid(int cols, int rows, int R, int64_t planes) {
    const int64_t groups_x = (cols + 255) / 256, groups_y = (rows + R - 1) / R, n_groups = groups_x * groups_y * planes;
    return {(int)groups_x, (int)groups_y, (unsigned)n_groups, xcd_run_groups(n_groups), n_groups <= INT32_MAX};
}
template <typename K, typename... A>
inline void launch_lanes(K kernel, const LaneGrid &g, hipStream_t s, const float *from, float *to, int h_in, int w_in, int h_out, int w_out, const A &...tail) {
    hipLaunchKernelGGL(kernel, dim3(g.n_groups), dim3(64), 0, s, from, to, h_in, w_in, h_out, w_out, g.groups_x, g.groups_y, g.xcd_groups, tail...);
}
// The gradient kernels' W for a worst window of `need` <= 16 upstream columns, as a constant (as with_width, launch_util.hpp):
//   with_window(need, [&](auto w) { constexpr int W = decltype(w)::value; ... kernel<W, ...> ... });
template <typename F> inline void with_window(int need, F &&f) {
    if (need <= 8) f(std::integral_constant<int, 8>{}); else if (need <= 12) f(std::integral_constant<int, 12>{}); else f(std::integral_constant<int, 16>{});
}

}  // namespace pbr
