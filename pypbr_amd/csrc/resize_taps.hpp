// resize_taps.hpp -- the tap rule of the bilinear resize and the workgroup order of its one-wave kernels: what host and device, the forward
// (resize.hip) and the gradient (resize_backward.hip) share.  The lane frame of those kernels builds on this file: resize_lane.hpp.
//
// MaterialBase.resize (/root/reference/pypbr/materials/base.py:490-504) calls torchvision.transforms.functional.resize on every (C,H,W)
// float map; for float tensors that is torch.nn.functional.interpolate(mode="bilinear", align_corners=False, antialias=...).
// ATen's antialiased kernel is separable (width pass, then height pass, fp32 intermediate); per
// output index i along an axis of input size n_in and output size n_out:
//     scale   = n_in / n_out                 support = antialias && scale >= 1 ? scale : 1
//     center  = scale * (i + 0.5)            invscale = antialias && scale >= 1 ? 1/scale : 1
//     xmin    = max(0, (int)(center - support + 0.5))
//     xsize   = min(n_in, (int)(center + support + 0.5)) - xmin
//     w_j     = max(0, 1 - |(j + xmin - center + 0.5) * invscale|),  normalised to sum 1
// With antialias off (or when up-scaling) this reduces to the ordinary 2-tap bilinear rule with
// edge clamping, so one rule covers both settings.
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>

namespace pbr {

struct AxisFilter {
    float scale, support, invscale;
    int n_in;
};

inline AxisFilter make_filter(int n_in, int n_out, bool antialias) {
    AxisFilter f;
    f.scale = (float)n_in / (float)n_out;            // area_pixel_compute_scale<float>, align_corners = False
    const bool aa = antialias && f.scale >= 1.0f;
    f.support = aa ? f.scale : 1.0f;                 // interp_size / 2 * scale, interp_size = 2
    f.invscale = aa ? 1.0f / f.scale : 1.0f;
    f.n_in = n_in;
    return f;
}

__host__ __device__ __forceinline__ void tap_window(const AxisFilter &f, int i, int &xmin, int &xsize, float &center) {
    center = f.scale * ((float)i + 0.5f);
    const int lo = (int)(center - f.support + 0.5f), hi = (int)(center + f.support + 0.5f);
    xmin = lo > 0 ? lo : 0;
    xsize = (hi < f.n_in ? hi : f.n_in) - xmin;
}
// first tap of output i (the window's start): what the gradient kernels bracket their contributors with; host and device agree bit for bit
__host__ __device__ __forceinline__ int first_tap(const AxisFilter &f, int i) {
    int xmin, n; float c;
    tap_window(f, i, xmin, n, c);
    return xmin;
}

__host__ __device__ __forceinline__ float tap_weight(const AxisFilter &f, int j, int xmin, float center) {
    const float x = ((float)(j + xmin) - center + 0.5f) * f.invscale;
    return fmaxf(0.0f, 1.0f - fabsf(x));
}
// the window of output i and its normalisation: 1 / (sum of its taps' weights), 0 for a window without weight (0 x inf must not become NaN)
__host__ __device__ __forceinline__ float window_norm(const AxisFilter &f, int i, int &xmin, int &n, float &center) {
    float wsum = 0.0f;
    tap_window(f, i, xmin, n, center);
    for (int j = 0; j < n; ++j) wsum += tap_weight(f, j, xmin, center);
    return wsum != 0.0f ? 1.0f / wsum : 0.0f;
}

// the two normalised taps of an up-scale's output (scale <= 1: support = 1) -- resize_up2_kernel and its transposes
typedef float rf4 __attribute__((ext_vector_type(4), aligned(4)));
typedef float rf2 __attribute__((ext_vector_type(2), aligned(4)));
__device__ __forceinline__ void two_taps(const AxisFilter &f, int i, int &first, float &w0, float &w1) {
    int n; float center;
    tap_window(f, i, first, n, center);
    const float a = tap_weight(f, 0, first, center), b = n > 1 ? tap_weight(f, 1, first, center) : 0.0f;
    const float inv = __builtin_amdgcn_rcpf(a + b);         // a + b > 0: the window always holds the tap nearest the centre (1 ulp; the
    w0 = a * inv; w1 = b * inv;                             // strip kernel divides -- results agree to ~1e-7, both <= 2e-6 from ATen)
}

// XCD run order of the one-wave kernels (resize_up2_kernel, resize_up2_backward_kernel, resize_backward_gather_kernel): workgroups are
// dealt to the 8 XCDs round-robin, and XCD x takes runs of 1 << kUpRunLog2 consecutive workgroups (tile_of_workgroup's map in
// ct_kernel.hpp), so that every XCD keeps whole bands of rows and the rows two neighbours share meet in one L2.  The launch's last,
// partial span of 8 runs keeps the identity order: xcd_run_groups is the number of workgroups in whole spans.
constexpr int kUpRunLog2 = 9;
__device__ __forceinline__ uint32_t xcd_run_order(uint32_t wg, uint32_t xcd_groups) {
    if (wg < xcd_groups) {
        const uint32_t c = kUpRunLog2, xcd = wg & 7u, slot = wg >> 3;
        wg = ((slot >> c) << (c + 3)) + (xcd << c) + (slot & ((1u << c) - 1u));
    }
    return wg;
}
inline uint32_t xcd_run_groups(int64_t n_groups) {
    const uint32_t span = 8u << kUpRunLog2;
    return (uint32_t)(n_groups / span) * span;
}

}  // namespace pbr
