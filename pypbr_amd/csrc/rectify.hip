// rectify.hip -- photographs (uint8 (H,W,C) samples, as PIL hands them out) -> the targets and coverage weights of a light-stack fit, on the
// texture grid: a homography warp with bilinear taps, zeros padding, optional supersampling and a clip level.  No upstream counterpart.
//
// The definition (include/pbr_hip.h, pbr_rectify_images; tools/rectify_oracle.py is the same in numpy float64).  Output
// pixel (y, x) of shot l, S = supersample, sub-samples (i, j), i, j < S:
//   X = x + (i + 0.5) / S,  Y = y + (j + 0.5) / S                      output pixel centres at + 0.5
//   d = m20 X + m21 Y + m22,  u = (m00 X + m01 Y + m02) / d - 0.5,  v = (m10 X + m11 Y + m12) / d - 0.5      source INDEX units
//   outside when d <= 0, u or v not finite, u <= -1, u >= Ws, v <= -1 or v >= Hs;
//   else the four bilinear taps around (floor u, floor v), weights from fx = u - floor u, fy = v - floor v; a tap outside the image
//   contributes nothing (zeros padding: F.grid_sample(bilinear, zeros, align_corners=False)), and so does a tap with a channel >= clip_level;
//   value_c = sum w_t sample_tc / 255 / S^2,  coverage = sum w_t / S^2,  weights = coverage,
//   targets_c = clamp(value_c / coverage, 0, 1) where coverage > 0, exactly 0 elsewhere.
// Coordinates are float64 (a float32 projective divide loses ~1e-3 source pixels at 4000-pixel photographs), fx and fy are rounded to
// float32 after the floor, weights and sums are float32.  The quotient is formed as one reciprocal of d and two products: 1.5 ulp of a
// double, and exact for d = 1, so an integer translation at S = 1 gives pbr_unpack_image's floats bit for bit (one tap of weight 1, the
// others 0, and sample / 255 the IEEE quotient) and weights of exactly 1 or 0.
//
// One launch for all images: the homographies travel in the kernel arguments, blockIdx.y is the image.  A workgroup covers a 2-D tile of
// the output -- under rotation an output row walks diagonally through the source, and a tile keeps the source footprint compact -- of
// (256 >> TILE_W_LOG2) rows by (1 << TILE_W_LOG2) lanes; the tile shape is a measured choice (tools/rectify_probe.py).
//   quad form     width % 4 == 0 and both outputs 16-byte aligned: a lane owns 4 consecutive pixels of a row, one 16-byte store per plane;
//   pixel form    everything else: one pixel per lane.  Both forms run the same rectify_pixel, so they agree bit for bit.
// Every element of both outputs is written exactly once; no workspace, no atomics, no LDS.  Addresses are 64-bit.
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstdint>

#include "../../include/pbr_hip.h"
#include "brdf_math.hpp"
#include "launch_util.hpp"

// Build-time variants, for tools/rectify_probe.py only (the library is built with the defaults).
#ifndef PBR_RECTIFY_COORD
#define PBR_RECTIFY_COORD double
#endif
#ifndef PBR_RECTIFY_TILE_W_LOG2
#define PBR_RECTIFY_TILE_W_LOG2 3               // 8 lanes x 32 rows: a 32 x 32 pixel tile in the quad form
#endif

namespace pbr {
namespace {

typedef PBR_RECTIFY_COORD coord_t;
constexpr int TILE_W_LOG2 = PBR_RECTIFY_TILE_W_LOG2;
constexpr int TILE_LANES_X = 1 << TILE_W_LOG2, TILE_ROWS = 256 >> TILE_W_LOG2;
static_assert(TILE_W_LOG2 >= 0 && TILE_W_LOG2 <= 8, "a tile is 256 lanes");

struct RectifyTable {
    double m[PBR_MAX_RECTIFY_IMAGES][9];
};

struct RectifySource {
    const uint8_t *src;
    int64_t image_stride, stride_h, stride_w, stride_c;
    int32_t height, width, clip_level;
};

// One output pixel of one image: its three targets and its weight.
template <int S, bool LINEAR>
__device__ __forceinline__ void rectify_pixel(const uint8_t *__restrict__ img, const RectifySource &g, const coord_t (&m)[9], int32_t x, int32_t y,
                                              float (&target)[3], float &weight) {
    constexpr coord_t step = (coord_t)1 / S;
    float acc[3] = {0.0f, 0.0f, 0.0f}, cov = 0.0f;
    for (int j = 0; j < S; ++j) {
        const coord_t Y = (coord_t)y + ((coord_t)j + (coord_t)0.5) * step;
        for (int i = 0; i < S; ++i) {
            const coord_t X = (coord_t)x + ((coord_t)i + (coord_t)0.5) * step;
            const coord_t d = m[6] * X + m[7] * Y + m[8];
            const coord_t r = (coord_t)1 / d;
            const coord_t u = (m[0] * X + m[1] * Y + m[2]) * r - (coord_t)0.5;
            const coord_t v = (m[3] * X + m[4] * Y + m[5]) * r - (coord_t)0.5;
            // every comparison is false for a NaN; an infinity fails its bound
            const bool inside = d > 0 && u > (coord_t)-1 && u < (coord_t)g.width && v > (coord_t)-1 && v < (coord_t)g.height;
            const coord_t us = inside ? u : (coord_t)0, vs = inside ? v : (coord_t)0;
            const coord_t fu = floor(us), fv = floor(vs);
            const float fx = (float)(us - fu), fy = (float)(vs - fv);
            const int32_t x0 = (int32_t)fu, y0 = (int32_t)fv;                      // [-1, Ws - 1], [-1, Hs - 1]
            const float wx[2] = {1.0f - fx, fx}, wy[2] = {1.0f - fy, fy};
#pragma unroll
            for (int ty = 0; ty < 2; ++ty) {
#pragma unroll
                for (int tx = 0; tx < 2; ++tx) {
                    const int32_t xi = x0 + tx, yi = y0 + ty;
                    bool live = inside && xi >= 0 && xi < g.width && yi >= 0 && yi < g.height;
                    // the address is formed from the clamped index: a dead tap reads a sample of the image and weighs it with 0
                    const int32_t xc = min(max(xi, 0), g.width - 1), yc = min(max(yi, 0), g.height - 1);
                    const uint8_t *p = img + (int64_t)yc * g.stride_h + (int64_t)xc * g.stride_w;
                    const uint32_t s0 = p[0], s1 = p[g.stride_c], s2 = p[2 * g.stride_c];
                    live = live && (g.clip_level == 0 || max(s0, max(s1, s2)) < (uint32_t)g.clip_level);
                    const float w = live ? wx[tx] * wy[ty] : 0.0f;
                    cov += w;
                    if (LINEAR) {
                        acc[0] = fmaf(w, srgb_to_linear((float)s0 / 255.0f), acc[0]);
                        acc[1] = fmaf(w, srgb_to_linear((float)s1 / 255.0f), acc[1]);
                        acc[2] = fmaf(w, srgb_to_linear((float)s2 / 255.0f), acc[2]);
                    } else {                                                         // w * s now, / 255 once per pixel below
                        acc[0] = fmaf(w, (float)s0, acc[0]);
                        acc[1] = fmaf(w, (float)s1, acc[1]);
                        acc[2] = fmaf(w, (float)s2, acc[2]);
                    }
                }
            }
        }
    }
    constexpr float inv = 1.0f / (S * S);                                            // a power of two: exact
    weight = fminf(cov * inv, 1.0f);                                                 // (four rounded weights can sum to 1 + 2^-23)
#pragma unroll
    for (int c = 0; c < 3; ++c) {
        const float value = (LINEAR ? acc[c] : acc[c] / 255.0f) * inv;
        target[c] = cov > 0.0f ? fminf(fmaxf(value / weight, 0.0f), 1.0f) : 0.0f;
    }
}

// V = 4: the quad form (width % 4 == 0, aligned outputs); V = 1: the pixel form.  blockIdx.x walks the tiles of one image row-major.
template <int S, bool LINEAR, int V>
__global__ __launch_bounds__(256) void rectify_kernel(RectifyTable tab, RectifySource g, float *__restrict__ targets, float *__restrict__ weights,
                                                      int32_t height, int32_t width, int32_t tiles_x) {
    const int32_t tile_y = (int32_t)blockIdx.x / tiles_x, tile_x = (int32_t)blockIdx.x - tile_y * tiles_x;
    const int32_t y = tile_y * TILE_ROWS + ((int32_t)threadIdx.x >> TILE_W_LOG2);
    const int32_t x = (tile_x * TILE_LANES_X + ((int32_t)threadIdx.x & (TILE_LANES_X - 1))) * V;
    if (y >= height || x >= width) return;                                           // (quad form: width % 4 == 0, so x + 3 < width)
    const int64_t l = blockIdx.y, plane = (int64_t)height * width;
    coord_t m[9];
#pragma unroll
    for (int k = 0; k < 9; ++k) m[k] = (coord_t)tab.m[l][k];
    const uint8_t *img = g.src + l * g.image_stride;
    float t[3][V], w[V];
#pragma unroll
    for (int p = 0; p < V; ++p) {
        float tp[3];
        rectify_pixel<S, LINEAR>(img, g, m, x + p, y, tp, w[p]);
        t[0][p] = tp[0]; t[1][p] = tp[1]; t[2][p] = tp[2];
    }
    const int64_t at = (int64_t)y * width + x;
    float *tdst = targets + l * 3 * plane + at, *wdst = weights + l * plane + at;
    if constexpr (V == 4) {
#pragma unroll
        for (int c = 0; c < 3; ++c) *reinterpret_cast<float4 *>(tdst + c * plane) = make_float4(t[c][0], t[c][1], t[c][2], t[c][3]);
        *reinterpret_cast<float4 *>(wdst) = make_float4(w[0], w[1], w[2], w[3]);
    } else {
#pragma unroll
        for (int c = 0; c < 3; ++c) tdst[c * plane] = t[c][0];
        wdst[0] = w[0];
    }
}

template <int S, bool LINEAR>
void launch_rectify(const RectifyTable &tab, const RectifySource &g, int32_t n_images, float *targets, float *weights, int32_t height, int32_t width,
                    bool quads, int64_t tiles_x, int64_t tiles, hipStream_t s) {
    const dim3 grid((uint32_t)tiles, (uint32_t)n_images);
    with_width(quads, [&](auto w) {
        constexpr int V = decltype(w)::value;
        hipLaunchKernelGGL((rectify_kernel<S, LINEAR, V>), grid, dim3(256), 0, s, tab, g, targets, weights, height, width, (int32_t)tiles_x);
    });
}

}  // namespace
}  // namespace pbr

extern "C" int pbr_rectify_images(const void *src, int32_t n_images, int32_t src_height, int32_t src_width, int64_t src_image_stride,
                                  int64_t src_stride_h, int64_t src_stride_w, int64_t src_stride_c, const double *homographies, float *targets,
                                  float *weights, int32_t height, int32_t width, int32_t supersample, int32_t clip_level, int32_t to_linear,
                                  void *stream) {
    using namespace pbr;
    if (!src || !homographies || !targets || !weights) return PBR_ERR_NULL_MAP;
    if (n_images < 1 || n_images > PBR_MAX_RECTIFY_IMAGES) return PBR_ERR_SHAPE;
    if (src_height < 1 || src_width < 1 || height < 1 || width < 1 || height > (1 << 30) || width > (1 << 30)) return PBR_ERR_SHAPE;   // (lane x, y stay int32)
    if ((int64_t)height * width > ((int64_t)1 << 40)) return PBR_ERR_SHAPE;
    if (supersample != 1 && supersample != 2 && supersample != 4) return PBR_ERR_SHAPE;
    if (clip_level < 0 || clip_level > 255) return PBR_ERR_SHAPE;
    if (src_image_stride < 0 || src_stride_h < 0 || src_stride_w < 0 || src_stride_c < 0) return PBR_ERR_SHAPE;
    RectifyTable tab;
    for (int32_t l = 0; l < PBR_MAX_RECTIFY_IMAGES; ++l)
        for (int k = 0; k < 9; ++k) {
            tab.m[l][k] = l < n_images ? homographies[9 * l + k] : 0.0;
            if (!std::isfinite(tab.m[l][k])) return PBR_ERR_SHAPE;
        }
    const RectifySource g = {static_cast<const uint8_t *>(src), src_image_stride, src_stride_h, src_stride_w, src_stride_c, src_height, src_width,
                             clip_level};
    const bool quads = width % 4 == 0 && all_aligned(16, {targets, weights});
    const int64_t tiles_x = ((quads ? width / 4 : width) + TILE_LANES_X - 1) / TILE_LANES_X, tiles_y = ((int64_t)height + TILE_ROWS - 1) / TILE_ROWS;
    const int64_t tiles = tiles_x * tiles_y;
    if (tiles > 0x7fffffff) return PBR_ERR_SHAPE;
    hipStream_t s = static_cast<hipStream_t>(stream);
    auto go = [&](auto ss) {
        constexpr int S = decltype(ss)::value;
        if (to_linear) launch_rectify<S, true>(tab, g, n_images, targets, weights, height, width, quads, tiles_x, tiles, s);
        else launch_rectify<S, false>(tab, g, n_images, targets, weights, height, width, quads, tiles_x, tiles, s);
    };
    if (supersample == 1) go(std::integral_constant<int, 1>{});
    else if (supersample == 2) go(std::integral_constant<int, 2>{});
    else go(std::integral_constant<int, 4>{});
    return launch_status();
}
