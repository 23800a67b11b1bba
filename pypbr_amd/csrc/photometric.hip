// photometric.hip -- a rectified light stack (targets [L][3][H][W], weights) -> the maps a fit starts from: Lambertian photometric stereo
// with reweighting passes against attached shadows, per pixel, in one launch.  No upstream counterpart.
//
// The definition (include/pbr_hip.h, pbr_photometric_stereo; the numpy restatement lives under tools/).  Pixel
// (y, x), P = (xs[x], -ys[y], 0) on the point light's grid:
//   geometry     point: d = light_l - P, w_l = d / (|d| + 1e-7), a_l = 1 / (|d|^2 + 1e-7); directional: w_l = normalize(light_l), a_l = 1
//   observation  r_lc = lin(T_lc) / (I_lc a_l), y_l = (r_l0 + r_l1 + r_l2) / 3
//   pass k < K   u_l = weight_l m_l (m = 1 at first); shots with u_l == 0 are SKIPPED; A = sum u w w^T, b = sum u y w; t = tr A,
//                c = det A / (t/3)^3 (0 when t <= 0); c < kappa: invalid.  g = adj(A) b / det A; |g| 0 or not finite, or g_z <= 0: invalid.
//                k < K - 1: m_l = [w_l . g > tau |g|]
//   normal       g / |g| (valid) | (0, 0, 1) with u_l = weight_l (invalid)
//   albedo_c     clamp(pi sum u s r_c / sum u s^2, 0, 1), s_l = max(w_l . n, 0); 0 where the denominator is 0
//   confidence   c (valid) | 0 (invalid)
//
// One launch, registers only: a lane owns V consecutive pixels of a row and walks the L shots once per pass (K solves at most, then the
// albedo).  What a pass needs again -- r_lc, the weight -- is READ again, not kept: a register array indexed by a run-time l would go to
// scratch, and held for 16 shots it is 64 registers per pixel (the variant PBR_PHOTOMETRIC_CACHE keeps them, one pixel per lane, the shot
// loops unrolled under l < L predicates; measured by tools/photometric_probe.py, profiles/EXPERIMENTS.md).  The mask m is 16 bits of one
// register.  A pass after the first is skipped by a pixel whose mask did not change -- the pass would repeat the one before it bit for
// bit -- and by a lane none of whose pixels still iterates.
//   quad form     width % 4 == 0 and all five pointers 16-byte aligned: V = 4, one 16-byte access per plane;
//   pixel form    everything else: V = 1.  A pixel's arithmetic does not depend on its neighbours: the forms agree bit for bit.
// A workgroup is a tile of 16 lanes x 16 rows.  Every output element is written exactly once; no workspace, no atomics, no LDS; 64-bit
// addresses.  The lights travel in the kernel arguments: 16 x 6 floats.
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstdint>

#include "../../include/pbr_hip.h"
#include "brdf_math.hpp"
#include "ct_kernel.hpp"
#include "launch_util.hpp"

// Build-time variant, for tools/photometric_probe.py only (the library is built with 0): 16 keeps every shot's r_lc and weight in registers.
#ifndef PBR_PHOTOMETRIC_CACHE
#define PBR_PHOTOMETRIC_CACHE 0
#endif

namespace pbr {
namespace {

constexpr int PS_CACHE = PBR_PHOTOMETRIC_CACHE;
constexpr int PS_TILE_W_LOG2 = 4, PS_TILE_LANES_X = 1 << PS_TILE_W_LOG2, PS_TILE_ROWS = 256 >> PS_TILE_W_LOG2;
static_assert(PS_CACHE == 0 || PS_CACHE == PBR_MAX_PHOTOMETRIC_SHOTS, "the shots are read again, or all of them are kept");

struct PsLights {
    float light[PBR_MAX_PHOTOMETRIC_SHOTS][3];          // point: the position; directional: the UNIT direction (normalised on the host)
    float inv_intensity[PBR_MAX_PHOTOMETRIC_SHOTS][3];  // 1 / I_lc
};

struct PsArgs {
    const float *targets, *weights;                     // weights: NULL = all 1
    float *normal, *albedo, *confidence;
    int64_t weight_stride;                              // elements between the weight planes of two shots: H W | 0 (one plane for all)
    int32_t height, width, tiles_x, n_shots, iterations;
    int32_t targets_srgb, albedo_srgb;
    float x0, x1, xstep, y0, y1, ystep;                 // torch.linspace(-s/2, s/2, .) per axis, as the render kernels form it
    float shadow_cos, min_condition;
};

// The shot loop: a run-time loop where the shots are read again, an unrolled one under l < L where they are kept (compile-time indices).
template <int CAP, class F> __device__ __forceinline__ void for_shots(int32_t n, F &&f) {
    if constexpr (CAP == 0) {
        for (int32_t l = 0; l < n; ++l) f(l);
    } else {
#pragma unroll
        for (int32_t l = 0; l < CAP; ++l)
            if (l < n) f(l);
    }
}

// Unit vector towards light l and 1 / a_l.
template <int LIGHT>
__device__ __forceinline__ void shot_geometry(const PsLights &tab, int32_t l, float px, float py, float (&w)[3], float &inv_att) {
    if (LIGHT == PBR_LIGHT_POINT) {
        const float dx = tab.light[l][0] - px, dy = tab.light[l][1] - py, dz = tab.light[l][2];          // P = (xs, -ys, 0): py is -ys
        const float dd = fmaf(dz, dz, fmaf(dy, dy, dx * dx));
        const float inv = rcp(sqrt_hw(dd) + 1e-7f);
        w[0] = dx * inv; w[1] = dy * inv; w[2] = dz * inv;
        inv_att = dd + 1e-7f;
    } else {
        w[0] = tab.light[l][0]; w[1] = tab.light[l][1]; w[2] = tab.light[l][2];
        inv_att = 1.0f;
    }
}

template <int V> struct PsPixelState {
    float g[V][3], conf[V];
    uint32_t mask[V];                                   // bit l: shot l is lit under the current solution
    bool valid[V], iterating[V];
};

// One solve: A (a00 a01 a02 a11 a12 a22) and b -> c and g; false = the pixel is invalid.
__device__ __forceinline__ bool solve_normal(const float (&A)[6], const float (&b)[3], float kappa, float (&g)[3], float &c, float &gg) {
    const float t = A[0] + A[3] + A[5];
    const float c00 = fmaf(A[3], A[5], -(A[4] * A[4])), c01 = fmaf(A[2], A[4], -(A[1] * A[5])), c02 = fmaf(A[1], A[4], -(A[2] * A[3]));
    const float c11 = fmaf(A[0], A[5], -(A[2] * A[2])), c12 = fmaf(A[1], A[2], -(A[0] * A[4])), c22 = fmaf(A[0], A[3], -(A[1] * A[1]));
    const float det = fmaf(A[2], c02, fmaf(A[1], c01, A[0] * c00));
    const float t3 = t * (1.0f / 3.0f);
    c = t > 0.0f ? det * rcp(t3 * t3 * t3) : 0.0f;
    if (c < kappa) return false;
    const float inv = rcp(det);
    g[0] = fmaf(c02, b[2], fmaf(c01, b[1], c00 * b[0])) * inv;
    g[1] = fmaf(c12, b[2], fmaf(c11, b[1], c01 * b[0])) * inv;
    g[2] = fmaf(c22, b[2], fmaf(c12, b[1], c02 * b[0])) * inv;
    gg = fmaf(g[2], g[2], fmaf(g[1], g[1], g[0] * g[0]));
    return gg > 0.0f && gg < __builtin_inff() && g[2] > 0.0f;        // (a NaN fails every comparison)
}

template <int LIGHT, int V, int CAP>
__global__ __launch_bounds__(256) void photometric_kernel(PsLights tab, PsArgs a) {
    static_assert(CAP == 0 || V == 1, "the kept shots are one pixel's");
    const int32_t tile_y = (int32_t)blockIdx.x / a.tiles_x, tile_x = (int32_t)blockIdx.x - tile_y * a.tiles_x;
    const int32_t y = tile_y * PS_TILE_ROWS + ((int32_t)threadIdx.x >> PS_TILE_W_LOG2);
    const int32_t x = (tile_x * PS_TILE_LANES_X + ((int32_t)threadIdx.x & (PS_TILE_LANES_X - 1))) * V;
    if (y >= a.height || x >= a.width) return;                                       // (quad form: width % 4 == 0, so x + 3 < width)
    const int64_t plane = (int64_t)a.height * a.width, at = (int64_t)y * a.width + x;
    const int32_t L = a.n_shots;
    float px[V];
#pragma unroll
    for (int p = 0; p < V; ++p) px[p] = LIGHT == PBR_LIGHT_POINT ? linspace_at(a.x0, a.x1, a.xstep, a.width, x + p) : 0.0f;
    const float py = LIGHT == PBR_LIGHT_POINT ? -linspace_at(a.y0, a.y1, a.ystep, a.height, y) : 0.0f;

    // r_lc of the lane's pixels and their weight, from memory: shot l's three target planes and its weight plane
    auto read_shot = [&](int32_t l, float (&r)[3][V], float (&wt)[V]) {
        const float *t = a.targets + (int64_t)l * 3 * plane + at;
#pragma unroll
        for (int c = 0; c < 3; ++c) {
            Span<float, V>::ld(t + c * plane, 0, r[c]);
            const float scale = tab.inv_intensity[l][c];
#pragma unroll
            for (int p = 0; p < V; ++p) r[c][p] = (a.targets_srgb ? srgb_to_linear(r[c][p]) : r[c][p]) * scale;
        }
        if (a.weights) {
            Span<float, V>::ld(a.weights + (int64_t)l * a.weight_stride + at, 0, wt);
        } else {
#pragma unroll
            for (int p = 0; p < V; ++p) wt[p] = 1.0f;
        }
    };
    float kept_r[CAP ? CAP : 1][3], kept_w[CAP ? CAP : 1];                           // (CAP > 0: V == 1)
    if constexpr (CAP != 0) {
        for_shots<CAP>(L, [&](int32_t l) {
            float r[3][V], wt[V];
            read_shot(l, r, wt);
            kept_r[l][0] = r[0][0]; kept_r[l][1] = r[1][0]; kept_r[l][2] = r[2][0]; kept_w[l] = wt[0];
        });
    }
    // shot l as the passes see it: r_lc / a_l still to be applied (the geometry is the pixel's)
    auto shot = [&](int32_t l, float (&r)[3][V], float (&wt)[V]) {
        if constexpr (CAP != 0) {
            r[0][0] = kept_r[l][0]; r[1][0] = kept_r[l][1]; r[2][0] = kept_r[l][2]; wt[0] = kept_w[l];
        } else {
            read_shot(l, r, wt);
        }
    };

    PsPixelState<V> s;
#pragma unroll
    for (int p = 0; p < V; ++p) {
        s.mask[p] = 0xffffffffu; s.valid[p] = true; s.iterating[p] = true; s.conf[p] = 0.0f;
        s.g[p][0] = 0.0f; s.g[p][1] = 0.0f; s.g[p][2] = 1.0f;
    }
    for (int32_t k = 0; k < a.iterations; ++k) {
        bool any = false;
#pragma unroll
        for (int p = 0; p < V; ++p) any = any || s.iterating[p];
        if (!any) break;
        float A[V][6], b[V][3];
#pragma unroll
        for (int p = 0; p < V; ++p) {
#pragma unroll
            for (int q = 0; q < 6; ++q) A[p][q] = 0.0f;
            b[p][0] = b[p][1] = b[p][2] = 0.0f;
        }
        for_shots<CAP>(L, [&](int32_t l) {
            float r[3][V], wt[V];
            shot(l, r, wt);
#pragma unroll
            for (int p = 0; p < V; ++p) {
                float w[3], inv_att;
                shot_geometry<LIGHT>(tab, l, px[p], py, w, inv_att);
                const float yl = ((r[0][p] + r[1][p] + r[2][p]) * inv_att) * (1.0f / 3.0f);
                const bool use = ((s.mask[p] >> l) & 1u) != 0u && wt[p] != 0.0f;      // selected, not multiplied: a NaN target under a zero weight is never read into a sum
                const float u = wt[p], uy = u * yl;
                const float ux = u * w[0], uyy = u * w[1], uz = u * w[2];
                A[p][0] = use ? fmaf(ux, w[0], A[p][0]) : A[p][0];
                A[p][1] = use ? fmaf(ux, w[1], A[p][1]) : A[p][1];
                A[p][2] = use ? fmaf(ux, w[2], A[p][2]) : A[p][2];
                A[p][3] = use ? fmaf(uyy, w[1], A[p][3]) : A[p][3];
                A[p][4] = use ? fmaf(uyy, w[2], A[p][4]) : A[p][4];
                A[p][5] = use ? fmaf(uz, w[2], A[p][5]) : A[p][5];
                b[p][0] = use ? fmaf(uy, w[0], b[p][0]) : b[p][0];
                b[p][1] = use ? fmaf(uy, w[1], b[p][1]) : b[p][1];
                b[p][2] = use ? fmaf(uy, w[2], b[p][2]) : b[p][2];
            }
        });
        const bool last = k == a.iterations - 1;
#pragma unroll
        for (int p = 0; p < V; ++p) {
            if (!s.iterating[p]) continue;
            float g[3], c, gg;
            if (!solve_normal(A[p], b[p], a.min_condition, g, c, gg)) {
                s.valid[p] = false; s.iterating[p] = false;
                continue;
            }
            s.g[p][0] = g[0]; s.g[p][1] = g[1]; s.g[p][2] = g[2]; s.conf[p] = c;
            if (last) continue;
            const float thr = a.shadow_cos * sqrt_hw(gg);
            uint32_t m = 0;
            for_shots<CAP>(L, [&](int32_t l) {
                float w[3], inv_att;
                shot_geometry<LIGHT>(tab, l, px[p], py, w, inv_att);
                m |= (fmaf(w[2], g[2], fmaf(w[1], g[1], w[0] * g[0])) > thr ? 1u : 0u) << l;
            });
            const uint32_t live = L >= 32 ? 0xffffffffu : (1u << L) - 1u;
            s.iterating[p] = ((m ^ s.mask[p]) & live) != 0u;                         // an unchanged mask: the next pass would repeat this one
            s.mask[p] = m;
        }
    }

    float n[V][3], num[V][3], den[V], conf[V];
#pragma unroll
    for (int p = 0; p < V; ++p) {
        const float inv = s.valid[p] ? rsq(fmaf(s.g[p][2], s.g[p][2], fmaf(s.g[p][1], s.g[p][1], s.g[p][0] * s.g[p][0]))) : 0.0f;
        n[p][0] = s.valid[p] ? s.g[p][0] * inv : 0.0f;
        n[p][1] = s.valid[p] ? s.g[p][1] * inv : 0.0f;
        n[p][2] = s.valid[p] ? s.g[p][2] * inv : 1.0f;
        conf[p] = s.valid[p] ? s.conf[p] : 0.0f;
        num[p][0] = num[p][1] = num[p][2] = den[p] = 0.0f;
    }
    for_shots<CAP>(L, [&](int32_t l) {
        float r[3][V], wt[V];
        shot(l, r, wt);
#pragma unroll
        for (int p = 0; p < V; ++p) {
            float w[3], inv_att;
            shot_geometry<LIGHT>(tab, l, px[p], py, w, inv_att);
            const bool use = (!s.valid[p] || ((s.mask[p] >> l) & 1u) != 0u) && wt[p] != 0.0f;
            const float sl = fmaxf(fmaf(w[2], n[p][2], fmaf(w[1], n[p][1], w[0] * n[p][0])), 0.0f);
            const float us = wt[p] * sl, usa = us * inv_att;
            den[p] = use ? fmaf(us, sl, den[p]) : den[p];
#pragma unroll
            for (int c = 0; c < 3; ++c) num[p][c] = use ? fmaf(usa, r[c][p], num[p][c]) : num[p][c];
        }
    });
    float out_n[3][V], out_a[3][V];
#pragma unroll
    for (int p = 0; p < V; ++p) {
        const float scale = kPi * rcp(den[p]);
#pragma unroll
        for (int c = 0; c < 3; ++c) {
            const float lin = den[p] == 0.0f ? 0.0f : clamp01(num[p][c] * scale);
            out_a[c][p] = a.albedo_srgb ? linear_to_srgb_unit(lin) : lin;
            out_n[c][p] = n[p][c];
        }
    }
#pragma unroll
    for (int c = 0; c < 3; ++c) {
        Span<float, V>::st(a.normal + c * plane + at, 0, out_n[c]);
        Span<float, V>::st(a.albedo + c * plane + at, 0, out_a[c]);
    }
    Span<float, V>::st(a.confidence + at, 0, conf);
}

template <int LIGHT>
void launch_photometric(const PsLights &tab, const PsArgs &a, bool quads, int64_t tiles, hipStream_t s) {
    const dim3 grid((uint32_t)tiles);
    if (PS_CACHE != 0) quads = false;
    with_width(quads, [&](auto w) {
        constexpr int V = decltype(w)::value;
        constexpr int CAP = V == 1 ? PS_CACHE : 0;
        hipLaunchKernelGGL((photometric_kernel<LIGHT, V, CAP>), grid, dim3(256), 0, s, tab, a);
    });
}

}  // namespace
}  // namespace pbr

extern "C" int pbr_photometric_stereo(const float *targets, const float *weights, int32_t weights_shared, int32_t n_shots, int32_t height,
                                      int32_t width, const float *lights, const float *intensities, int32_t light_type, float light_size,
                                      int32_t targets_srgb, int32_t iterations, float shadow_cos, float min_condition, int32_t albedo_srgb,
                                      float *normal, float *albedo, float *confidence, void *stream) {
    using namespace pbr;
    if (!targets || !lights || !intensities || !normal || !albedo || !confidence) return PBR_ERR_NULL_MAP;
    if (n_shots < 1 || n_shots > PBR_MAX_PHOTOMETRIC_SHOTS) return PBR_ERR_SHAPE;
    if (height < 1 || width < 1 || height > (1 << 30) || width > (1 << 30)) return PBR_ERR_SHAPE;        // (lane x, y stay int32)
    if ((int64_t)height * width > ((int64_t)1 << 40)) return PBR_ERR_SHAPE;
    if (iterations < 1 || iterations > 4) return PBR_ERR_SHAPE;
    if (!(shadow_cos >= 0.0f && shadow_cos < 1.0f) || !(min_condition > 0.0f && min_condition < 1.0f)) return PBR_ERR_SHAPE;   // (a NaN fails)
    if (light_type != PBR_LIGHT_POINT && light_type != PBR_LIGHT_DIRECTIONAL) return PBR_ERR_SHAPE;
    if (light_type == PBR_LIGHT_POINT && !std::isfinite(light_size)) return PBR_ERR_SHAPE;
    PsLights tab = {};
    for (int32_t l = 0; l < n_shots; ++l) {
        for (int c = 0; c < 3; ++c) {
            const float v = lights[3 * l + c], i = intensities[3 * l + c];
            if (!std::isfinite(v) || !std::isfinite(i) || !(i > 0.0f)) return PBR_ERR_SHAPE;
            tab.light[l][c] = v;
            tab.inv_intensity[l][c] = (float)(1.0 / (double)i);
        }
        if (light_type == PBR_LIGHT_DIRECTIONAL) {                                  // F.normalize: v / max(|v|, 1e-12), in double
            const double vx = lights[3 * l], vy = lights[3 * l + 1], vz = lights[3 * l + 2];
            const double norm = std::fmax(std::sqrt(vx * vx + vy * vy + vz * vz), 1e-12);
            tab.light[l][0] = (float)(vx / norm); tab.light[l][1] = (float)(vy / norm); tab.light[l][2] = (float)(vz / norm);
        }
    }
    PsArgs a = {};
    a.targets = targets; a.weights = weights; a.normal = normal; a.albedo = albedo; a.confidence = confidence;
    a.weight_stride = weights_shared ? 0 : (int64_t)height * width;
    a.height = height; a.width = width; a.n_shots = n_shots; a.iterations = iterations;
    a.targets_srgb = targets_srgb != 0; a.albedo_srgb = albedo_srgb != 0;
    // `light_size or 1.0`, and the two-ended linspace of the render kernels (ct_launch.hpp)
    const float size = light_size != 0.0f ? light_size : 1.0f;
    const float lo = (float)(-(double)size / 2), hi = (float)((double)size / 2);
    a.x0 = lo; a.x1 = width > 1 ? hi : lo; a.xstep = width > 1 ? (hi - lo) / (float)(width - 1) : 0.0f;
    a.y0 = lo; a.y1 = height > 1 ? hi : lo; a.ystep = height > 1 ? (hi - lo) / (float)(height - 1) : 0.0f;
    a.shadow_cos = shadow_cos; a.min_condition = min_condition;
    const bool quads = width % 4 == 0 && all_aligned(16, {targets, weights, normal, albedo, confidence});
    const int64_t tiles_x = ((quads && PS_CACHE == 0 ? width / 4 : width) + PS_TILE_LANES_X - 1) / PS_TILE_LANES_X;
    const int64_t tiles = tiles_x * (((int64_t)height + PS_TILE_ROWS - 1) / PS_TILE_ROWS);
    if (tiles > 0x7fffffff) return PBR_ERR_SHAPE;
    a.tiles_x = (int32_t)tiles_x;
    hipStream_t s = static_cast<hipStream_t>(stream);
    if (light_type == PBR_LIGHT_POINT) launch_photometric<PBR_LIGHT_POINT>(tab, a, quads, tiles, s);
    else launch_photometric<PBR_LIGHT_DIRECTIONAL>(tab, a, quads, tiles, s);
    return launch_status();
}
