// normal_ops.hip -- the normal-map operations of the reference, with their gradients: height -> normal (a 3x3 stencil) and the
// per-pixel affine transform of a normal's (x, y) followed by an optional renormalisation (rotate, strength, invert).
//
// Reference functions replaced (paths under pypbr/):
//   utils/functions.py:123-177   compute_normal_from_height
//   utils/functions.py:69-108    rotate_normals            (M = R(theta), renormalised)
//   utils/functions.py:111-120   invert_normal             (M = diag(1, -1), not renormalised)
//   materials/base.py:673-729    MaterialBase.invert_normal / adjust_normal_strength (M = f I, renormalised) / compute_normal_from_height
//
// Layout: height [B][1][H][W], normals [B][3][H][W]; rows dense, batch and plane strides free (elements, 64-bit).
// Arithmetic follows the reference's rounding order (IEEE sqrt and division, no v_rsq, no clamps on the stencil path), so a
// NaN height makes exactly the normals NaN that the reference makes NaN.
#include <hip/hip_runtime.h>
#include <hip/hip_fp16.h>

#include <cstdint>

#include "../../include/pbr_hip.h"
#include "normal_affine.hpp"
#include "stream_shape.hpp"

namespace pbr {
namespace {

// (V consecutive elements at an element offset: Span<T, V>, launch_util.hpp -- plain loads, non-temporal stores)
// One row of the height map as a wave sees it: lane l holds the V pixels of unit u (x = u V ... u V + V - 1), lane 0 also the pixel
// left of its unit and lane 63 the pixel right of its unit (the neighbours the other lanes take from their neighbour lane).  Rows
// outside the map, units outside the row and pixels outside the map are 0 (the reference's zero padding).
template <typename T, int V> struct HRow {
    float v[V], el, er;
    __device__ __forceinline__ void load(const void *h, int r, int H, int W, int u, bool live, int lane) {
#pragma unroll
        for (int j = 0; j < V; ++j) v[j] = 0.0f;
        el = 0.0f; er = 0.0f;
        if (r < 0 || r >= H) return;
        const int64_t row = (int64_t)r * W, x0 = (int64_t)u * V;
        if (live) Span<T, V>::ld(h, row + x0, v);
        if (lane == 0 && x0 > 0 && x0 <= W) el = Elem<T>::ld(h, row + x0 - 1);
        if (lane == 63 && x0 + V < W) er = Elem<T>::ld(h, row + x0 + V);
    }
    // h(x - 1) for the unit's first pixel and h(x + V) for its last (all lanes take part in the cross-lane moves)
    __device__ __forceinline__ void sides(int lane, float &left, float &right) const {
        const float from_left = __shfl_up(v[V - 1], 1, 64), from_right = __shfl_down(v[0], 1, 64);
        left = lane == 0 ? el : from_left;
        right = lane == 63 ? er : from_right;
    }
};

// a = -(gx scale), b = -+(gy scale), n = (a, b, 1) / |(a, b, 1)|   (functions.py:146-175; the norm is >= 1, F.normalize's clamp is moot)
__device__ __forceinline__ void stencil_normal(float l, float r, float u, float d, float scale, int directx, float &nx, float &ny, float &nz,
                                               float &len) {
    const float a = -(__fmul_rn(__fsub_rn(l, r), scale));
    const float gys = __fmul_rn(__fsub_rn(u, d), scale);
    const float b = directx ? gys : -gys;
    len = __fsqrt_rn(__fadd_rn(__fadd_rn(__fmul_rn(a, a), __fmul_rn(b, b)), 1.0f));
    nx = __fdiv_rn(a, len); ny = __fdiv_rn(b, len); nz = __fdiv_rn(1.0f, len);
}

// ---- height -> normal, forward ----------------------------------------------------------------------------------------------
// Each wave owns a strip of 64 units (64 V pixels) of one image and walks `rows` rows down it, holding rows y-1, y, y+1 in registers
// (and prefetching y+2): every height value is read once per strip, plus two halo rows per band.  x neighbours come from the
// neighbour lane; lanes 0 and 63 read the one pixel beyond the strip.  Grid: 1-D, block = 4 waves = 4 adjacent strips.
template <typename T, int V>
__global__ __launch_bounds__(256) void normal_from_height_kernel(const void *__restrict__ height, int64_t h_bs, void *__restrict__ normal,
                                                                 int64_t n_bs, int64_t n_ps, int H, int W, int rows, int bands, int strip_groups,
                                                                 float scale, int directx) {
    const int lane = threadIdx.x & 63;
    int64_t blk = blockIdx.x;
    const int sg = (int)(blk % strip_groups); blk /= strip_groups;
    const int band = (int)(blk % bands);
    const int64_t b = blk / bands;
    const int units = W / V, u = (sg * 4 + (int)(threadIdx.x >> 6)) * 64 + lane;
    if ((u - lane) >= units) return;                                   // the whole wave is beyond the row
    const bool live = u < units;
    const int y0 = band * rows, y1 = min(H, y0 + rows);
    const void *h = static_cast<const T *>(height) + b * h_bs;
    T *nb = static_cast<T *>(normal) + b * n_bs;
    HRow<T, V> up, cur, dn, nxt;
    up.load(h, y0 - 1, H, W, u, live, lane);
    cur.load(h, y0, H, W, u, live, lane);
    dn.load(h, y0 + 1, H, W, u, live, lane);
    for (int y = y0; y < y1; ++y) {
        nxt.load(h, y + 2 <= y1 ? y + 2 : -1, H, W, u, live, lane);     // rows y0-1 ... y1 are all the band needs
        float left, right;
        cur.sides(lane, left, right);
        float nx[V], ny[V], nz[V];
#pragma unroll
        for (int j = 0; j < V; ++j) {
            const float l = j == 0 ? left : cur.v[j - 1], r = j == V - 1 ? right : cur.v[j + 1];
            float len;
            stencil_normal(l, r, up.v[j], dn.v[j], scale, directx, nx[j], ny[j], nz[j], len);
        }
        if (live) {
            const int64_t o = (int64_t)y * W + (int64_t)u * V;
            Span<T, V>::st_nt(nb, o, nx);
            Span<T, V>::st_nt(nb, n_ps + o, ny);
            Span<T, V>::st_nt(nb, 2 * n_ps + o, nz);
        }
        up = cur; cur = dn; dn = nxt;
    }
}

// ---- height -> normal, backward ---------------------------------------------------------------------------------------------
// g_v = (g_n - n (n . g_n)) / |v| per pixel (F.normalize's adjoint), then the transposed stencil:
//   g_h(y, x) = s (g_a(y, x-1) - g_a(y, x+1)) + sb s (g_b(y+1, x) - g_b(y-1, x)),  sb = -1 (OpenGL) | +1 (DirectX).
// (g_a, g_b) is formed ONCE per pixel: a wave walks down its strip forming the pair for row r and emitting g_h for row r-1 from the
// three rows it holds; strips overlap by one unit on each side (lanes 0 and 63 form the pair for the neighbour strips' edge units and
// write nothing), so a pair is never needed from another wave.
__device__ __forceinline__ void pair_adjoint(float l, float r, float u, float d, float gx, float gy, float gz, float scale, int directx,
                                             float &ga, float &gb) {
    float nx, ny, nz, len;
    stencil_normal(l, r, u, d, scale, directx, nx, ny, nz, len);
    const float k = fmaf(nz, gz, fmaf(ny, gy, nx * gx));
    ga = (gx - nx * k) / len;
    gb = (gy - ny * k) / len;
}

template <int V>
__global__ __launch_bounds__(256) void normal_from_height_backward_kernel(const float *__restrict__ height, int64_t h_bs,
                                                                          const float *__restrict__ grad_n, int64_t g_bs, int64_t g_ps,
                                                                          float *__restrict__ grad_h, int64_t gh_bs, int H, int W, int rows,
                                                                          int bands, int strip_groups, float scale, int directx) {
    const int lane = threadIdx.x & 63;
    int64_t blk = blockIdx.x;
    const int sg = (int)(blk % strip_groups); blk /= strip_groups;
    const int band = (int)(blk % bands);
    const int64_t b = blk / bands;
    const int units = W / V, u = (sg * 4 + (int)(threadIdx.x >> 6)) * 62 + lane - 1;
    if ((u - lane + 1) >= units) return;                               // the wave's first interior unit is beyond the row
    const bool live = u >= 0 && u < units, writes = live && lane >= 1 && lane <= 62;
    const int y0 = band * rows, y1 = min(H, y0 + rows);
    const float *h = height + b * h_bs, *g = grad_n + b * g_bs;
    float *gh = grad_h + b * gh_bs;
    const float sb = directx ? scale : -scale;
    HRow<float, V> hu, hc, hd, hn;                                     // height rows r-1, r, r+1, r+2
    float ga1[V], gb1[V], gb2[V];                                      // (g_a, g_b) of row r-1, g_b of row r-2
#pragma unroll
    for (int j = 0; j < V; ++j) { ga1[j] = 0.0f; gb1[j] = 0.0f; gb2[j] = 0.0f; }
    hu.load(h, y0 - 2, H, W, u, live, lane);
    hc.load(h, y0 - 1, H, W, u, live, lane);
    hd.load(h, y0, H, W, u, live, lane);
    for (int r = y0 - 1; r <= y1; ++r) {
        hn.load(h, r + 2 <= y1 + 1 ? r + 2 : -1, H, W, u, live, lane);  // the pairs of rows y0-1 ... y1 need rows y0-2 ... y1+1
        float gx[V], gy[V], gz[V];
#pragma unroll
        for (int j = 0; j < V; ++j) { gx[j] = 0.0f; gy[j] = 0.0f; gz[j] = 0.0f; }
        const bool row_in = r >= 0 && r < H;
        if (live && row_in) {
            const int64_t o = (int64_t)r * W + (int64_t)u * V;
            Span<float, V>::ld(g, o, gx);
            Span<float, V>::ld(g, g_ps + o, gy);
            Span<float, V>::ld(g, 2 * g_ps + o, gz);
        }
        float left, right;
        hc.sides(lane, left, right);
        float ga0[V], gb0[V];                                          // the pair of row r
#pragma unroll
        for (int j = 0; j < V; ++j) {
            const float l = j == 0 ? left : hc.v[j - 1], rr = j == V - 1 ? right : hc.v[j + 1];
            pair_adjoint(l, rr, hu.v[j], hd.v[j], gx[j], gy[j], gz[j], scale, directx, ga0[j], gb0[j]);
            if (!(live && row_in)) { ga0[j] = 0.0f; gb0[j] = 0.0f; }
        }
        if (r - 1 >= y0) {                                             // emit row r-1
            const float a_left = __shfl_up(ga1[V - 1], 1, 64), a_right = __shfl_down(ga1[0], 1, 64);
            float out[V];
#pragma unroll
            for (int j = 0; j < V; ++j) {
                const float al = j == 0 ? a_left : ga1[j - 1], ar = j == V - 1 ? a_right : ga1[j + 1];
                out[j] = fmaf(sb, gb0[j] - gb2[j], scale * (al - ar));
            }
            if (writes) Span<float, V>::st_nt(gh, (int64_t)(r - 1) * W + (int64_t)u * V, out);
        }
#pragma unroll
        for (int j = 0; j < V; ++j) { gb2[j] = gb1[j]; gb1[j] = gb0[j]; ga1[j] = ga0[j]; }
        hu = hc; hc = hd; hd = hn;
    }
}

// ---- the affine transform of (x, y), optional renormalisation ---------------------------------------------------------------
// Affine, affine_xy, norm_denominator, normal_affine and normal_affine_backward: normal_affine.hpp (shared with rotation.hip)
template <typename T, int V>
__global__ __launch_bounds__(256) void normal_transform_kernel(const void *src, int64_t s_bs, int64_t s_ps, void *dst, int64_t d_bs,
                                                               int64_t d_ps, int64_t units, int64_t total, Affine M) {
    const int64_t q = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (q >= total) return;
    const int64_t b = q / units, p = (q - b * units) * V;
    const int64_t so = b * s_bs + p, dO = b * d_bs + p;
    float x[V], y[V], z[V];
    Span<T, V>::ld(src, so, x);
    Span<T, V>::ld(src, so + s_ps, y);
    Span<T, V>::ld(src, so + 2 * s_ps, z);
#pragma unroll
    for (int j = 0; j < V; ++j) normal_affine(M, x[j], y[j], z[j]);
    Span<T, V>::st_nt(dst, dO, x);                                         // dst == src: every lane reads its pixels before it writes them
    Span<T, V>::st_nt(dst, dO + d_ps, y);
    Span<T, V>::st_nt(dst, dO + 2 * d_ps, z);
}

// normal_affine_backward per pixel: g_v = renorm ? (g - n (n . g)) / |v|  (g / 1e-12 where the clamp held) : g;  g_xy = M^T g_v_xy, g_z = g_v_z
template <int V>
__global__ __launch_bounds__(256) void normal_transform_backward_kernel(const float *src, int64_t s_bs, int64_t s_ps, const float *grad,
                                                                        int64_t g_bs, int64_t g_ps, float *grad_in, int64_t gi_bs,
                                                                        int64_t gi_ps, int64_t units, int64_t total, Affine M) {
    const int64_t q = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (q >= total) return;
    const int64_t b = q / units, p = (q - b * units) * V;
    const int64_t so = b * s_bs + p, go = b * g_bs + p, io = b * gi_bs + p;
    float x[V], y[V], z[V], gx[V], gy[V], gz[V];
    Span<float, V>::ld(src, so, x);
    Span<float, V>::ld(src, so + s_ps, y);
    Span<float, V>::ld(src, so + 2 * s_ps, z);
    Span<float, V>::ld(grad, go, gx);
    Span<float, V>::ld(grad, go + g_ps, gy);
    Span<float, V>::ld(grad, go + 2 * g_ps, gz);
#pragma unroll
    for (int j = 0; j < V; ++j) normal_affine_backward(M, x[j], y[j], z[j], gx[j], gy[j], gz[j]);
    Span<float, V>::st_nt(grad_in, io, gx);
    Span<float, V>::st_nt(grad_in, io + gi_ps, gy);
    Span<float, V>::st_nt(grad_in, io + 2 * gi_ps, gz);
}

// Rows per wave of the stencil walks: enough waves to fill the chip (about 16 per CU), at least 8 rows so that the two halo rows
// stay a small share of the height reads, at most 64.
int walk_rows(int64_t strips, int64_t batch, int H) {
    const int64_t want = 256 * 16;
    int64_t r = strips * batch * H / want;
    if (r < 8) r = 8;
    if (r > 64) r = 64;
    return (int)r;
}

bool stencil_shape_ok(int32_t batch, int32_t H, int32_t W) { return batch >= 1 && H >= 1 && W >= 1; }

}  // namespace
}  // namespace pbr

extern "C" {

int pbr_normal_from_height(const void *height, int64_t height_batch_stride, void *normal, int64_t normal_batch_stride,
                           int64_t normal_plane_stride, int32_t batch, int32_t height_px, int32_t width, float scale, int32_t directx,
                           int dtype, void *stream) {
    using namespace pbr;
    if (!height || !normal) return PBR_ERR_NULL_MAP;
    if (!stencil_shape_ok(batch, height_px, width) || height_batch_stride < 0 || normal_batch_stride < 0 || normal_plane_stride < 0)
        return PBR_ERR_SHAPE;
    if (dtype != PBR_F32 && dtype != PBR_F16) return PBR_ERR_DTYPE;
    const bool vec = width % 4 == 0 && all_aligned(quad_bytes(dtype), {height, normal}) && height_batch_stride % 4 == 0 &&
                     normal_batch_stride % 4 == 0 && normal_plane_stride % 4 == 0;
    const int V = vec ? 4 : 1, units = width / V;
    const int64_t strips = (units + 63) / 64, groups = (strips + 3) / 4;
    const int rows = walk_rows(strips, batch, height_px), bands = (height_px + rows - 1) / rows;
    const int64_t blocks = groups * bands * (int64_t)batch;
    if (blocks > 0x7fffffff) return PBR_ERR_SHAPE;
    hipStream_t s = static_cast<hipStream_t>(stream);
    with_dtype(dtype, [&](auto t) {
        with_width(vec, [&](auto w) {
            using T = typename decltype(t)::type;
            hipLaunchKernelGGL((normal_from_height_kernel<T, decltype(w)::value>), dim3((unsigned)blocks), dim3(256), 0, s, height, height_batch_stride,
                               normal, normal_batch_stride, normal_plane_stride, (int)height_px, (int)width, rows, bands, (int)groups, scale,
                               (int)(directx != 0));
        });
    });
    return launch_status();
}

int pbr_normal_from_height_backward(const void *height, int64_t height_batch_stride, const void *grad_normal, int64_t grad_batch_stride,
                                    int64_t grad_plane_stride, void *grad_height, int64_t grad_height_batch_stride, int32_t batch,
                                    int32_t height_px, int32_t width, float scale, int32_t directx, void *stream) {
    using namespace pbr;
    if (!height || !grad_normal || !grad_height) return PBR_ERR_NULL_MAP;
    if (!stencil_shape_ok(batch, height_px, width) || height_batch_stride < 0 || grad_batch_stride < 0 || grad_plane_stride < 0 ||
        grad_height_batch_stride < 0)
        return PBR_ERR_SHAPE;
    const bool vec = width % 4 == 0 && all_aligned(16, {height, grad_normal, grad_height}) &&
                     height_batch_stride % 4 == 0 && grad_batch_stride % 4 == 0 && grad_plane_stride % 4 == 0 && grad_height_batch_stride % 4 == 0;
    const int V = vec ? 4 : 1, units = width / V;
    const int64_t strips = (units + 61) / 62, groups = (strips + 3) / 4;
    const int rows = walk_rows(strips, batch, height_px), bands = (height_px + rows - 1) / rows;
    const int64_t blocks = groups * bands * (int64_t)batch;
    if (blocks > 0x7fffffff) return PBR_ERR_SHAPE;
    hipStream_t s = static_cast<hipStream_t>(stream);
    auto h = static_cast<const float *>(height), g = static_cast<const float *>(grad_normal);
    auto gh = static_cast<float *>(grad_height);
    with_width(vec, [&](auto w) {
        hipLaunchKernelGGL((normal_from_height_backward_kernel<decltype(w)::value>), dim3((unsigned)blocks), dim3(256), 0, s, h, height_batch_stride, g,
                           grad_batch_stride, grad_plane_stride, gh, grad_height_batch_stride, (int)height_px, (int)width, rows, bands, (int)groups,
                           scale, (int)(directx != 0));
    });
    return launch_status();
}

int pbr_normal_transform(const void *src, int64_t src_batch_stride, int64_t src_plane_stride, void *dst, int64_t dst_batch_stride,
                         int64_t dst_plane_stride, int32_t batch, int64_t pixels, float m00, float m01, float m10, float m11,
                         int32_t renormalize, int dtype, void *stream) {
    using namespace pbr;
    if (!src || !dst) return PBR_ERR_NULL_MAP;
    if (batch < 1 || pixels < 1 || src_batch_stride < 0 || src_plane_stride < 0 || dst_batch_stride < 0 || dst_plane_stride < 0)
        return PBR_ERR_SHAPE;
    if (dtype != PBR_F32 && dtype != PBR_F16) return PBR_ERR_DTYPE;
    const bool vec = pixels % 4 == 0 && all_aligned(quad_bytes(dtype), {src, dst}) && src_batch_stride % 4 == 0 &&
                     src_plane_stride % 4 == 0 && dst_batch_stride % 4 == 0 && dst_plane_stride % 4 == 0;
    const Affine M = make_affine(m00, m01, m10, m11, renormalize);
    const int64_t units = vec ? pixels / 4 : pixels, total = units * batch;
    const StreamShape sh = stream_shape((size_t)total, {1, 0});
    if ((int64_t)sh.grid * sh.block < total) return PBR_ERR_SHAPE;
    hipStream_t s = static_cast<hipStream_t>(stream);
    with_dtype(dtype, [&](auto t) {
        with_width(vec, [&](auto w) {
            using T = typename decltype(t)::type;
            hipLaunchKernelGGL((normal_transform_kernel<T, decltype(w)::value>), dim3(sh.grid), dim3(sh.block), 0, s, src, src_batch_stride, src_plane_stride,
                               dst, dst_batch_stride, dst_plane_stride, units, total, M);
        });
    });
    return launch_status();
}

int pbr_normal_transform_backward(const void *src, int64_t src_batch_stride, int64_t src_plane_stride, const void *grad_out,
                                  int64_t grad_batch_stride, int64_t grad_plane_stride, void *grad_in, int64_t grad_in_batch_stride,
                                  int64_t grad_in_plane_stride, int32_t batch, int64_t pixels, float m00, float m01, float m10, float m11,
                                  int32_t renormalize, void *stream) {
    using namespace pbr;
    if (!src || !grad_out || !grad_in) return PBR_ERR_NULL_MAP;
    if (batch < 1 || pixels < 1 || src_batch_stride < 0 || src_plane_stride < 0 || grad_batch_stride < 0 || grad_plane_stride < 0 ||
        grad_in_batch_stride < 0 || grad_in_plane_stride < 0)
        return PBR_ERR_SHAPE;
    const bool vec = pixels % 4 == 0 && all_aligned(16, {src, grad_out, grad_in}) && src_batch_stride % 4 == 0 &&
                     src_plane_stride % 4 == 0 && grad_batch_stride % 4 == 0 && grad_plane_stride % 4 == 0 && grad_in_batch_stride % 4 == 0 &&
                     grad_in_plane_stride % 4 == 0;
    const Affine M = make_affine(m00, m01, m10, m11, renormalize);
    const int64_t units = vec ? pixels / 4 : pixels, total = units * batch;
    const StreamShape sh = stream_shape((size_t)total, {1, 0});
    if ((int64_t)sh.grid * sh.block < total) return PBR_ERR_SHAPE;
    hipStream_t s = static_cast<hipStream_t>(stream);
    auto a = static_cast<const float *>(src), g = static_cast<const float *>(grad_out);
    auto gi = static_cast<float *>(grad_in);
    with_width(vec, [&](auto w) {
        hipLaunchKernelGGL((normal_transform_backward_kernel<decltype(w)::value>), dim3(sh.grid), dim3(sh.block), 0, s, a, src_batch_stride, src_plane_stride,
                           g, grad_batch_stride, grad_plane_stride, gi, grad_in_batch_stride, grad_in_plane_stride, units, total, M);
    });
    return launch_status();
}

}  // extern "C"
