// height_ops.hip -- normal -> height by Poisson reconstruction (the inverse of normal_ops.hip's height -> normal), with its gradient:
// everything of the reference's compute_height_from_normal except the two Fourier transforms, which stay with the FFT library.
//
// Reference functions replaced (paths under pypbr/):
//   utils/functions.py:180-247   compute_height_from_normal (gradient field, mean / min / max normalisation)
//   utils/functions.py:250-283   _compute_divergence
//   utils/functions.py:286-323   _poisson_solver            (the division by the Laplacian's eigenvalues; fft2 / ifft2 are the caller's)
//   materials/base.py:731-751    MaterialBase.compute_height_from_normal
//
// Stages, forward:  normal_divergence -> [rfft2] -> poisson_scale -> [irfft2] -> height_stats -> height_normalize
//          backward: height_normalize_backward -> [rfft2] -> poisson_scale -> [irfft2] -> normal_divergence_backward
// Layout: normals [B][3][H][W], every other map [B][H][W]; rows dense, batch and plane strides free (elements, 64-bit).  The divergence
// follows the reference's rounding order (IEEE division, no fused multiply-add) and is bit-equal to it; the eigenvalues are evaluated
// as -4 (sin^2(pi kx / W) + sin^2(pi ky / H)), which equals the reference's (2 cos(2 pi kx / W) - 2) + (2 cos(2 pi ky / H) - 2) without
// its cancellation at the low frequencies.  The reductions write per-workgroup partials for FIXED pixel ranges and are folded in index
// order (in two fixed levels): no atomics, the same bits on every run, and an image's result does not depend on the batch it is in.
#include <hip/hip_runtime.h>
#include <hip/hip_fp16.h>

#include <cstdint>

#include "../../include/pbr_hip.h"
#include "stream_shape.hpp"

namespace pbr {
namespace {

constexpr float kZEps = 1e-8f;                 // functions.py:211 (n_z + 1e-8) and :240 (range + 1e-8)
constexpr int kTileW = 64, kTileH = 4;         // the stencil kernels: one wave per 64-pixel row segment, 4 rows per workgroup
constexpr int kScaleRows = 16;                 // poisson_scale: rows per workgroup (<= 64: lane l computes the row term of row l)
constexpr int64_t kChunk = 256 * 4 * 12;       // pixels behind one partial of the reductions: 12288 (512^2 -> 22 partials, the last of 4096 px)

// g = (-+n / (n_z + 1e-8)) scale, in the reference's order: negate, divide, scale (functions.py:211-225)
__device__ __forceinline__ float slope(float n, float nz, float scale, bool negate) {
    return __fmul_rn(__fdiv_rn(negate ? -n : n, __fadd_rn(nz, kZEps)), scale);
}

// ---- stage 1: normals -> divergence of the gradient field -------------------------------------------------------------------
// One pixel per lane.  g_x at x + 1 and g_y at y + 1 are recomputed from the neighbour's normal (an L1 hit) instead of passed between
// lanes: the pixel past the last column / row is the last one again (replicate padding), so that difference is g - g = 0 -- or NaN
// where g is infinite, as upstream's.
template <typename T>
__global__ __launch_bounds__(256) void normal_divergence_kernel(const void *__restrict__ normal, int64_t n_bs, int64_t n_ps,
                                                                float *__restrict__ div, int64_t d_bs, int H, int W, int tiles_x, int tiles_y,
                                                                float scale, int directx) {
    int64_t blk = blockIdx.x;
    const int tx = (int)(blk % tiles_x); blk /= tiles_x;
    const int ty = (int)(blk % tiles_y);
    const int64_t b = blk / tiles_y;
    const int x = tx * kTileW + (int)(threadIdx.x & 63), y = ty * kTileH + (int)(threadIdx.x >> 6);
    if (x >= W || y >= H) return;
    const void *n = static_cast<const T *>(normal) + b * n_bs;
    const int64_t i = (int64_t)y * W + x, ir = (int64_t)y * W + min(x + 1, W - 1), id = (int64_t)min(y + 1, H - 1) * W + x;
    const float nz = Elem<T>::ld(n, 2 * n_ps + i);
    const float gx0 = slope(Elem<T>::ld(n, i), nz, scale, true);
    const float gx1 = slope(Elem<T>::ld(n, ir), Elem<T>::ld(n, 2 * n_ps + ir), scale, true);
    const float gy0 = slope(Elem<T>::ld(n, n_ps + i), nz, scale, !directx);
    const float gy1 = slope(Elem<T>::ld(n, n_ps + id), Elem<T>::ld(n, 2 * n_ps + id), scale, !directx);
    div[b * d_bs + i] = __fadd_rn(__fsub_rn(gx1, gx0), __fsub_rn(gy1, gy0));
}

// ---- stage 7: the divergence's adjoint --------------------------------------------------------------------------------------
// a_x(y,x) = dd(y,x-1) [x >= 1] - dd(y,x) [x <= W-2] is the gradient w.r.t. g_x(y,x) (a_y likewise); then the chain rule of
// g = -+n / (n_z + 1e-8) scale.  A gather: every output value is written by the lane that owns it.
__global__ __launch_bounds__(256) void normal_divergence_backward_kernel(const float *__restrict__ normal, int64_t n_bs, int64_t n_ps,
                                                                         const float *__restrict__ dd, int64_t d_bs, float *__restrict__ grad,
                                                                         int64_t g_bs, int64_t g_ps, int H, int W, int tiles_x, int tiles_y,
                                                                         float scale, int directx) {
    int64_t blk = blockIdx.x;
    const int tx = (int)(blk % tiles_x); blk /= tiles_x;
    const int ty = (int)(blk % tiles_y);
    const int64_t b = blk / tiles_y;
    const int x = tx * kTileW + (int)(threadIdx.x & 63), y = ty * kTileH + (int)(threadIdx.x >> 6);
    if (x >= W || y >= H) return;
    const float *n = normal + b * n_bs, *d = dd + b * d_bs;
    float *g = grad + b * g_bs;
    const int64_t i = (int64_t)y * W + x;
    const float d0 = d[i];
    const float ax = (x >= 1 ? d[i - 1] : 0.0f) - (x <= W - 2 ? d0 : 0.0f);
    const float ay = (y >= 1 ? d[i - W] : 0.0f) - (y <= H - 2 ? d0 : 0.0f);
    const float nx = n[i], ny = n[n_ps + i], ze = n[2 * n_ps + i] + kZEps;
    const float sy = directx ? scale : -scale;                                   // g_y = sy n_y / ze
    g[i] = -scale * ax / ze;
    g[g_ps + i] = sy * ay / ze;
    g[2 * g_ps + i] = (scale * (nx * ax) - sy * (ny * ay)) / (ze * ze);
}

// ---- stage 2: the half spectrum over the Laplacian's eigenvalues ---------------------------------------------------------------
// spec [B][H][W/2+1] complex64, in place: both components / den(ky, kx), den = -4 (sin^2(pi kx / W) + sin^2(pi ky' / H)) with
// ky' = min(ky, H - ky) (the same sine, its argument exact near ky = H); the DC bin becomes 0.  A workgroup owns 256 columns of
// kScaleRows rows: the column term is computed once per lane, the row term once per row (by lane r of every wave, read across lanes).
__global__ __launch_bounds__(256) void poisson_scale_kernel(float2 *__restrict__ spec, int64_t s_bs, int H, int W, int Wh, int chunks, int bands) {
    int64_t blk = blockIdx.x;
    const int c = (int)(blk % chunks); blk /= chunks;
    const int band = (int)(blk % bands);
    const int64_t b = blk / bands;
    const int lane = (int)(threadIdx.x & 63), kx = c * 256 + (int)threadIdx.x, y0 = band * kScaleRows;
    const bool live = kx < Wh;                                                   // (no early return: every lane serves the row terms)
    const int ky = lane < kScaleRows && y0 + lane < H ? y0 + lane : 0;           // only lanes 0 ... kScaleRows - 1 are read back below; the others take ky = 0
    const float sr = sinpif((float)min(ky, H - ky) / (float)H), row_term = __fmul_rn(sr, sr);
    const float sc = sinpif((float)(live ? kx : 0) / (float)W), col_term = __fmul_rn(sc, sc);       // kx <= W / 2
    float2 *p = spec + b * s_bs + (int64_t)y0 * Wh + kx;                         // (formed by every lane, dereferenced by live ones only)
#pragma unroll
    for (int r = 0; r < kScaleRows; ++r) {
        const float den = __fmul_rn(-4.0f, __fadd_rn(col_term, __shfl(row_term, r, 64)));
        if (live && y0 + r < H) {
            float2 v = p[(int64_t)r * Wh];
            if (kx == 0 && y0 + r == 0) { v.x = 0.0f; v.y = 0.0f; }
            else { v.x = __fdiv_rn(v.x, den); v.y = __fdiv_rn(v.y, den); }
            p[(int64_t)r * Wh] = v;
        }
    }
}

// ---- the reductions ------------------------------------------------------------------------------------------------------------
// Partial p of image b covers the pixels [p kChunk, min(n, (p + 1) kChunk)) of that image, whatever the batch or the device.
struct HeightPartial { double sum; float mn, mx; int32_t imin, imax; };           // 24 bytes
struct GradPartial { double sg, sgo; };                                           // 16 bytes: sum G, sum G out

// the smaller value, the lower index among equal values (a NaN never wins: the sum carries it)
__device__ __forceinline__ void take_min(float &v, int32_t &i, float ov, int32_t oi) { if (ov < v || (ov == v && oi < i)) { v = ov; i = oi; } }
__device__ __forceinline__ void take_max(float &v, int32_t &i, float ov, int32_t oi) { if (ov > v || (ov == v && oi < i)) { v = ov; i = oi; } }

__device__ __forceinline__ int64_t lesser(int64_t a, int64_t b) { return a < b ? a : b; }

// (V consecutive elements at an element offset: Span<T, V>, launch_util.hpp -- plain loads and plain stores here)

// stage 3: sum (fp64), min, max and the first index of each, per partial.  A lane visits its pixels in rising order and the tree
// joins lanes by (value, index), so the index is the first one's; the tree's shape is fixed, so is the sum's rounding.
template <int V>
__global__ __launch_bounds__(256) void height_stats_kernel(const float *__restrict__ h, int64_t h_bs, HeightPartial *__restrict__ ws, int64_t n,
                                                           int P) {
    const int p = (int)(blockIdx.x % P), t = (int)threadIdx.x;
    const int64_t b = blockIdx.x / P;
    const float *img = h + b * h_bs;
    const int64_t lo = (int64_t)p * kChunk, hi = lesser(n, lo + kChunk);
    double sum = 0.0;
    float mn = INFINITY, mx = -INFINITY;
    int32_t imin = INT32_MAX, imax = INT32_MAX;
    for (int64_t i = lo + (int64_t)t * V; i < hi; i += 256 * V) {                // V == 4: n % 4 == 0, so a unit is whole
        float v[V];
        Span<float, V>::ld(img, i, v);
#pragma unroll
        for (int j = 0; j < V; ++j) {
            sum += (double)v[j];
            if (v[j] < mn) { mn = v[j]; imin = (int32_t)(i + j); }
            if (v[j] > mx) { mx = v[j]; imax = (int32_t)(i + j); }
        }
    }
    __shared__ double s_sum[256];
    __shared__ float s_mn[256], s_mx[256];
    __shared__ int32_t s_imin[256], s_imax[256];
    s_sum[t] = sum; s_mn[t] = mn; s_mx[t] = mx; s_imin[t] = imin; s_imax[t] = imax;
    __syncthreads();
    for (int off = 128; off > 0; off >>= 1) {
        if (t < off) {
            s_sum[t] += s_sum[t + off];
            take_min(s_mn[t], s_imin[t], s_mn[t + off], s_imin[t + off]);
            take_max(s_mx[t], s_imax[t], s_mx[t + off], s_imax[t + off]);
        }
        __syncthreads();
    }
    if (t == 0) ws[b * P + p] = {s_sum[0], s_mn[0], s_mx[0], s_imin[0], s_imax[0]};
}

// The fold of an image's P partials, by the first wave of a workgroup, in index order on two fixed levels: lane l folds the
// consecutive partials [l k, (l + 1) k), k = ceil(P / 64), one after the other, then lane 0 folds the 64 lane results in lane order.
// Min, max and their first indices are exactly those of a one-by-one fold; the sum's association is fixed by P alone, so every
// workgroup of the image -- and every run, in any batch -- gets the same bits.  (One lane folding all P one by one waits for P
// dependent loads: 108 us instead of 50 for the 4096^2 normalisation, profiles/EXPERIMENTS.md.)
struct HeightFold { double sum; float mn, mx; int32_t imin, imax; };
__device__ __forceinline__ void fold_height_partials(const HeightPartial *w, int P, int t, HeightFold *lanes) {
    if (t < 64) {
        const int k = (P + 63) / 64, p0 = t * k, p1 = p0 + k < P ? p0 + k : P;
        HeightFold f = {0.0, INFINITY, -INFINITY, INT32_MAX, INT32_MAX};
        for (int p = p0; p < p1; ++p) {
            f.sum += w[p].sum;
            take_min(f.mn, f.imin, w[p].mn, w[p].imin);
            take_max(f.mx, f.imax, w[p].mx, w[p].imax);
        }
        lanes[t] = f;
    }
    __syncthreads();
    if (t == 0) {
        HeightFold f = lanes[0];
        for (int l = 1; l < 64; ++l) {
            f.sum += lanes[l].sum;
            take_min(f.mn, f.imin, lanes[l].mn, lanes[l].imin);
            take_max(f.mx, f.imax, lanes[l].mx, lanes[l].imax);
        }
        lanes[0] = f;
    }
    __syncthreads();
}

// stage 4: fold the image's partials (every workgroup: the same sequence, so the same bits, in each), then
//   out = ((h - mean) - mn) / ((mx - mn) + 1e-8),  mn = fl(min h - mean), mx = fl(max h - mean)        (functions.py:234-242)
// and stats[b] = {mean, mn, range, argmin, argmax} (the two indices as int32 bit patterns) for the backward.
template <typename T, int V>
__global__ __launch_bounds__(256) void height_normalize_kernel(const float *__restrict__ h, int64_t h_bs, const HeightPartial *__restrict__ ws,
                                                               void *__restrict__ out, int64_t o_bs, float *__restrict__ stats, int64_t n, int P,
                                                               int spans, int64_t span) {
    const int sp = (int)(blockIdx.x % spans), t = (int)threadIdx.x;
    const int64_t b = blockIdx.x / spans;
    __shared__ HeightFold s_lanes[64];
    fold_height_partials(ws + b * P, P, t, s_lanes);
    const HeightFold f = s_lanes[0];
    const float mean = (float)(f.sum / (double)n);
    const float lo = __fsub_rn(f.mn, mean), range = __fadd_rn(__fsub_rn(__fsub_rn(f.mx, mean), lo), kZEps);
    if (sp == 0 && t == 0) {
        float *st = stats + b * 5;
        st[0] = mean; st[1] = lo; st[2] = range; st[3] = __int_as_float(f.imin); st[4] = __int_as_float(f.imax);
    }
    const float *img = h + b * h_bs;
    T *o = static_cast<T *>(out) + b * o_bs;
    const int64_t first = (int64_t)sp * span, last = lesser(n, first + span);
    for (int64_t i = first + (int64_t)t * V; i < last; i += 256 * V) {
        float v[V];
        Span<float, V>::ld(img, i, v);
#pragma unroll
        for (int j = 0; j < V; ++j) v[j] = __fdiv_rn(__fsub_rn(__fsub_rn(v[j], mean), lo), range);
        Span<T, V>::st(o, i, v);
    }
}

// stage 5a: sum G and sum G out per partial (fp64; the products are exact in fp64)
template <int V>
__global__ __launch_bounds__(256) void height_grad_sums_kernel(const float *__restrict__ grad, int64_t g_bs, const float *__restrict__ out,
                                                               int64_t o_bs, GradPartial *__restrict__ ws, int64_t n, int P) {
    const int p = (int)(blockIdx.x % P), t = (int)threadIdx.x;
    const int64_t b = blockIdx.x / P;
    const float *g = grad + b * g_bs, *o = out + b * o_bs;
    const int64_t lo = (int64_t)p * kChunk, hi = lesser(n, lo + kChunk);
    double sg = 0.0, sgo = 0.0;
    for (int64_t i = lo + (int64_t)t * V; i < hi; i += 256 * V) {
        float gv[V], ov[V];
        Span<float, V>::ld(g, i, gv);
        Span<float, V>::ld(o, i, ov);
#pragma unroll
        for (int j = 0; j < V; ++j) { sg += (double)gv[j]; sgo += (double)gv[j] * (double)ov[j]; }
    }
    __shared__ double s_g[256], s_go[256];
    s_g[t] = sg; s_go[t] = sgo;
    __syncthreads();
    for (int off = 128; off > 0; off >>= 1) {
        if (t < off) { s_g[t] += s_g[t + off]; s_go[t] += s_go[t + off]; }
        __syncthreads();
    }
    if (t == 0) ws[b * P + p] = {s_g[0], s_go[0]};
}

// stage 5b: dh = G / r + [i = argmin] (q - s) - [i = argmax] q,  q = sum(G out) / r,  s = sum(G) / r.
// (out = (hc - mn) / r with r = mx - mn + eps: d out_i / d mn = (out_i - 1) / r, d out_i / d mx = -out_i / r; min and max hand their
// gradient to their first index.)  The mean subtraction's adjoint, dh - mean(dh), is NOT applied: sum(dh) = s + (q - s) - q = 0
// identically, and the solve that follows drops the DC bin anyway.
template <int V>
__global__ __launch_bounds__(256) void height_normalize_backward_kernel(const float *__restrict__ grad, int64_t g_bs,
                                                                        const float *__restrict__ stats, const GradPartial *__restrict__ ws,
                                                                        float *__restrict__ dh, int64_t d_bs, int64_t n, int P, int spans,
                                                                        int64_t span) {
    const int sp = (int)(blockIdx.x % spans), t = (int)threadIdx.x;
    const int64_t b = blockIdx.x / spans;
    __shared__ GradPartial s_lanes[64];
    const float range = stats[b * 5 + 2];
    if (t < 64) {                                                                // the two-level fold of fold_height_partials
        const GradPartial *w = ws + b * P;
        const int k = (P + 63) / 64, p0 = t * k, p1 = p0 + k < P ? p0 + k : P;
        GradPartial f = {0.0, 0.0};
        for (int p = p0; p < p1; ++p) { f.sg += w[p].sg; f.sgo += w[p].sgo; }
        s_lanes[t] = f;
    }
    __syncthreads();
    if (t == 0) {
        GradPartial f = s_lanes[0];
        for (int l = 1; l < 64; ++l) { f.sg += s_lanes[l].sg; f.sgo += s_lanes[l].sgo; }
        s_lanes[0] = f;
    }
    __syncthreads();
    const float q = (float)(s_lanes[0].sgo / (double)range), s = (float)(s_lanes[0].sg / (double)range);
    const int64_t imin = __float_as_int(stats[b * 5 + 3]), imax = __float_as_int(stats[b * 5 + 4]);
    const float *g = grad + b * g_bs;
    float *d = dh + b * d_bs;
    const int64_t first = (int64_t)sp * span, last = lesser(n, first + span);
    for (int64_t i = first + (int64_t)t * V; i < last; i += 256 * V) {
        float v[V];
        Span<float, V>::ld(g, i, v);
#pragma unroll
        for (int j = 0; j < V; ++j) {
            float r = v[j] / range;
            if (i + j == imin) r += q - s;
            if (i + j == imax) r -= q;
            v[j] = r;
        }
        Span<float, V>::st(d, i, v);
    }
}

struct Tiles { int x, y; int64_t blocks; };
Tiles stencil_tiles(int32_t batch, int32_t H, int32_t W) {
    const int tx = (W + kTileW - 1) / kTileW, ty = (H + kTileH - 1) / kTileH;
    return {tx, ty, (int64_t)tx * ty * batch};
}

bool map_shape_ok(int32_t batch, int32_t H, int32_t W) { return batch >= 1 && H >= 1 && W >= 1 && (int64_t)H * W <= 0x7fffffff; }
int partials(int64_t n) { return (int)((n + kChunk - 1) / kChunk); }
bool vec4(int64_t n, std::initializer_list<const void *> ptrs, std::initializer_list<int64_t> strides) {
    bool ok = n % 4 == 0 && all_aligned(16, ptrs);
    for (int64_t s : strides) ok = ok && s % 4 == 0;
    return ok;
}

}  // namespace
}  // namespace pbr

extern "C" {

int pbr_normal_divergence(const void *normal, int64_t normal_batch_stride, int64_t normal_plane_stride, void *div, int64_t div_batch_stride,
                          int32_t batch, int32_t height_px, int32_t width, float scale, int32_t directx, int dtype, void *stream) {
    using namespace pbr;
    if (!normal || !div) return PBR_ERR_NULL_MAP;
    if (!map_shape_ok(batch, height_px, width) || normal_batch_stride < 0 || normal_plane_stride < 0 || div_batch_stride < 0) return PBR_ERR_SHAPE;
    if (dtype != PBR_F32 && dtype != PBR_F16) return PBR_ERR_DTYPE;
    const Tiles t = stencil_tiles(batch, height_px, width);
    if (t.blocks > 0x7fffffff) return PBR_ERR_SHAPE;
    hipStream_t s = static_cast<hipStream_t>(stream);
    with_dtype(dtype, [&](auto e) {
        using T = typename decltype(e)::type;
        hipLaunchKernelGGL((normal_divergence_kernel<T>), dim3((unsigned)t.blocks), dim3(256), 0, s, normal, normal_batch_stride, normal_plane_stride,
                           static_cast<float *>(div), div_batch_stride, (int)height_px, (int)width, t.x, t.y, scale, (int)(directx != 0));
    });
    return launch_status();
}

int pbr_normal_divergence_backward(const void *normal, int64_t normal_batch_stride, int64_t normal_plane_stride, const void *grad_div,
                                   int64_t grad_div_batch_stride, void *grad_normal, int64_t grad_batch_stride, int64_t grad_plane_stride,
                                   int32_t batch, int32_t height_px, int32_t width, float scale, int32_t directx, void *stream) {
    using namespace pbr;
    if (!normal || !grad_div || !grad_normal) return PBR_ERR_NULL_MAP;
    if (!map_shape_ok(batch, height_px, width) || normal_batch_stride < 0 || normal_plane_stride < 0 || grad_div_batch_stride < 0 ||
        grad_batch_stride < 0 || grad_plane_stride < 0)
        return PBR_ERR_SHAPE;
    const Tiles t = stencil_tiles(batch, height_px, width);
    if (t.blocks > 0x7fffffff) return PBR_ERR_SHAPE;
    hipLaunchKernelGGL(normal_divergence_backward_kernel, dim3((unsigned)t.blocks), dim3(256), 0, static_cast<hipStream_t>(stream),
                       static_cast<const float *>(normal), normal_batch_stride, normal_plane_stride, static_cast<const float *>(grad_div),
                       grad_div_batch_stride, static_cast<float *>(grad_normal), grad_batch_stride, grad_plane_stride, (int)height_px, (int)width,
                       t.x, t.y, scale, (int)(directx != 0));
    return launch_status();
}

int pbr_poisson_scale(void *spectrum, int64_t spectrum_batch_stride, int32_t batch, int32_t height_px, int32_t width, void *stream) {
    using namespace pbr;
    if (!spectrum) return PBR_ERR_NULL_MAP;
    if (!map_shape_ok(batch, height_px, width) || spectrum_batch_stride < 0 || !is_aligned(spectrum, 8)) return PBR_ERR_SHAPE;
    const int Wh = width / 2 + 1, chunks = (Wh + 255) / 256, bands = (height_px + kScaleRows - 1) / kScaleRows;
    const int64_t blocks = (int64_t)chunks * bands * batch;
    if (blocks > 0x7fffffff) return PBR_ERR_SHAPE;
    hipLaunchKernelGGL(poisson_scale_kernel, dim3((unsigned)blocks), dim3(256), 0, static_cast<hipStream_t>(stream),
                       static_cast<float2 *>(spectrum), spectrum_batch_stride, (int)height_px, (int)width, Wh, chunks, bands);
    return launch_status();
}

size_t pbr_height_workspace_bytes(int32_t batch, int32_t height_px, int32_t width) {
    using namespace pbr;
    if (!map_shape_ok(batch, height_px, width)) return 0;
    return (size_t)batch * partials((int64_t)height_px * width) * sizeof(HeightPartial);
}

int pbr_height_stats(const void *height, int64_t height_batch_stride, void *workspace, int32_t batch, int32_t height_px, int32_t width,
                     void *stream) {
    using namespace pbr;
    if (!height || !workspace) return PBR_ERR_NULL_MAP;
    if (!map_shape_ok(batch, height_px, width) || height_batch_stride < 0 || !is_aligned(workspace, 8)) return PBR_ERR_SHAPE;
    const int64_t n = (int64_t)height_px * width;
    const int P = partials(n);
    if ((int64_t)P * batch > 0x7fffffff) return PBR_ERR_SHAPE;
    const dim3 grid((unsigned)(P * batch));
    hipStream_t s = static_cast<hipStream_t>(stream);
    auto h = static_cast<const float *>(height);
    auto ws = static_cast<HeightPartial *>(workspace);
    with_width(vec4(n, {height}, {height_batch_stride}), [&](auto w) {
        hipLaunchKernelGGL(height_stats_kernel<decltype(w)::value>, grid, dim3(256), 0, s, h, height_batch_stride, ws, n, P);
    });
    return launch_status();
}

int pbr_height_normalize(const void *height, int64_t height_batch_stride, const void *workspace, void *out, int64_t out_batch_stride,
                         void *stats, int32_t batch, int32_t height_px, int32_t width, int dtype, void *stream) {
    using namespace pbr;
    if (!height || !workspace || !out || !stats) return PBR_ERR_NULL_MAP;
    if (!map_shape_ok(batch, height_px, width) || height_batch_stride < 0 || out_batch_stride < 0 || !is_aligned(workspace, 8) ||
        !is_aligned(stats, 4))
        return PBR_ERR_SHAPE;
    if (dtype != PBR_F32 && dtype != PBR_F16) return PBR_ERR_DTYPE;
    const int64_t n = (int64_t)height_px * width;
    const int P = partials(n);
    const bool vec = vec4(n, {height}, {height_batch_stride, out_batch_stride}) && is_aligned(out, quad_bytes(dtype));
    const int64_t span = 256 * (vec ? 4 : 1) * 8, spans = (n + span - 1) / span;
    if (spans * batch > 0x7fffffff) return PBR_ERR_SHAPE;
    const dim3 grid((unsigned)(spans * batch));
    hipStream_t s = static_cast<hipStream_t>(stream);
    auto h = static_cast<const float *>(height);
    auto ws = static_cast<const HeightPartial *>(workspace);
    with_dtype(dtype, [&](auto t) {
        with_width(vec, [&](auto w) {
            using T = typename decltype(t)::type;
            hipLaunchKernelGGL((height_normalize_kernel<T, decltype(w)::value>), grid, dim3(256), 0, s, h, height_batch_stride, ws, out, out_batch_stride,
                               static_cast<float *>(stats), n, P, (int)spans, span);
        });
    });
    return launch_status();
}

int pbr_height_normalize_backward(const void *grad_out, int64_t grad_batch_stride, const void *out, int64_t out_batch_stride, const void *stats,
                                  void *workspace, void *grad_height, int64_t grad_height_batch_stride, int32_t batch, int32_t height_px,
                                  int32_t width, void *stream) {
    using namespace pbr;
    if (!grad_out || !out || !stats || !workspace || !grad_height) return PBR_ERR_NULL_MAP;
    if (!map_shape_ok(batch, height_px, width) || grad_batch_stride < 0 || out_batch_stride < 0 || grad_height_batch_stride < 0 ||
        !is_aligned(workspace, 8) || !is_aligned(stats, 4))
        return PBR_ERR_SHAPE;
    const int64_t n = (int64_t)height_px * width;
    const int P = partials(n);
    const bool vec = vec4(n, {grad_out, out, grad_height}, {grad_batch_stride, out_batch_stride, grad_height_batch_stride});
    const int64_t span = 256 * (vec ? 4 : 1) * 8, spans = (n + span - 1) / span;
    if (spans * batch > 0x7fffffff || (int64_t)P * batch > 0x7fffffff) return PBR_ERR_SHAPE;
    const dim3 sums((unsigned)(P * batch)), grid((unsigned)(spans * batch));
    hipStream_t s = static_cast<hipStream_t>(stream);
    auto g = static_cast<const float *>(grad_out), o = static_cast<const float *>(out), st = static_cast<const float *>(stats);
    auto ws = static_cast<GradPartial *>(workspace);
    auto dh = static_cast<float *>(grad_height);
    with_width(vec, [&](auto w) {
        constexpr int V = decltype(w)::value;
        hipLaunchKernelGGL(height_grad_sums_kernel<V>, sums, dim3(256), 0, s, g, grad_batch_stride, o, out_batch_stride, ws, n, P);
        hipLaunchKernelGGL(height_normalize_backward_kernel<V>, grid, dim3(256), 0, s, g, grad_batch_stride, st, ws, dh, grad_height_batch_stride, n, P,
                           (int)spans, span);
    });
    return launch_status();
}

}  // extern "C"
