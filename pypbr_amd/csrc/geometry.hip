// geometry.hip -- the geometric material transforms of the reference as ONE index map per axis, forward and backward, over all planes of a
// block of maps in one launch.
//
// Reference functions replaced (paths under pypbr/):
//   materials/base.py:506-522   MaterialBase.crop            (in-bounds crops: a slice)
//   materials/base.py:524-537   MaterialBase.tile            (map.repeat(1, n, n))
//   materials/base.py:605-639   MaterialBase.flip_horizontal / flip_vertical   (flip, and the normal map's x / y plane negated)
//   materials/base.py:641-655   MaterialBase.roll            (torch.roll over (1, 2))
//   transforms/transforms.py:33-56   Compose over a run of them: the chain folds into one map
//
// Per axis src(i) = (offset + step i) mod N for i in [0, L), step = +-1; L < N is a crop, L > N a tile.  Each plane carries a sign.
// Layout: [batch][planes][h][w]; rows dense, batch and plane strides free (elements, 64-bit).  One lane owns a quad of 4 consecutive
// pixels of a row and walks the planes; quads are numbered row by row, so a wave covers 256 contiguous pixels of a row (or several short
// rows).  A quad whose four source pixels are one contiguous span is ONE load (reversed in registers when step = -1); a quad that
// straddles the wrap point or the end of a ragged row goes pixel by pixel.  Source spans start wherever the offset puts them: they are
// read through vector types of ELEMENT alignment (a misaligned float4* would be undefined behaviour).  Values are moved as bits: a
// negated plane has its sign bit flipped, nothing is converted or rounded.
#include <hip/hip_runtime.h>

#include <cstdint>

#include "../../include/pbr_hip.h"
#include "launch_util.hpp"
#include "plane_quads.hpp"

namespace pbr {
namespace {

struct Axes { int hs, ws, ho, wo, oy, sy, ox, sx; };

// v a few steps outside [0, n) (a quad's pixels on an axis shorter than the quad)
__device__ __forceinline__ int wrap_near(int v, int n) {
    while (v < 0) v += n;
    while (v >= n) v -= n;
    return v;
}

// ---- forward ------------------------------------------------------------------------------------------------------------------
// VST: the destination's quads are 16-byte (fp16: 8-byte) aligned and rows are whole quads -- one vector store per quad and plane.
template <typename U, bool VST>
__global__ __launch_bounds__(256) void remap_planes_kernel(const U *__restrict__ src, int64_t s_bs, int64_t s_ps, U *__restrict__ dst,
                                                           int64_t d_bs, int64_t d_ps, int planes, Axes A, uint32_t neg, uint32_t qpr,
                                                           uint32_t quads, uint32_t blocks_per_image) {
    typedef typename Quad<U>::v4 v4;
    typedef typename Quad<U>::v4e v4e;
    const uint32_t b = blockIdx.x / blocks_per_image;
    const uint32_t q = (blockIdx.x - b * blocks_per_image) * 256u + threadIdx.x;
    if (q >= quads) return;
    const uint32_t y = q / qpr, x0 = (q - y * qpr) * 4u;
    const int ry = wrap_once(A.oy + A.sy * (int)(y % (uint32_t)A.hs), A.hs);
    const int c0 = wrap_once(A.ox + A.sx * (int)(x0 % (uint32_t)A.ws), A.ws);
    const U *sp = src + (int64_t)b * s_bs + (int64_t)ry * A.ws;
    U *dp = dst + (int64_t)b * d_bs + (int64_t)y * A.wo + x0;
    const bool full = VST || x0 + 3u < (uint32_t)A.wo;
    const bool span = full && (A.sx > 0 ? c0 + 3 < A.ws : c0 >= 3);
    if (span) {
        const U *lo = sp + (A.sx > 0 ? c0 : c0 - 3);
#pragma unroll 3
        for (int p = 0; p < planes; ++p) {
            v4 v = *reinterpret_cast<const v4e *>(lo + p * s_ps);
            if (A.sx < 0) v = v4{v.w, v.z, v.y, v.x};
            if ((neg >> p) & 1u) v ^= Quad<U>::sign;
            if (VST) {
                __builtin_nontemporal_store(v, reinterpret_cast<v4 *>(dp + p * d_ps));
            } else {
                U *d = dp + p * d_ps;
                d[0] = v.x; d[1] = v.y; d[2] = v.z; d[3] = v.w;
            }
        }
    } else {
        int c[4];
#pragma unroll
        for (int j = 0; j < 4; ++j) c[j] = wrap_near(c0 + A.sx * j, A.ws);
        for (int p = 0; p < planes; ++p) {
            const U flip = ((neg >> p) & 1u) ? Quad<U>::sign : (U)0;
#pragma unroll
            for (int j = 0; j < 4; ++j)
                if (x0 + (uint32_t)j < (uint32_t)A.wo) dp[p * d_ps + j] = sp[p * s_ps + c[j]] ^ flip;
        }
    }
}

// ---- backward -----------------------------------------------------------------------------------------------------------------
// A gather over SOURCE quads: source pixel (py, px) sums grad_out at rows iy0 + ky hs < ho, columns ix0 + kx ws < wo (rows outer,
// columns inner, ascending), iy0 = sy (py - oy) mod hs, ix0 = sx (px - ox) mod ws.  0 where a crop left no preimage.
template <bool VST>
__global__ __launch_bounds__(256) void remap_planes_backward_kernel(const float *__restrict__ go, int64_t g_bs, int64_t g_ps,
                                                                    float *__restrict__ gs, int64_t i_bs, int64_t i_ps, int planes, Axes A,
                                                                    uint32_t neg, uint32_t qpr, uint32_t quads, uint32_t blocks_per_image) {
    const uint32_t b = blockIdx.x / blocks_per_image;
    const uint32_t q = (blockIdx.x - b * blocks_per_image) * 256u + threadIdx.x;
    if (q >= quads) return;
    const uint32_t py = q / qpr, px0 = (q - py * qpr) * 4u;
    const int iy0 = wrap_once(A.sy * ((int)py - A.oy), A.hs);
    const int ix0 = wrap_once(A.sx * ((int)px0 - A.ox), A.ws);
    const float *gp = go + (int64_t)b * g_bs;
    float *ip = gs + (int64_t)b * i_bs + (int64_t)py * A.ws + px0;
    const bool full = VST || px0 + 3u < (uint32_t)A.ws;
    const bool span = full && (A.sx > 0 ? ix0 + 3 < A.ws : ix0 >= 3);
    int c[4];
#pragma unroll
    for (int j = 0; j < 4; ++j) c[j] = wrap_near(ix0 + A.sx * j, A.ws);
    const int lo = A.sx > 0 ? ix0 : ix0 - 3;                              // span: the quad's lowest first-preimage column
    for (int p = 0; p < planes; ++p) {
        float acc[4] = {0.0f, 0.0f, 0.0f, 0.0f};
        for (int64_t iy = iy0; iy < A.ho; iy += A.hs) {
            const float *row = gp + p * g_ps + iy * A.wo;
            if (span) {
                for (int64_t base = lo; base < A.wo; base += A.ws) {
                    if (base + 3 < A.wo) {
                        const f4 v = *reinterpret_cast<const f4e *>(row + base);
                        if (A.sx > 0) { acc[0] += v.x; acc[1] += v.y; acc[2] += v.z; acc[3] += v.w; }
                        else { acc[0] += v.w; acc[1] += v.z; acc[2] += v.y; acc[3] += v.x; }
                    } else {                                              // the output row ends inside the span
#pragma unroll
                        for (int j = 0; j < 4; ++j) {
                            const int64_t ix = base + (c[j] - lo);
                            if (ix < A.wo) acc[j] += row[ix];
                        }
                    }
                }
            } else {
#pragma unroll
                for (int j = 0; j < 4; ++j)
                    if (px0 + (uint32_t)j < (uint32_t)A.ws)
                        for (int64_t ix = c[j]; ix < A.wo; ix += A.ws) acc[j] += row[ix];
            }
        }
        if ((neg >> p) & 1u) {
#pragma unroll
            for (int j = 0; j < 4; ++j) acc[j] = -acc[j];
        }
        float *d = ip + p * i_ps;
        if (VST) {
            __builtin_nontemporal_store(f4{acc[0], acc[1], acc[2], acc[3]}, reinterpret_cast<f4 *>(d));
        } else {
#pragma unroll
            for (int j = 0; j < 4; ++j)
                if (px0 + (uint32_t)j < (uint32_t)A.ws) d[j] = acc[j];
        }
    }
}

// What both entry points check before anything is launched.
int remap_arguments(int64_t a_bs, int64_t a_ps, int64_t w_bs, int64_t w_ps, int32_t batch, int32_t planes, int32_t h_src, int32_t w_src,
                    int32_t h_out, int32_t w_out, int32_t y_offset, int32_t y_step, int32_t x_offset, int32_t x_step) {
    if (batch < 1 || planes < 1 || planes > 32 || h_src < 1 || w_src < 1 || h_out < 1 || w_out < 1) return PBR_ERR_SHAPE;
    if (a_bs < 0 || a_ps < 0 || w_bs < 0 || w_ps < 0) return PBR_ERR_SHAPE;
    if ((batch > 1 && w_bs == 0) || (planes > 1 && w_ps == 0)) return PBR_ERR_SHAPE;     // the written side: images / planes on top of each other
    if (y_offset < 0 || y_offset >= h_src || x_offset < 0 || x_offset >= w_src) return PBR_ERR_SHAPE;
    if ((y_step != 1 && y_step != -1) || (x_step != 1 && x_step != -1)) return PBR_ERR_SHAPE;
    return PBR_OK;
}

}  // namespace
}  // namespace pbr

extern "C" {

int pbr_remap_planes(const void *src, int64_t src_batch_stride, int64_t src_plane_stride, void *dst, int64_t dst_batch_stride,
                     int64_t dst_plane_stride, int32_t batch, int32_t planes, int32_t h_src, int32_t w_src, int32_t h_out, int32_t w_out,
                     int32_t y_offset, int32_t y_step, int32_t x_offset, int32_t x_step, uint32_t negate_mask, int dtype, void *stream) {
    using namespace pbr;
    if (!src || !dst) return PBR_ERR_NULL_MAP;
    const int rc = remap_arguments(src_batch_stride, src_plane_stride, dst_batch_stride, dst_plane_stride, batch, planes, h_src, w_src, h_out,
                                   w_out, y_offset, y_step, x_offset, x_step);
    if (rc != PBR_OK) return rc;
    if (dtype != PBR_F32 && dtype != PBR_F16) return PBR_ERR_DTYPE;
    uint32_t qpr, quads, per_image, blocks;
    if (!quad_grid(batch, h_out, w_out, qpr, quads, per_image, blocks)) return PBR_ERR_SHAPE;
    const size_t esz = elem_bytes(dtype);
    const bool vst = w_out % 4 == 0 && is_aligned(dst, 4 * esz) && dst_batch_stride % 4 == 0 && dst_plane_stride % 4 == 0;
    const Axes A = {h_src, w_src, h_out, w_out, y_offset, y_step, x_offset, x_step};
    hipStream_t s = static_cast<hipStream_t>(stream);
#define PBR_REMAP(U, VST) hipLaunchKernelGGL((remap_planes_kernel<U, VST>), dim3(blocks), dim3(256), 0, s, static_cast<const U *>(src), \
                                             src_batch_stride, src_plane_stride, static_cast<U *>(dst), dst_batch_stride, dst_plane_stride, \
                                             (int)planes, A, negate_mask, qpr, quads, per_image)
    if (dtype == PBR_F32) { if (vst) PBR_REMAP(uint32_t, true); else PBR_REMAP(uint32_t, false); }
    else { if (vst) PBR_REMAP(uint16_t, true); else PBR_REMAP(uint16_t, false); }
#undef PBR_REMAP
    return launch_status();
}

int pbr_remap_planes_backward(const void *grad_out, int64_t grad_out_batch_stride, int64_t grad_out_plane_stride, void *grad_src,
                              int64_t grad_src_batch_stride, int64_t grad_src_plane_stride, int32_t batch, int32_t planes, int32_t h_src,
                              int32_t w_src, int32_t h_out, int32_t w_out, int32_t y_offset, int32_t y_step, int32_t x_offset,
                              int32_t x_step, uint32_t negate_mask, void *stream) {
    using namespace pbr;
    if (!grad_out || !grad_src) return PBR_ERR_NULL_MAP;
    const int rc = remap_arguments(grad_out_batch_stride, grad_out_plane_stride, grad_src_batch_stride, grad_src_plane_stride, batch, planes,
                                   h_src, w_src, h_out, w_out, y_offset, y_step, x_offset, x_step);
    if (rc != PBR_OK) return rc;
    uint32_t qpr, quads, per_image, blocks;
    if (!quad_grid(batch, h_src, w_src, qpr, quads, per_image, blocks)) return PBR_ERR_SHAPE;
    const bool vst = w_src % 4 == 0 && is_aligned(grad_src, 16) && grad_src_batch_stride % 4 == 0 && grad_src_plane_stride % 4 == 0;
    const Axes A = {h_src, w_src, h_out, w_out, y_offset, y_step, x_offset, x_step};
    hipStream_t s = static_cast<hipStream_t>(stream);
    auto g = static_cast<const float *>(grad_out);
    auto gi = static_cast<float *>(grad_src);
#define PBR_REMAP_BWD(VST) hipLaunchKernelGGL((remap_planes_backward_kernel<VST>), dim3(blocks), dim3(256), 0, s, g, grad_out_batch_stride, \
                                              grad_out_plane_stride, gi, grad_src_batch_stride, grad_src_plane_stride, (int)planes, A, \
                                              negate_mask, qpr, quads, per_image)
    if (vst) PBR_REMAP_BWD(true); else PBR_REMAP_BWD(false);
#undef PBR_REMAP_BWD
    return launch_status();
}

}  // extern "C"
