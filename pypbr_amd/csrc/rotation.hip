// rotation.hip -- the rotation of a material's maps as ONE nearest-neighbour index function per output pixel, forward and backward, over
// all planes of a block of maps in one launch, the rotation of the normal vectors included.
//
// Reference functions replaced (paths under pypbr/):
//   materials/base.py:539-603    MaterialBase.rotate    (pad, torchvision's nearest rotate(expand=True), centre crop, rotate_normals)
//   utils/functions.py:69-108    rotate_normals         (the normal triple: normal_affine.hpp)
//
// The chain pad -> affine grid -> grid_sample(nearest, zeros, align_corners=False) -> centre crop collapses to a closed form
// (DESIGN.md 3.11).  The host computes the constants (pbr_rotate_geom); per output pixel (i, j), in fp32 and in THIS rounding order:
//     x  = j + x0,  y = i + y0                         exact (integers and half-integers)
//     gx = rn(rn(x t00) + rn(y t10))                   both products rounded, then their sum: no fused multiply-add
//     gy = rn(rn(x t01) + rn(y t11))
//     fx = rn(rn(rn(rn(gx + 1) Wp) - 1) / 2)           grid_sample's un-normalisation; fy likewise with Hp
//     ix = rint(fx), iy = rint(fy)                     halves to even
// outside [0, Wp) x [0, Hp): fill (0); else minus `pad`: constant mode fills outside [0, w) x [0, h), circular mode wraps once.
// Layout and launch shape as geometry.hip: [batch][planes][h][w], one lane per quad of four output pixels, the index computed once per
// pixel and reused by every plane.  Reads are scattered along a rotated line and stay scalar; stores are one nontemporal vector per quad
// and plane where the alignment allows.  Values move as bits, except the normal triple, which passes through normal_affine.
#include <hip/hip_runtime.h>

#include <cstdint>

#include "../../include/pbr_hip.h"
#include "launch_util.hpp"
#include "normal_affine.hpp"
#include "plane_quads.hpp"

namespace pbr {
namespace {

struct RotGeom {
    int h, w, H, W, pad, hp, wp;
    float fhp, fwp, x0, y0, t00, t10, t01, t11;
    float cr, sr, cx, cy;                                 // backward: theta's cosine and sine, the padded image's centre
};

// The index function, part 1: output pixel (i, j) -> its nearest texel (ix, iy) of the PADDED image; false outside it.
__device__ __forceinline__ bool rot_padded(const RotGeom &G, int i, int j, int &ix, int &iy) {
    const float x = __fadd_rn((float)j, G.x0), y = __fadd_rn((float)i, G.y0);
    const float gx = __fadd_rn(__fmul_rn(x, G.t00), __fmul_rn(y, G.t10));
    const float gy = __fadd_rn(__fmul_rn(x, G.t01), __fmul_rn(y, G.t11));
    const float fx = __fmul_rn(__fsub_rn(__fmul_rn(__fadd_rn(gx, 1.0f), G.fwp), 1.0f), 0.5f);
    const float fy = __fmul_rn(__fsub_rn(__fmul_rn(__fadd_rn(gy, 1.0f), G.fhp), 1.0f), 0.5f);
    const float rx = rintf(fx), ry = rintf(fy);
    if (!(rx >= 0.0f && rx < G.fwp && ry >= 0.0f && ry < G.fhp)) return false;      // NaN coordinates fill as well
    ix = (int)rx; iy = (int)ry;
    return true;
}

// Part 2: a texel of the padded image -> the element offset sy w + sx inside a source plane, or -1 for fill.
template <bool CIRC> __device__ __forceinline__ int rot_unpad(const RotGeom &G, int ix, int iy) {
    int sx = ix - G.pad, sy = iy - G.pad;
    if (CIRC) { sx = wrap_once(sx, G.w); sy = wrap_once(sy, G.h); }                // pad <= w, h: one wrap
    else if (sx < 0 || sx >= G.w || sy < 0 || sy >= G.h) return -1;
    return sy * G.w + sx;
}

template <bool CIRC> __device__ __forceinline__ int rot_source(const RotGeom &G, int i, int j) {
    int ix, iy;
    return rot_padded(G, i, j, ix, iy) ? rot_unpad<CIRC>(G, ix, iy) : -1;
}

// The value behind an element's bits, for the normal triple.
template <typename U> struct Bits;
template <> struct Bits<uint32_t> {
    static __device__ __forceinline__ float get(uint32_t u) { return __uint_as_float(u); }
    static __device__ __forceinline__ uint32_t put(float f) { return __float_as_uint(f); }
};
template <> struct Bits<uint16_t> {
    static __device__ __forceinline__ float get(uint16_t u) { return (float)__builtin_bit_cast(_Float16, u); }
    static __device__ __forceinline__ uint16_t put(float f) { return __builtin_bit_cast(uint16_t, (_Float16)f); }
};

// ---- forward ------------------------------------------------------------------------------------------------------------------
// VST: the destination's quads are 16-byte (fp16: 8-byte) aligned and rows are whole quads -- one vector store per quad and plane.
template <typename U, bool VST>
__device__ __forceinline__ void store_quad(U *d, const U v[4], uint32_t j0, uint32_t W) {
    typedef typename Quad<U>::v4 v4;
    if (VST) {
        __builtin_nontemporal_store(v4{v[0], v[1], v[2], v[3]}, reinterpret_cast<v4 *>(d));
    } else {
#pragma unroll
        for (int k = 0; k < 4; ++k)
            if (j0 + (uint32_t)k < W) d[k] = v[k];
    }
}

template <typename U, bool VST, bool CIRC>
__global__ __launch_bounds__(256) void rotate_planes_kernel(const U *__restrict__ src, int64_t s_bs, int64_t s_ps, U *__restrict__ dst,
                                                            int64_t d_bs, int64_t d_ps, int planes, RotGeom G, int nfp, Affine M, uint32_t qpr,
                                                            uint32_t quads, uint32_t blocks_per_image) {
    const uint32_t b = blockIdx.x / blocks_per_image;
    const uint32_t q = (blockIdx.x - b * blocks_per_image) * 256u + threadIdx.x;
    if (q >= quads) return;
    const uint32_t i = q / qpr, j0 = (q - i * qpr) * 4u;
    int off[4];
#pragma unroll
    for (int k = 0; k < 4; ++k) off[k] = (VST || j0 + (uint32_t)k < (uint32_t)G.W) ? rot_source<CIRC>(G, (int)i, (int)j0 + k) : -1;
    const U *sp = src + (int64_t)b * s_bs;
    U *dp = dst + (int64_t)b * d_bs + (int64_t)i * G.W + j0;
    int p = 0;
    while (p < planes) {
        if (p == nfp) {                                                            // the normal triple: planes p, p + 1, p + 2 of each pixel
            U vx[4], vy[4], vz[4];
#pragma unroll
            for (int k = 0; k < 4; ++k) {
                float x = 0.0f, y = 0.0f, z = 0.0f;
                if (off[k] >= 0) {
                    x = Bits<U>::get(sp[p * s_ps + off[k]]);
                    y = Bits<U>::get(sp[(p + 1) * s_ps + off[k]]);
                    z = Bits<U>::get(sp[(p + 2) * s_ps + off[k]]);
                }
                normal_affine(M, x, y, z);                                         // a filled pixel stays 0: 0 / max(0, 1e-12)
                vx[k] = Bits<U>::put(x); vy[k] = Bits<U>::put(y); vz[k] = Bits<U>::put(z);
            }
            store_quad<U, VST>(dp + p * d_ps, vx, j0, (uint32_t)G.W);
            store_quad<U, VST>(dp + (p + 1) * d_ps, vy, j0, (uint32_t)G.W);
            store_quad<U, VST>(dp + (p + 2) * d_ps, vz, j0, (uint32_t)G.W);
            p += 3;
            continue;
        }
        U v[4];
#pragma unroll
        for (int k = 0; k < 4; ++k) v[k] = off[k] >= 0 ? sp[p * s_ps + off[k]] : (U)0;
        store_quad<U, VST>(dp + p * d_ps, v, j0, (uint32_t)G.W);
        ++p;
    }
}

// ---- backward -----------------------------------------------------------------------------------------------------------------
// A gather over SOURCE texels, one lane each.  The texel sits at one place of the padded image in constant mode and, in circular mode,
// at up to three per axis (s + pad + k n for k = -1, 0, 1 inside the padded extent: pad <= n).  Each place's centre goes through the
// rotation itself (theta is orthogonal: its transpose inverts it) to output coordinates; the preimages of the texel's square lie within
// 0.5 (|cos| + |sin|) <= 0.71 pixel of that point per axis, so they are among the 3 x 3 output pixels around the nearest one.  A candidate
// IS a preimage when rot_padded -- the forward's own function -- maps it to this place: forward and backward agree at every tie.  The
// preimages are kept as nine bits per place; the planes then sum grad_out in a fixed order: places ascending (row, then column), inside
// a place output rows ascending, then columns.  No atomics, no workspace; every element of grad_src is written.
template <bool CIRC>
__global__ __launch_bounds__(256) void rotate_planes_backward_kernel(const float *__restrict__ go, int64_t g_bs, int64_t g_ps,
                                                                     float *__restrict__ gs, int64_t i_bs, int64_t i_ps,
                                                                     const float *__restrict__ src, int64_t s_bs, int64_t s_ps, int planes,
                                                                     RotGeom G, int nfp, Affine M, uint32_t texels, uint32_t blocks_per_image) {
    constexpr int NP = CIRC ? 3 : 1;
    const uint32_t b = blockIdx.x / blocks_per_image;
    const uint32_t t = (blockIdx.x - b * blocks_per_image) * 256u + threadIdx.x;
    if (t >= texels) return;
    const int sy = (int)(t / (uint32_t)G.w), sx = (int)t - sy * G.w;
    int base[NP * NP];                                                             // offset of the candidate window's first pixel
    uint32_t hit[NP * NP];                                                         // bit 3 di + dj: candidate (i0 + di, j0 + dj) is a preimage
#pragma unroll
    for (int ky = 0; ky < NP; ++ky) {
#pragma unroll
        for (int kx = 0; kx < NP; ++kx) {
            const int py = sy + G.pad + (CIRC ? (ky - 1) * G.h : 0), px = sx + G.pad + (CIRC ? (kx - 1) * G.w : 0);
            uint32_t m = 0;
            int i0 = 0, j0 = 0;
            if (py >= 0 && py < G.hp && px >= 0 && px < G.wp) {
                const float u = (float)px - G.cx, v = (float)py - G.cy;
                i0 = (int)rintf(fmaf(G.sr, u, G.cr * v) - G.y0) - 1;
                j0 = (int)rintf(fmaf(G.cr, u, -(G.sr * v)) - G.x0) - 1;
#pragma unroll
                for (int di = 0; di < 3; ++di) {
#pragma unroll
                    for (int dj = 0; dj < 3; ++dj) {
                        const int i = i0 + di, j = j0 + dj;
                        int ix, iy;
                        if (i >= 0 && i < G.H && j >= 0 && j < G.W && rot_padded(G, i, j, ix, iy) && ix == px && iy == py) m |= 1u << (3 * di + dj);
                    }
                }
            }
            hit[ky * NP + kx] = m;
            base[ky * NP + kx] = i0 * G.W + j0;
        }
    }
    auto gather = [&](const float *plane) {
        float acc = 0.0f;
#pragma unroll
        for (int n = 0; n < NP * NP; ++n) {
            uint32_t m = hit[n];
            while (m) {
                const int bit = __builtin_ctz(m);
                m &= m - 1u;
                const int di = bit / 3, dj = bit - 3 * di;
                acc += plane[base[n] + di * G.W + dj];
            }
        }
        return acc;
    };
    const float *gp = go + (int64_t)b * g_bs;
    float *ip = gs + (int64_t)b * i_bs + t;
    int p = 0;
    while (p < planes) {
        if (p == nfp) {                                                            // every preimage shares the texel's normal: sum first, adjoint once
            float gx = gather(gp + p * g_ps), gy = gather(gp + (p + 1) * g_ps), gz = gather(gp + (p + 2) * g_ps);
            const float *n = src + (int64_t)b * s_bs + t;
            normal_affine_backward(M, n[p * s_ps], n[(p + 1) * s_ps], n[(p + 2) * s_ps], gx, gy, gz);
            ip[p * i_ps] = gx; ip[(p + 1) * i_ps] = gy; ip[(p + 2) * i_ps] = gz;
            p += 3;
            continue;
        }
        ip[p * i_ps] = gather(gp + p * g_ps);
        ++p;
    }
}

// What both entry points check before anything is launched; fills G.
int rotate_arguments(int64_t a_bs, int64_t a_ps, int64_t w_bs, int64_t w_ps, int32_t batch, int32_t planes, int32_t h, int32_t w, int32_t H,
                     int32_t W, const pbr_rotate_geom *g, int32_t nfp, RotGeom &G) {
    if (!g) return PBR_ERR_NULL_MAP;
    if (batch < 1 || planes < 1 || planes > 32 || h < 1 || w < 1 || H < 1 || W < 1) return PBR_ERR_SHAPE;
    if (a_bs < 0 || a_ps < 0 || w_bs < 0 || w_ps < 0) return PBR_ERR_SHAPE;
    if ((batch > 1 && w_bs == 0) || (planes > 1 && w_ps == 0)) return PBR_ERR_SHAPE;     // the written side: images / planes on top of each other
    if (nfp != -1 && (nfp < 0 || nfp + 3 > planes)) return PBR_ERR_SHAPE;
    if (g->pad < 0 || g->pad > (1 << 24)) return PBR_ERR_SHAPE;
    if (g->circular && (g->pad > h || g->pad > w)) return PBR_ERR_SHAPE;                 // one wrap must do
    const int64_t hp = (int64_t)h + 2 * (int64_t)g->pad, wp = (int64_t)w + 2 * (int64_t)g->pad;
    if (hp > (1 << 24) || wp > (1 << 24) || H > (1 << 24) || W > (1 << 24)) return PBR_ERR_SHAPE;    // coordinates are exact in fp32
    if ((int64_t)h * w > 0x7fffffff || (int64_t)H * W > 0x7fffffff) return PBR_ERR_SHAPE;            // in-plane offsets are 32-bit
    G = {h, w, H, W, g->pad, (int)hp, (int)wp, (float)hp, (float)wp, g->x0, g->y0, g->t00, g->t10, g->t01, g->t11,
         g->cos_r, g->sin_r, 0.5f * (float)wp - 0.5f, 0.5f * (float)hp - 0.5f};
    return PBR_OK;
}

}  // namespace
}  // namespace pbr

extern "C" {

int pbr_rotate_planes(const void *src, int64_t src_batch_stride, int64_t src_plane_stride, void *dst, int64_t dst_batch_stride,
                      int64_t dst_plane_stride, int32_t batch, int32_t planes, int32_t h_src, int32_t w_src, int32_t h_out, int32_t w_out,
                      const pbr_rotate_geom *geom, int32_t normal_first_plane, float m00, float m01, float m10, float m11, int dtype,
                      void *stream) {
    using namespace pbr;
    if (!src || !dst) return PBR_ERR_NULL_MAP;
    RotGeom G;
    const int rc = rotate_arguments(src_batch_stride, src_plane_stride, dst_batch_stride, dst_plane_stride, batch, planes, h_src, w_src, h_out,
                                    w_out, geom, normal_first_plane, G);
    if (rc != PBR_OK) return rc;
    if (dtype != PBR_F32 && dtype != PBR_F16) return PBR_ERR_DTYPE;
    uint32_t qpr, quads, per_image, blocks;
    if (!quad_grid(batch, h_out, w_out, qpr, quads, per_image, blocks)) return PBR_ERR_SHAPE;
    const size_t esz = elem_bytes(dtype);
    const bool vst = w_out % 4 == 0 && is_aligned(dst, 4 * esz) && dst_batch_stride % 4 == 0 && dst_plane_stride % 4 == 0;
    const Affine M = make_affine(m00, m01, m10, m11, 1);
    const bool circ = geom->circular != 0;
    hipStream_t s = static_cast<hipStream_t>(stream);
#define PBR_ROTATE(U, VST, CIRC) hipLaunchKernelGGL((rotate_planes_kernel<U, VST, CIRC>), dim3(blocks), dim3(256), 0, s, static_cast<const U *>(src), \
                                                    src_batch_stride, src_plane_stride, static_cast<U *>(dst), dst_batch_stride, dst_plane_stride, \
                                                    (int)planes, G, (int)normal_first_plane, M, qpr, quads, per_image)
#define PBR_ROTATE_U(U) do { if (vst) { if (circ) PBR_ROTATE(U, true, true); else PBR_ROTATE(U, true, false); } \
                             else { if (circ) PBR_ROTATE(U, false, true); else PBR_ROTATE(U, false, false); } } while (0)
    if (dtype == PBR_F32) PBR_ROTATE_U(uint32_t); else PBR_ROTATE_U(uint16_t);
#undef PBR_ROTATE_U
#undef PBR_ROTATE
    return launch_status();
}

int pbr_rotate_planes_backward(const void *grad_out, int64_t grad_out_batch_stride, int64_t grad_out_plane_stride, void *grad_src,
                               int64_t grad_src_batch_stride, int64_t grad_src_plane_stride, const void *src, int64_t src_batch_stride,
                               int64_t src_plane_stride, int32_t batch, int32_t planes, int32_t h_src, int32_t w_src, int32_t h_out,
                               int32_t w_out, const pbr_rotate_geom *geom, int32_t normal_first_plane, float m00, float m01, float m10,
                               float m11, void *stream) {
    using namespace pbr;
    if (!grad_out || !grad_src || (normal_first_plane >= 0 && !src)) return PBR_ERR_NULL_MAP;
    RotGeom G;
    const int rc = rotate_arguments(grad_out_batch_stride, grad_out_plane_stride, grad_src_batch_stride, grad_src_plane_stride, batch, planes,
                                    h_src, w_src, h_out, w_out, geom, normal_first_plane, G);
    if (rc != PBR_OK) return rc;
    if (src_batch_stride < 0 || src_plane_stride < 0) return PBR_ERR_SHAPE;
    const int64_t texels = (int64_t)h_src * w_src, bpi = (texels + 255) / 256, blocks = bpi * batch;
    if (blocks > 0x7fffffff) return PBR_ERR_SHAPE;
    const Affine M = make_affine(m00, m01, m10, m11, 1);
    hipStream_t s = static_cast<hipStream_t>(stream);
#define PBR_ROTATE_BWD(CIRC) hipLaunchKernelGGL((rotate_planes_backward_kernel<CIRC>), dim3((uint32_t)blocks), dim3(256), 0, s, \
                                                static_cast<const float *>(grad_out), grad_out_batch_stride, grad_out_plane_stride, \
                                                static_cast<float *>(grad_src), grad_src_batch_stride, grad_src_plane_stride, \
                                                static_cast<const float *>(src), src_batch_stride, src_plane_stride, (int)planes, G, \
                                                (int)normal_first_plane, M, (uint32_t)texels, (uint32_t)bpi)
    if (geom->circular) PBR_ROTATE_BWD(true); else PBR_ROTATE_BWD(false);
#undef PBR_ROTATE_BWD
    return launch_status();
}

}  // extern "C"
