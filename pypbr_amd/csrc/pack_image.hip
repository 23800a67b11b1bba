// pack_image.hip -- planar float32 maps -> image samples (uint8 / uint16, dense (H,W,C) as PIL takes them), on the device: the mirror image
// of unpack.hip.
//
// Reference function replaced: /root/reference/pypbr/materials/base.py:793-850 `MaterialBase.to_pil`.  Per map:
//   default modes  torchvision's to_pil_image of the float map: pic.mul(255).byte() -- one fp32 product, rounded, truncated toward zero --
//                  transposed to (H,W,C);
//   16-bit modes   base.py:837: (t * 65535).clip(0, 65535).astype(uint16), in fp32;
//   a normal map   base.py:818 first: (n + 1.0) * 0.5 -- an fp32 sum, rounded, then an fp32 product, rounded -- then the 8-bit rule.
// Every product and sum is rounded on its own (__fmul_rn / __fadd_rn: nothing may merge into an fma).  Where upstream is undefined
// (.byte() of a float outside [0, 255], astype(uint16) of a NaN) this build SATURATES: below 0 -> 0, above the maximum -> the maximum,
// +-inf likewise, NaN -> 0; inside [0, 1] every sample is upstream's bit for bit.
//
// Why on the device: upstream copies every float map to the host whole and runs three host passes per map (mul, byte, transpose).  Here
// the samples are made where the maps are -- ONE launch for all maps of a material, the table of maps a kernel argument, blockIdx.y the
// map -- and a quarter of the bytes (half for 16 bit) travel home.  One HBM-bound pass; no workspace, no atomics, no LDS.
//   dense form    rows dense, width % 4 == 0, plane starts 16-byte aligned, dst dword aligned: a lane takes 4 consecutive pixels, one
//                 float4 load per plane, its 4*C samples assembled in registers into whole dwords -- no sub-dword stores;
//   general form  any non-negative element strides, any extents: one pixel per lane, byte / short stores.
// The form of a map (channels, bits, normal, dense or not) is uniform over a block.
#include <hip/hip_runtime.h>

#include <cstdint>

#include "../../include/pbr_hip.h"
#include "table_launch.hpp"

namespace pbr {
namespace {

struct PackTable {
    pbr_image_pack map[PBR_MAX_IMAGE_PACKS];
    int32_t dense[PBR_MAX_IMAGE_PACKS];       // decided on the host: the map takes the dense form
};

// One sample.  The clamp comes BEFORE the conversion, so that the conversion is defined for every float: fmaxf(NaN, 0) is 0, -0 and
// everything below become 0, everything above `top` (+inf too) becomes `top`.  Inside [0, top] the clamp changes nothing and the
// conversion truncates toward zero, as .byte() and astype(uint16) do.
template <bool NORMAL> __device__ __forceinline__ unsigned to_sample(float v, float top) {
    if (NORMAL) v = __fmul_rn(__fadd_rn(v, 1.0f), 0.5f);                          // base.py:818
    return (unsigned)fminf(fmaxf(__fmul_rn(v, top), 0.0f), top);
}

typedef uint32_t u32x2 __attribute__((ext_vector_type(2), aligned(4)));
typedef uint32_t u32x3 __attribute__((ext_vector_type(3), aligned(4)));
typedef uint32_t u32x4 __attribute__((ext_vector_type(4), aligned(4)));

template <int WORDS> __device__ __forceinline__ void store_words(uint32_t *p, const uint32_t (&w)[WORDS]) {
    if constexpr (WORDS == 1) p[0] = w[0];
    else if constexpr (WORDS == 2) *reinterpret_cast<u32x2 *>(p) = u32x2{w[0], w[1]};
    else if constexpr (WORDS == 3) *reinterpret_cast<u32x3 *>(p) = u32x3{w[0], w[1], w[2]};
    else if constexpr (WORDS == 4) *reinterpret_cast<u32x4 *>(p) = u32x4{w[0], w[1], w[2], w[3]};
    else if constexpr (WORDS == 6) {
        *reinterpret_cast<u32x3 *>(p) = u32x3{w[0], w[1], w[2]};
        *reinterpret_cast<u32x3 *>(p + 3) = u32x3{w[3], w[4], w[5]};
    } else {
        static_assert(WORDS == 8, "4 pixels of 1..4 channels are 1, 2, 3, 4, 6 or 8 dwords");
        *reinterpret_cast<u32x4 *>(p) = u32x4{w[0], w[1], w[2], w[3]};
        *reinterpret_cast<u32x4 *>(p + 4) = u32x4{w[4], w[5], w[6], w[7]};
    }
}

// Dense form: the lane's 4 pixels [4q, 4q + 4) of C planes -> 4*C samples = C (uint8) or 2*C (uint16) dwords at dst + q * WORDS.
template <int BYTES, int C, bool NORMAL> __device__ __forceinline__ void pack_quad(const pbr_image_pack &m, int64_t q) {
    constexpr int WORDS = C * BYTES;
    constexpr float top = BYTES == 1 ? 255.0f : 65535.0f;
    float4 v[C];
#pragma unroll
    for (int c = 0; c < C; ++c) v[c] = *reinterpret_cast<const float4 *>(m.src + (int64_t)c * m.stride_c + 4 * q);
    uint32_t w[WORDS];
#pragma unroll
    for (int k = 0; k < WORDS; ++k) w[k] = 0u;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
#pragma unroll
        for (int c = 0; c < C; ++c) {
            const float f = j == 0 ? v[c].x : j == 1 ? v[c].y : j == 2 ? v[c].z : v[c].w;
            const unsigned s = to_sample<NORMAL>(f, top);
            const int k = j * C + c;                                              // the k-th sample of the lane's 4*C
            if (BYTES == 1) w[k >> 2] |= s << (8 * (k & 3));
            else w[k >> 1] |= s << (16 * (k & 1));
        }
    }
    store_words<WORDS>(static_cast<uint32_t *>(m.dst) + q * WORDS, w);
}

// General form: pixel p = (y, x) of every channel, read through the strides, written as one byte / short per sample.
template <typename U, bool NORMAL> __device__ __forceinline__ void pack_pixel(const pbr_image_pack &m, int64_t p, int32_t width) {
    const float top = sizeof(U) == 1 ? 255.0f : 65535.0f;
    const int64_t y = p / width, x = p - y * width, base = y * m.stride_h + x * m.stride_w;
    U *dst = static_cast<U *>(m.dst) + p * m.channels;
    for (int c = 0; c < m.channels; ++c) dst[c] = (U)to_sample<NORMAL>(m.src[base + c * m.stride_c], top);
}

__global__ __launch_bounds__(256) void pack_images_kernel(PackTable tab, int32_t width, int64_t plane) {
    const pbr_image_pack &m = tab.map[blockIdx.y];
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (tab.dense[blockIdx.y]) {
        if (i >= plane / 4) return;
        if (m.bits == 8) {
            if (m.encode_normal) pack_quad<1, 3, true>(m, i);
            else if (m.channels == 1) pack_quad<1, 1, false>(m, i);
            else if (m.channels == 2) pack_quad<1, 2, false>(m, i);
            else if (m.channels == 3) pack_quad<1, 3, false>(m, i);
            else pack_quad<1, 4, false>(m, i);
        } else {
            if (m.encode_normal) pack_quad<2, 3, true>(m, i);
            else if (m.channels == 1) pack_quad<2, 1, false>(m, i);
            else if (m.channels == 2) pack_quad<2, 2, false>(m, i);
            else if (m.channels == 3) pack_quad<2, 3, false>(m, i);
            else pack_quad<2, 4, false>(m, i);
        }
        return;
    }
    if (i >= plane) return;
    if (m.bits == 8) {
        if (m.encode_normal) pack_pixel<uint8_t, true>(m, i, width);
        else pack_pixel<uint8_t, false>(m, i, width);
    } else {
        if (m.encode_normal) pack_pixel<uint16_t, true>(m, i, width);
        else pack_pixel<uint16_t, false>(m, i, width);
    }
}

inline bool takes_dense_form(const pbr_image_pack &m, int32_t height, int32_t width) {
    return m.stride_w == 1 && (height == 1 || m.stride_h == width) && width % 4 == 0 && is_aligned(m.src, 16) && (m.channels == 1 || m.stride_c % 4 == 0) &&
           is_aligned(m.dst, 4);
}

}  // namespace
}  // namespace pbr

extern "C" int pbr_pack_images(const pbr_image_pack *maps, int32_t n_maps, int32_t height, int32_t width, void *stream) {
    using namespace pbr;
    if (!maps) return PBR_ERR_NULL_MAP;
    if (n_maps < 1 || n_maps > PBR_MAX_IMAGE_PACKS) return PBR_ERR_SHAPE;
    if (height < 1 || width < 1 || (int64_t)height * width > ((int64_t)1 << 40)) return PBR_ERR_SHAPE;
    const int64_t plane = (int64_t)height * width;
    for (int32_t i = 0; i < n_maps; ++i) {
        const pbr_image_pack &m = maps[i];
        if (!m.src || !m.dst) return PBR_ERR_NULL_MAP;
        if (m.bits != 8 && m.bits != 16) return PBR_ERR_DTYPE;
        if (m.channels < 1 || m.channels > 4 || (m.encode_normal && m.channels != 3)) return PBR_ERR_CHANNELS;
        if (m.stride_c < 0 || m.stride_h < 0 || m.stride_w < 0) return PBR_ERR_SHAPE;
        if (!is_aligned(m.src, 4) || (m.bits == 16 && !is_aligned(m.dst, 2))) return PBR_ERR_SHAPE;
    }
    auto dst_end = [&](const pbr_image_pack &m) { return reinterpret_cast<uintptr_t>(m.dst) + (uintptr_t)(plane * m.channels * (m.bits / 8)); };
    for (int32_t i = 0; i < n_maps; ++i)                                            // two maps written on top of each other
        for (int32_t j = i + 1; j < n_maps; ++j)
            if (reinterpret_cast<uintptr_t>(maps[i].dst) < dst_end(maps[j]) && reinterpret_cast<uintptr_t>(maps[j].dst) < dst_end(maps[i]))
                return PBR_ERR_SHAPE;
    PackTable tab;
    bool any_general = false;
    pad_table(tab.map, maps, n_maps);
    for (int32_t i = 0; i < PBR_MAX_IMAGE_PACKS; ++i) {
        tab.dense[i] = takes_dense_form(tab.map[i], height, width) ? 1 : 0;
        any_general = any_general || !tab.dense[i];
    }
    const int64_t blocks = ((any_general ? plane : plane / 4) + 255) / 256;        // a dense map's lanes beyond its quads return at once
    if (blocks > 0x7fffffff) return PBR_ERR_SHAPE;
    hipLaunchKernelGGL(pack_images_kernel, dim3((uint32_t)blocks, (uint32_t)n_maps), dim3(256), 0, static_cast<hipStream_t>(stream), tab, width, plane);
    return launch_status();
}
