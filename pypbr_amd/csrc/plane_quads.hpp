// plane_quads.hpp -- what the kernels that give one lane a quad of four consecutive pixels of a row share (geometry.hip, rotation.hip):
// the element-bit vector types, the single wrap of an index and the 1-D grid over [batch] images of quads.
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>

namespace pbr {

// The bits of one element (uint32_t: fp32, uint16_t: fp16): quads aligned as quads (stores) and as single elements (source spans).
template <typename U> struct Quad;
template <> struct Quad<uint32_t> {
    typedef uint32_t v4 __attribute__((ext_vector_type(4)));
    typedef uint32_t v4e __attribute__((ext_vector_type(4), aligned(4)));
    static constexpr uint32_t sign = 0x80000000u;
};
template <> struct Quad<uint16_t> {
    typedef uint16_t v4 __attribute__((ext_vector_type(4)));
    typedef uint16_t v4e __attribute__((ext_vector_type(4), aligned(2)));
    static constexpr uint16_t sign = 0x8000u;
};
typedef float f4 __attribute__((ext_vector_type(4)));
typedef float f4e __attribute__((ext_vector_type(4), aligned(4)));

// v in (-n, 2 n) -> [0, n)
__device__ __forceinline__ int wrap_once(int v, int n) { return v < 0 ? v + n : (v >= n ? v - n : v); }

// Quads per row, quads per image and workgroups of a launch over [batch] images of h x w; false when the grid would not fit.
inline bool quad_grid(int32_t batch, int32_t h, int32_t w, uint32_t &qpr, uint32_t &quads, uint32_t &per_image, uint32_t &blocks) {
    const int64_t per_row = ((int64_t)w + 3) / 4, total = per_row * h;
    if (total > 0x7fffffff) return false;
    const int64_t bpi = (total + 255) / 256, all = bpi * batch;
    if (all > 0x7fffffff) return false;
    qpr = (uint32_t)per_row; quads = (uint32_t)total; per_image = (uint32_t)bpi; blocks = (uint32_t)all;
    return true;
}

}  // namespace pbr
