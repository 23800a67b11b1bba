// packing.hip -- packed material tensors: a network's output becomes a material's maps and a material's maps a network's input, each as
// ONE launch over a table of plane operations, forward and backward.
//
// Reference functions replaced (paths under pypbr/):
//   materials/base.py:416-487   MaterialBase.from_tensor   (per map: slice, clone, x 0.5 + 0.5 when is_normalized, z of a 2-channel normal)
//   materials/base.py:223-242   MaterialBase._compute_normal_map_z_component
//   materials/base.py:319-414   MaterialBase.as_tensor     (per map: slice, (t - 0.5) / 0.5 when normalize, torch.cat)
//   materials/base.py:279-291   MaterialBase.normal_rgb    ((n + 1) 0.5)
//
// A launch carries at most 32 operations (pbr_plane_op) as a kernel argument: the table is the same for every lane of a workgroup -- the
// operation is blockIdx.y -- so its fields are scalar loads from the argument segment.  Grid: (groups of 4 pixels / 256, operations, batch).
//   AFFINE      one plane:   dst = src scale + bias.  (1, 0) copies bits; (0.5, 0.5) and (2, -1) round once whether or not the
//               multiply-add is fused (x 0.5 and x 2 are exact), so every result is the reference's.
//   NORMAL_XY   two planes -> three: a = src scale + bias, v = 2 a - 1, s = x^2 + y^2, z = sqrt(max(1 - s, 1e-6)), n = (x, y, z) / max(|.|, 1e-12).
//               Near the unit circle z amplifies the rounding of s by 1 / (2 z): x^2, y^2, their sum and 1 - s are rounded one by one, in
//               the reference's order (__fmul_rn / __fadd_rn: the build's -ffp-contract=on would fuse x * x + y * y), sqrt and the
//               division are IEEE.  A fused s is 2.9e-5 from the reference there, this sequence 1.2e-7.
// Alignment: planes of a packed tensor are H W elements apart, so for odd H W every second plane starts off a 16-byte boundary.  The
// groups of an operation are laid so that its FIRST destination plane is stored in whole vectors: group g covers pixels [4 g - s, 4 g - s + 4)
// with s the elements that plane's base lies past a vector boundary; the first and the last group may be partial (a scalar head and tail).
// Every other plane of the operation is read / written in vectors when its own base has the same phase (a wave-uniform test), else
// through element-aligned vector loads and scalar stores.  Index arithmetic is 64-bit.  No LDS, no atomics, no workspace.
#include <hip/hip_runtime.h>

#include <cstdint>

#include "../../include/pbr_hip.h"
#include "table_launch.hpp"

namespace pbr {
namespace {

struct OpTable { pbr_plane_op op[PBR_MAX_PLANE_OPS]; };

template <typename T> struct Vec4;
template <> struct Vec4<float> {
    typedef float v4 __attribute__((ext_vector_type(4)));
    typedef float v4e __attribute__((ext_vector_type(4), aligned(4)));
};
template <> struct Vec4<_Float16> {
    typedef _Float16 v4 __attribute__((ext_vector_type(4)));
    typedef _Float16 v4e __attribute__((ext_vector_type(4), aligned(2)));
};

// The 4 pixels [i0, i0 + 4) of one lane, of which [lo, hi) exist.
struct Group { int64_t i0; int lo, hi; bool full; };

// Elements `p` lies past a boundary of 4 elements (0 ... 3).
template <typename T> __device__ __forceinline__ int phase_of(const T *p) { return (int)((reinterpret_cast<uintptr_t>(p) / sizeof(T)) & 3u); }

__device__ __forceinline__ bool make_group(int64_t pixels, int s, Group &g) {
    g.i0 = ((int64_t)blockIdx.x * 256 + threadIdx.x) * 4 - s;
    if (g.i0 >= pixels) return false;
    g.lo = g.i0 < 0 ? (int)-g.i0 : 0;
    g.hi = pixels - g.i0 < 4 ? (int)(pixels - g.i0) : 4;
    g.full = g.lo == 0 && g.hi == 4;
    return true;
}

// `vec`: p + i0 is a vector boundary (the plane's phase is the groups').  Pixels that do not exist read as 0.
template <typename T> __device__ __forceinline__ void load4(const T *p, const Group &g, bool vec, float (&v)[4]) {
    if (g.full) {
        typename Vec4<T>::v4 q;
        if (vec) q = *reinterpret_cast<const typename Vec4<T>::v4 *>(p + g.i0);
        else q = *reinterpret_cast<const typename Vec4<T>::v4e *>(p + g.i0);
        v[0] = (float)q.x; v[1] = (float)q.y; v[2] = (float)q.z; v[3] = (float)q.w;
    } else {
#pragma unroll
        for (int j = 0; j < 4; ++j) v[j] = (j >= g.lo && j < g.hi) ? (float)p[g.i0 + j] : 0.0f;
    }
}

template <typename T> __device__ __forceinline__ void store4(T *p, const Group &g, bool vec, const float (&v)[4]) {
    if (g.full && vec) {
        const typename Vec4<T>::v4 q = {(T)v[0], (T)v[1], (T)v[2], (T)v[3]};
        __builtin_nontemporal_store(q, reinterpret_cast<typename Vec4<T>::v4 *>(p + g.i0));
    } else {
#pragma unroll
        for (int j = 0; j < 4; ++j)
            if (j >= g.lo && j < g.hi) p[g.i0 + j] = (T)v[j];
    }
}

// The correctly rounded square root: the compiler's sqrtf expansion (v_sqrt_f32 and a correction step).  __fsqrt_rn is the bare
// v_sqrt_f32 in this toolchain, 1 ulp off on some arguments -- and next to the unit circle an ulp of s is what decides z.
__device__ __forceinline__ float sqrt_ieee(float v) { return __builtin_sqrtf(v); }

// base.py:235-242 for one pixel, from a = the stored value in [0, 1]: every product and sum rounded on its own, in the reference's order.
struct NormalXY { float x, y, z, c, len; };
__device__ __forceinline__ NormalXY normal_xy(float ax, float ay) {
    NormalXY r;
    r.x = __fsub_rn(__fmul_rn(ax, 2.0f), 1.0f);
    r.y = __fsub_rn(__fmul_rn(ay, 2.0f), 1.0f);
    const float s = __fadd_rn(__fmul_rn(r.x, r.x), __fmul_rn(r.y, r.y));
    r.c = __fsub_rn(1.0f, s);                                                      // >= 1e-6: not clamped (torch's clamp passes the gradient)
    r.z = sqrt_ieee(fmaxf(r.c, 1e-6f));
    r.len = sqrt_ieee(__fadd_rn(s, __fmul_rn(r.z, r.z)));                        // F.normalize: (x^2 + y^2) + z^2
    return r;
}

// ---- forward ------------------------------------------------------------------------------------------------------------------
template <typename T> __global__ __launch_bounds__(256) void plane_ops_kernel(OpTable tab, int64_t pixels) {
    const pbr_plane_op &o = tab.op[blockIdx.y];
    const int64_t b = blockIdx.z;
    const T *src = static_cast<const T *>(o.src) + b * o.src_batch_stride;
    T *dst = static_cast<T *>(o.dst) + b * o.dst_batch_stride;
    const int s = phase_of(dst);
    Group g;
    if (!make_group(pixels, s, g)) return;
    if (o.kind == PBR_PLANE_AFFINE) {
        float v[4];
        load4(src, g, phase_of(src) == s, v);
        if (o.scale != 1.0f || o.bias != 0.0f) {
#pragma unroll
            for (int j = 0; j < 4; ++j) v[j] = v[j] * o.scale + o.bias;
        }
        store4(dst, g, true, v);
    } else {
        const T *sy = src + o.src_plane_stride;
        T *d1 = dst + o.dst_plane_stride, *d2 = d1 + o.dst_plane_stride;
        float x[4], y[4], z[4];
        load4(src, g, phase_of(src) == s, x);
        load4(sy, g, phase_of(sy) == s, y);
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const NormalXY n = normal_xy(x[j] * o.scale + o.bias, y[j] * o.scale + o.bias);
            const float d = fmaxf(n.len, 1e-12f);
            x[j] = __fdiv_rn(n.x, d); y[j] = __fdiv_rn(n.y, d); z[j] = __fdiv_rn(n.z, d);
        }
        store4(dst, g, true, x);
        store4(d1, g, phase_of(d1) == s, y);
        store4(d2, g, phase_of(d2) == s, z);
    }
}

// ---- backward -----------------------------------------------------------------------------------------------------------------
// The same table read the other way: o.src = the upstream gradient w.r.t. the forward's destination planes (NULL: zero), o.dst = the
// gradient w.r.t. the forward's source planes (every element written once), o.input = the forward's source (NORMAL_XY).  fp32.
//   AFFINE      g scale
//   NORMAL_XY   g_v = (g - n (n . g)) / |v| (F.normalize's adjoint); where 1 - s >= 1e-6 (torch's clamp passes the gradient there,
//               the bound included) z = sqrt(1 - s) adds -g_v.z x / z, -g_v.z y / z; then x 2 (v = 2 a - 1) and x scale.
__global__ __launch_bounds__(256) void plane_ops_backward_kernel(OpTable tab, int64_t pixels) {
    const pbr_plane_op &o = tab.op[blockIdx.y];
    const int64_t b = blockIdx.z;
    const float *up = o.src ? static_cast<const float *>(o.src) + b * o.src_batch_stride : nullptr;
    float *gi = static_cast<float *>(o.dst) + b * o.dst_batch_stride;
    const int s = phase_of(gi);
    Group g;
    if (!make_group(pixels, s, g)) return;
    if (o.kind == PBR_PLANE_AFFINE) {
        float v[4] = {0.0f, 0.0f, 0.0f, 0.0f};
        if (up) {
            load4(up, g, phase_of(up) == s, v);
#pragma unroll
            for (int j = 0; j < 4; ++j) v[j] *= o.scale;
        }
        store4(gi, g, true, v);
    } else {
        float *gi1 = gi + o.dst_plane_stride;
        float gx[4] = {0.0f, 0.0f, 0.0f, 0.0f}, gy[4] = {0.0f, 0.0f, 0.0f, 0.0f};
        if (up) {
            const float *in = static_cast<const float *>(o.input) + b * o.input_batch_stride, *in1 = in + o.input_plane_stride;
            const float *up1 = up + o.src_plane_stride, *up2 = up1 + o.src_plane_stride;
            float x[4], y[4], gz[4];
            load4(in, g, phase_of(in) == s, x);
            load4(in1, g, phase_of(in1) == s, y);
            load4(up, g, phase_of(up) == s, gx);
            load4(up1, g, phase_of(up1) == s, gy);
            load4(up2, g, phase_of(up2) == s, gz);
            const float back = 2.0f * o.scale;
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                const NormalXY n = normal_xy(x[j] * o.scale + o.bias, y[j] * o.scale + o.bias);
                const float d = fmaxf(n.len, 1e-12f);
                const float nx = n.x / d, ny = n.y / d, nz = n.z / d;
                const float k = nx * gx[j] + ny * gy[j] + nz * gz[j];
                float ax = (gx[j] - nx * k) / d, ay = (gy[j] - ny * k) / d;
                const float az = (gz[j] - nz * k) / d;
                if (n.c >= 1e-6f) {
                    const float w = az / n.z;
                    ax -= w * n.x; ay -= w * n.y;
                }
                gx[j] = ax * back; gy[j] = ay * back;
            }
        }
        store4(gi, g, true, gx);
        store4(gi1, g, phase_of(gi1) == s, gy);
    }
}

// Planes an operation reads / writes.
inline int planes_read(int kind) { return kind == PBR_PLANE_NORMAL_XY ? 2 : 1; }
inline int planes_written(int kind) { return kind == PBR_PLANE_NORMAL_XY ? 3 : 1; }

// [lo, hi): the bytes between the first and the last element of [batch] x [planes] planes of `pixels` elements.
struct Range { uintptr_t lo, hi; };
inline Range range_of(const void *p, int64_t bs, int64_t ps, int32_t batch, int planes, int64_t pixels, size_t esz) {
    const uintptr_t lo = reinterpret_cast<uintptr_t>(p);
    return {lo, lo + (uintptr_t)((batch - 1) * bs + (planes - 1) * ps + pixels) * esz};
}
inline bool overlap(const Range &a, const Range &b) { return a.lo < b.hi && b.lo < a.hi; }

inline bool strides_ok(int64_t bs, int64_t ps, int32_t batch, int planes, bool written) {
    if (bs < 0 || ps < 0) return false;
    return !written || ((batch == 1 || bs > 0) && (planes == 1 || ps > 0));        // written images / planes on top of each other
}

// What both entry points check before anything is launched; the grid of the launch.
int plane_ops_arguments(const pbr_plane_op *ops, int32_t n_ops, int32_t batch, int64_t pixels, int dtype, bool backward, dim3 &grid) {
    if (!ops) return PBR_ERR_NULL_MAP;
    if (n_ops < 1 || n_ops > PBR_MAX_PLANE_OPS || batch < 1 || batch > 65535 || pixels < 1) return PBR_ERR_SHAPE;
    if (dtype != PBR_F32 && (backward || dtype != PBR_F16)) return PBR_ERR_DTYPE;
    const size_t esz = elem_bytes(dtype);
    const int64_t blocks = ((pixels + 3 + 3) / 4 + 255) / 256;                     // groups of a plane shifted by up to 3 elements
    if (blocks > 0x7fffffff) return PBR_ERR_SHAPE;
    for (int32_t i = 0; i < n_ops; ++i) {
        const pbr_plane_op &o = ops[i];
        if (o.kind != PBR_PLANE_AFFINE && o.kind != PBR_PLANE_NORMAL_XY) return PBR_ERR_UNSUPPORTED;
        const bool xy = o.kind == PBR_PLANE_NORMAL_XY;
        // forward: src read, dst written.  backward: src (the upstream gradient, NULL allowed) and input read, dst written.
        const int n_src = backward ? planes_written(o.kind) : planes_read(o.kind), n_dst = backward ? planes_read(o.kind) : planes_written(o.kind);
        if (!o.dst || (!o.src && !backward) || (backward && xy && o.src && !o.input)) return PBR_ERR_NULL_MAP;
        if (!strides_ok(o.src_batch_stride, o.src_plane_stride, batch, n_src, false) || !strides_ok(o.dst_batch_stride, o.dst_plane_stride, batch, n_dst, true))
            return PBR_ERR_SHAPE;
        if (backward && xy && !strides_ok(o.input_batch_stride, o.input_plane_stride, batch, 2, false)) return PBR_ERR_SHAPE;
        if (!is_aligned(o.src, esz) || !is_aligned(o.dst, esz) || (backward && !is_aligned(o.input, esz))) return PBR_ERR_SHAPE;
    }
    for (int32_t i = 0; i < n_ops; ++i) {                                          // nothing that is written may be read by the same launch
        const pbr_plane_op &w = ops[i];
        const Range out = range_of(w.dst, w.dst_batch_stride, w.dst_plane_stride, batch, backward ? planes_read(w.kind) : planes_written(w.kind), pixels, esz);
        for (int32_t j = 0; j < n_ops; ++j) {
            const pbr_plane_op &r = ops[j];
            if (r.src && overlap(out, range_of(r.src, r.src_batch_stride, r.src_plane_stride, batch,
                                               backward ? planes_written(r.kind) : planes_read(r.kind), pixels, esz)))
                return PBR_ERR_SHAPE;
            if (backward && r.kind == PBR_PLANE_NORMAL_XY && r.src &&
                overlap(out, range_of(r.input, r.input_batch_stride, r.input_plane_stride, batch, 2, pixels, esz)))
                return PBR_ERR_SHAPE;
        }
    }
    grid = dim3((uint32_t)blocks, (uint32_t)n_ops, (uint32_t)batch);
    return PBR_OK;
}

}  // namespace
}  // namespace pbr

extern "C" {

int pbr_plane_ops(const pbr_plane_op *ops, int32_t n_ops, int32_t batch, int64_t pixels, int dtype, void *stream) {
    using namespace pbr;
    dim3 grid;
    const int rc = plane_ops_arguments(ops, n_ops, batch, pixels, dtype, false, grid);
    if (rc != PBR_OK) return rc;
    OpTable tab;
    pad_table(tab.op, ops, n_ops);
    hipStream_t s = static_cast<hipStream_t>(stream);
    if (dtype == PBR_F32) hipLaunchKernelGGL((plane_ops_kernel<float>), grid, dim3(256), 0, s, tab, pixels);
    else hipLaunchKernelGGL((plane_ops_kernel<_Float16>), grid, dim3(256), 0, s, tab, pixels);
    return launch_status();
}

int pbr_plane_ops_backward(const pbr_plane_op *ops, int32_t n_ops, int32_t batch, int64_t pixels, int dtype, void *stream) {
    using namespace pbr;
    dim3 grid;
    const int rc = plane_ops_arguments(ops, n_ops, batch, pixels, dtype, true, grid);
    if (rc != PBR_OK) return rc;
    OpTable tab;
    pad_table(tab.op, ops, n_ops);
    hipLaunchKernelGGL(plane_ops_backward_kernel, grid, dim3(256), 0, static_cast<hipStream_t>(stream), tab, pixels);
    return launch_status();
}

}  // extern "C"
