// normal_affine.hpp -- the per-pixel affine transform of a normal's (x, y) with its optional renormalisation, forward and adjoint, as the
// device functions shared by normal_ops.hip (pbr_normal_transform and its backward) and rotation.hip (the normal triple of a rotated
// material).  The arithmetic is the reference's rounding order: see normal_ops.hip.
#pragma once
#include <hip/hip_runtime.h>

namespace pbr {

struct Affine { float m00, m01, m10, m11; int diag, renorm; };

inline Affine make_affine(float m00, float m01, float m10, float m11, int renormalize) {
    return {m00, m01, m10, m11, (int)(m01 == 0.0f && m10 == 0.0f), (int)(renormalize != 0)};
}

__device__ __forceinline__ void affine_xy(const Affine &M, float x, float y, float &xo, float &yo) {
    if (M.diag) { xo = M.m00 * x; yo = M.m11 * y; }                   // strength / invert: x f, -y exactly as the reference's in-place ops
    else { xo = fmaf(M.m01, y, M.m00 * x); yo = fmaf(M.m11, y, M.m10 * x); }
}

// F.normalize's denominator: max(|v|, 1e-12); a NaN norm stays NaN
__device__ __forceinline__ float norm_denominator(float x, float y, float z) {
    const float len = __fsqrt_rn(__fadd_rn(__fadd_rn(__fmul_rn(x, x), __fmul_rn(y, y)), __fmul_rn(z, z)));
    return len < 1e-12f ? 1e-12f : len;
}

// (x, y) <- M (x, y), z kept, then F.normalize when M.renorm
__device__ __forceinline__ void normal_affine(const Affine &M, float &x, float &y, float &z) {
    float xo, yo;
    affine_xy(M, x, y, xo, yo);
    x = xo; y = yo;
    if (M.renorm) {
        const float d = norm_denominator(x, y, z);
        x = __fdiv_rn(x, d); y = __fdiv_rn(y, d); z = __fdiv_rn(z, d);
    }
}

// The adjoint at the forward's INPUT (x, y, z): g_v = renorm ? (g - n (n . g)) / |v|  (g / 1e-12 where the clamp held) : g;
// g_xy = M^T g_v_xy, g_z = g_v_z.  (gx, gy, gz) holds the upstream gradient on entry and the result on return.
__device__ __forceinline__ void normal_affine_backward(const Affine &M, float x, float y, float z, float &gx, float &gy, float &gz) {
    float vx, vy, vz = z;
    affine_xy(M, x, y, vx, vy);
    float ax = gx, ay = gy, az = gz;
    if (M.renorm) {
        const float d = norm_denominator(vx, vy, vz);
        if (d > 1e-12f) {
            const float nx = vx / d, ny = vy / d, nz = vz / d;
            const float k = fmaf(nz, az, fmaf(ny, ay, nx * ax));
            ax = (ax - nx * k) / d; ay = (ay - ny * k) / d; az = (az - nz * k) / d;
        } else {
            ax = ax / d; ay = ay / d; az = az / d;
        }
    }
    gx = fmaf(M.m10, ay, M.m00 * ax);
    gy = fmaf(M.m11, ay, M.m01 * ax);
    gz = az;
}

}  // namespace pbr
