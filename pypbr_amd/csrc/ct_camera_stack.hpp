// ct_camera_stack.hpp -- the bodies of the perspective camera's light-stack loss steps over a loss policy (ct_backward.hpp: StackMseLoss,
// WeightedStackMseLoss): a kernel is a body with its policy and `first_targets(p, loss)`, which fills what the policy holds beyond scale and
// targets and issues the first loads behind the texels' -- the arrangement of loss_step (ct_backward.hpp).  The weighted kernels
// (ct_camera_stack_weighted.hip, ct_view_stack_weighted.hip) are built from these.  The unweighted kernels of ct_camera_stack.hip and
// ct_view_stack.hip hold the same statements INLINE and stay that way: called through these functions every one of their 96 instantiations
// comes out with other scalar loads and another schedule (tried three ways; backward_body_to keeps its decode inline for the same reason),
// and their instructions are what the measurements of DESIGN.md 3.19 / 3.20 stand on.  Change the two together.
// Also here: the shots' camera positions as a kernel argument (ViewArgs).  The host side of the steps: ct_stack_host.hpp.
#pragma once
#include "ct_camera.hpp"

namespace pbr {

// ------------------------------------------------------------------ one camera position for all shots
// One-wave workgroups, one pixel group per lane (VEC = 2: a packed pair, for even widths; VEC = 1 otherwise: mse_vec -- no lane sees a pixel
// twice), one partial sum of squared differences per workgroup.  The body is cook_torrance_camera_backward_kernel's MULTI form (bwd_decode ...
// light loop ... bwd_tail) with the stack policy inside the light loop, as backward_body_to has it for the orthographic stack: per
// light the target pixels loaded a light ahead, eval_light, the image's own clamp and encode (loss_colour_adjoint), backprop_light into the
// shared accumulators; the tail and the stores once.  No second pass over the lights: a stack has no summed colour.
// Lanes outside the map shade a clamped position, so that every lane reaches the wave sums; their scale is 0, hence every adjoint they hold
// is exactly 0, and they store nothing and add nothing to the loss.
// PGRAD (the fit step): light l's six sums leave the lane inside the loop (pgrad_add8 -> the workgroup's LDS row of 3 + 6 L floats:
// camera, lights L x 3, intensities L x 3); after the tail the camera's per-pixel Jacobian, then the row goes to b.g_param_partials.  With one
// wave per workgroup the order of the LDS additions is fixed, and the rows are added up in fp64 in a fixed order: deterministic.
template <int LIGHT, int WF, int VEC, typename TM, bool PGRAD, class Loss, class FirstTargets>
__device__ __forceinline__ void camera_stack_step(const KArgs &a, const BArgs &b, const float *__restrict__ targets, float scale,
                                                  float *__restrict__ partials, FirstTargets &&first_targets) {
    static_assert(VEC == 1 || VEC == 2, "one pixel group per lane: the stack policies walk the lights once per lane");
    using R = typename RealOf<VEC, true>::type;
    static_assert(RealOf<VEC, true>::N == 1, "one pixel group per lane");
    constexpr int kParamSlots = 3 + 6 * PBR_MAX_LIGHTS;
    __shared__ float s_param[PGRAD ? kParamSlots : 1];
    const int n_param = 3 + 6 * a.n_lights;
    if constexpr (PGRAD) {
        for (int i = threadIdx.x; i < n_param; i += 64) s_param[i] = 0.0f;      // a 16-light row holds 99 floats: more than the wave has lanes
        __syncthreads();
    }
    const uint32_t tile = tile_of_workgroup(a, blockIdx.x);
    const int ty = (int)a.div_tx.div(tile);
    const LanePos p = lane_pos<VEC, true>(a, (int)tile - ty * a.tiles_x, ty);
    Texels<VEC> t;
    load_texels<WF, TM, VEC, true>(a, a.has_normal != 0, p, t);
    Loss loss;
    loss.sq = 0.0f;
    loss.scale = p.valid ? scale : 0.0f;                                      // a lane outside the map: every adjoint it holds is exactly 0
    loss.plane = a.o_cs;
    loss.lane = targets + ((int64_t)p.b * a.n_lights * 3 * a.o_cs + p.pix);   // 64-bit: B L 3 H W passes 2^31 long before a plane does
    first_targets(p, loss);
    if (!a.has_normal) {
#pragma unroll
        for (int j = 0; j < VEC; ++j) { t.nm[0][j] = 0.0f; t.nm[1][j] = 0.0f; t.nm[2][j] = 1.0f; }
    }
    const Vec3 C = camera_of(a);
    const float ys = linspace_at(a.y0, a.y1, a.ystep, a.H_total, p.y + a.y_offset);
    R xg[1];
    x_grid<R, 1, VEC>(a, p.x, xg);
    const R xs = xg[0];
    R rv;
    const PixelViewT<R> V = pixel_view(C, xs, ys, rv);
    BwdTexelT<R> x;
    bwd_decode<WF, VEC, R>(a, t, 0, V, x);
    const bool srgb = a.out_srgb != 0;
    PixelAdjointT<R> adj;
    adj.clear();
    Vec3T<R> g_view = {splat<R>(0.0f), splat<R>(0.0f), splat<R>(0.0f)};                  // adjoint of the pixel's unit view vector
    const int nl = a.n_lights;
    for (int l = 0; l < nl; ++l) {
        const LightU lu = light_of(a, l);
        const LightGeomT<R> lg = light_geom<LIGHT, R>(lu, V, xs, ys);
        loss.begin_light(l, nl);
        LightEvalT<R> e;
        eval_light(x.pt, lg, lu.inten, e);
        const R tgt[3] = {gather<R>(loss.tgt[0], 0), gather<R>(loss.tgt[1], 0), gather<R>(loss.tgt[2], 0)};
        R g_col[3];
        float sqd[3];
        loss_colour_adjoint(srgb, e.uc, tgt, loss, 0, g_col, sqd);            // THIS image's clamp (backprop_light masks it) and encode
        loss.sq += sqd[0]; loss.sq += sqd[1]; loss.sq += sqd[2];
        LightParamAdjT<R> pa;
        backprop_light<LIGHT, PGRAD>(x.pt, lg, lu.inten, e, g_col, adj, V, pa);
        if constexpr (PGRAD) {
            g_view = {g_view.x + pa.g_V.x, g_view.y + pa.g_V.y, g_view.z + pa.g_V.z};
            float v8[8] = {hsum(pa.g_L.x), hsum(pa.g_L.y), hsum(pa.g_L.z), hsum(pa.g_I[0]), hsum(pa.g_I[1]), hsum(pa.g_I[2]), 0.0f, 0.0f};
            pgrad_add8(v8, 6, s_param + 3 + 3 * l, s_param + 3 + 3 * a.n_lights + 3 * l);
        }
    }
    float ga[3][VEC], gn[3][VEC], gr[VEC], gm[VEC], gs[3][VEC];
    const R gv = bwd_tail<WF, VEC, R>(x, adj, V, 0, ga, gn, gr, gm, gs);
    if constexpr (PGRAD) {
        // v = e / |e|: g_C = (g_v - v (v . g_v)) / |e|, with N.V's direct share gv n in g_v; rv = 1/|e| is pixel_view's v_rsq
        // (cook_torrance_camera_backward_kernel's statements)
        const Vec3T<R> gvw = {fma_(gv, x.pt.n.x, g_view.x), fma_(gv, x.pt.n.y, g_view.y), fma_(gv, x.pt.n.z, g_view.z)};
        const R radial = dotv(gvw, V);
        float v8[8] = {hsum(fma_(-V.x, radial, gvw.x) * rv), hsum(fma_(-V.y, radial, gvw.y) * rv), hsum(fma_(-V.z, radial, gvw.z) * rv),
                       0.0f, 0.0f, 0.0f, 0.0f, 0.0f};
        pgrad_add8(v8, 3, s_param, s_param + 3);
        __syncthreads();
        for (int i = threadIdx.x; i < n_param; i += 64) b.g_param_partials[(int64_t)blockIdx.x * n_param + i] = s_param[i];
    }
    if (p.valid) store_gradients<WF, VEC, TM>(a, b, p, ga, gn, gr, gm, gs);
    const float mine = p.valid ? loss.sq : 0.0f;
    const float total = wave_sum(mine);
    if (threadIdx.x == 0) partials[blockIdx.x] = total;
}

// ------------------------------------------------------------------ one camera position per shot
// The shots' camera positions: kernel arguments, or device memory when `dev` is set.  Device memory is read through the CONSTANT address space
// like the DevParams block (ct_kernel.hpp: dev_params): written by an earlier kernel of the stream, never by this one -- scalar loads.
struct ViewArgs {
    float cam[PBR_MAX_LIGHTS][3];
    uint64_t dev;
};
__device__ __forceinline__ Vec3 camera_at(const ViewArgs &v, int l) {
    if (v.dev) {
        typedef const __attribute__((address_space(4))) float *ConstFloats;
        const ConstFloats p = (ConstFloats)v.dev;
        return Vec3{p[3 * l], p[3 * l + 1], p[3 * l + 2]};
    }
    return Vec3{v.cam[l][0], v.cam[l][1], v.cam[l][2]};
}
// The view that material_terms / bwd_decode / bwd_tail are handed where the real one is per shot: what they form from it is replaced
// (view_terms) or multiplied by an adjoint that is exactly 0 (bwd_tail: g_ndv).
__device__ __forceinline__ Vec3 no_view() { return Vec3{0.0f, 0.0f, 1.0f}; }

// camera_stack_step's frame: one-wave workgroups, one pixel group per lane (mse_vec), one partial sum of squared
// differences per workgroup; lanes outside the map shade a clamped position with scale 0, store nothing and add nothing.
// PGRAD (the fit step): the workgroup's LDS row is 9 L floats, [cameras L x 3 | lights L x 3 | intensities L x 3]; shot l's nine sums leave the
// lane inside the loop (pgrad_add8: the light's six, and the cameras' three of two shots together).  At L = 16 a row holds 144 floats, more
// than the wave has lanes: the zeroing and the copy-out stride.  One wave per workgroup, so the order of the LDS additions is fixed, and the
// rows are added up in fp64 in a fixed order: deterministic.
template <int LIGHT, int WF, int VEC, typename TM, bool PGRAD, class Loss, class FirstTargets>
__device__ __forceinline__ void view_stack_step(const KArgs &a, const BArgs &b, const ViewArgs &va, const float *__restrict__ targets, float scale,
                                                float *__restrict__ partials, FirstTargets &&first_targets) {
    static_assert(VEC == 1 || VEC == 2, "one pixel group per lane: the stack policies walk the lights once per lane");
    using R = typename RealOf<VEC, true>::type;
    static_assert(RealOf<VEC, true>::N == 1, "one pixel group per lane");
    constexpr int kParamSlots = 9 * PBR_MAX_LIGHTS;
    __shared__ float s_param[PGRAD ? kParamSlots : 1];
    const int nl = a.n_lights, n_param = 9 * nl;
    if constexpr (PGRAD) {
        for (int i = threadIdx.x; i < n_param; i += 64) s_param[i] = 0.0f;
        __syncthreads();
    }
    const uint32_t tile = tile_of_workgroup(a, blockIdx.x);
    const int ty = (int)a.div_tx.div(tile);
    const LanePos p = lane_pos<VEC, true>(a, (int)tile - ty * a.tiles_x, ty);
    Texels<VEC> t;
    load_texels<WF, TM, VEC, true>(a, a.has_normal != 0, p, t);
    Loss loss;
    loss.sq = 0.0f;
    loss.scale = p.valid ? scale : 0.0f;                                      // a lane outside the map: every adjoint it holds is exactly 0
    loss.plane = a.o_cs;
    loss.lane = targets + ((int64_t)p.b * a.n_lights * 3 * a.o_cs + p.pix);   // 64-bit: B L 3 H W passes 2^31 long before a plane does
    first_targets(p, loss);
    if (!a.has_normal) {
#pragma unroll
        for (int j = 0; j < VEC; ++j) { t.nm[0][j] = 0.0f; t.nm[1][j] = 0.0f; t.nm[2][j] = 1.0f; }
    }
    const float ys = linspace_at(a.y0, a.y1, a.ystep, a.H_total, p.y + a.y_offset);
    R xg[1];
    x_grid<R, 1, VEC>(a, p.x, xg);
    const R xs = xg[0];
    BwdTexelT<R> x;
    bwd_decode<WF, VEC, R>(a, t, 0, no_view(), x);
    const bool srgb = a.out_srgb != 0;
    PixelAdjointT<R> adj;
    adj.clear();
    float held[3] = {0.0f, 0.0f, 0.0f};                                       // PGRAD: an even shot's camera sums, until the odd shot behind it
    for (int l = 0; l < nl; ++l) {
        const LightU lu = light_of(a, l);
        const Vec3 C = camera_at(va, l);
        R rv;
        const PixelViewT<R> V = pixel_view(C, xs, ys, rv);
        view_terms(x.pt, V);
        const LightGeomT<R> lg = light_geom<LIGHT, R>(lu, V, xs, ys);
        loss.begin_light(l, nl);
        LightEvalT<R> e;
        eval_light(x.pt, lg, lu.inten, e);
        const R tgt[3] = {gather<R>(loss.tgt[0], 0), gather<R>(loss.tgt[1], 0), gather<R>(loss.tgt[2], 0)};
        R g_col[3];
        float sqd[3];
        loss_colour_adjoint(srgb, e.uc, tgt, loss, 0, g_col, sqd);            // THIS image's clamp (backprop_light masks it) and encode
        loss.sq += sqd[0]; loss.sq += sqd[1]; loss.sq += sqd[2];
        LightParamAdjT<R> pa;
        backprop_light<LIGHT, PGRAD>(x.pt, lg, lu.inten, e, g_col, adj, V, pa);
        // N.V is this shot's: its clamp (:163) and its share of the normal's adjoint close here, bwd_tail's statements with this shot's view
        const R gv = masked(in_unit(x.pt.ndv_raw, x.pt.ndv), adj.g_ndv);
        adj.g_ndv = splat<R>(0.0f);
        adj.g_n = {fma_(gv, V.x, adj.g_n.x), fma_(gv, V.y, adj.g_n.y), fma_(gv, V.z, adj.g_n.z)};
        if constexpr (PGRAD) {
            float v8[8] = {hsum(pa.g_L.x), hsum(pa.g_L.y), hsum(pa.g_L.z), hsum(pa.g_I[0]), hsum(pa.g_I[1]), hsum(pa.g_I[2]), 0.0f, 0.0f};
            pgrad_add8(v8, 6, s_param + 3 * nl + 3 * l, s_param + 6 * nl + 3 * l);
            // v = e / |e|: g_C = (g_v - v (v . g_v)) / |e|, with N.V's direct share gv n in g_v; rv = 1/|e| is pixel_view's v_rsq
            const Vec3T<R> gvw = {fma_(gv, x.pt.n.x, pa.g_V.x), fma_(gv, x.pt.n.y, pa.g_V.y), fma_(gv, x.pt.n.z, pa.g_V.z)};
            const R radial = dotv(gvw, V);
            const float mine[3] = {hsum(fma_(-V.x, radial, gvw.x) * rv), hsum(fma_(-V.y, radial, gvw.y) * rv), hsum(fma_(-V.z, radial, gvw.z) * rv)};
            // two shots' cameras share one wave sum: an even shot's three wait in the lane for the odd one behind it (their slots in the
            // row are neighbours); the last shot of an odd count goes alone.  `l` is wave-uniform: no lane takes another way.
            if (l & 1) {
                float c8[8] = {held[0], held[1], held[2], mine[0], mine[1], mine[2], 0.0f, 0.0f};
                pgrad_add8(c8, 6, s_param + 3 * (l - 1), s_param + 3 * l);
            } else if (l + 1 == nl) {
                float c8[8] = {mine[0], mine[1], mine[2], 0.0f, 0.0f, 0.0f, 0.0f, 0.0f};
                pgrad_add8(c8, 3, s_param + 3 * l, s_param);
            } else {
                held[0] = mine[0]; held[1] = mine[1]; held[2] = mine[2];
            }
        }
    }
    float ga[3][VEC], gn[3][VEC], gr[VEC], gm[VEC], gs[3][VEC];
    bwd_tail<WF, VEC, R>(x, adj, no_view(), 0, ga, gn, gr, gm, gs);          // g_ndv is 0: the placeholder view meets a zero adjoint
    if constexpr (PGRAD) {
        __syncthreads();
        for (int i = threadIdx.x; i < n_param; i += 64) b.g_param_partials[(int64_t)blockIdx.x * n_param + i] = s_param[i];
    }
    if (p.valid) store_gradients<WF, VEC, TM>(a, b, p, ga, gn, gr, gm, gs);
    const float mine = p.valid ? loss.sq : 0.0f;
    const float total = wave_sum(mine);
    if (threadIdx.x == 0) partials[blockIdx.x] = total;
}

// Exactly one source of positions: host values (copied into the kernel arguments now) or a device pointer (read when the kernel runs).
static bool one_camera_source(const float *cameras_host, const void *cameras_device) { return (cameras_host != nullptr) != (cameras_device != nullptr); }
static ViewArgs view_args(const pbr_render_desc *d, const float *cameras_host, const void *cameras_device) {
    ViewArgs v;
    std::memset(&v, 0, sizeof(v));
    if (cameras_host) std::memcpy(v.cam, cameras_host, sizeof(float) * 3 * (size_t)d->n_lights);
    v.dev = reinterpret_cast<uint64_t>(cameras_device);
    return v;
}

}  // namespace pbr
