// ct_camera.hip -- the perspective camera (C ABI: pbr_cook_torrance_camera, pbr_cook_torrance_camera_backward): the descriptor's view_dir
// is a camera POSITION C in the point light's coordinates, and the view vector of pixel (y, x) is F.normalize(C - P) with
// P = (xs[x], -ys[y], 0) the surface point of the point light's grid (cooktorrance.py:129-136) -- for both light types.  Pixel (y, x) of the
// result is pixel (y, x) of the reference's forward called with view_dir = C - P(y, x).
//
// Same lane frame, texel loads, decode, store policy, workgroup order and plane addressing as the orthographic families (ct_kernel.hpp,
// ct_backward.hpp); what differs is that the view is a PixelViewT<R> per pixel group (brdf_math.hpp) and that nothing of a directional light
// is folded on the host any more (light_geom's PixelViewT overload).  The chain rule is ct_chain_rule.hpp's, over the same view type.
//
// Gradient of the camera position: sum over pixels of (I - v v^T) / |e| g_v with e = C - P, v = e / |e| and g_v the adjoint of the pixel's
// unit view vector (every light's LightParamAdjT::g_V plus the N.V path, gv n).  The Jacobian depends on the pixel, so it is applied per
// pixel BEFORE the sum; the rows' finish (ct_backward.hip: param_grad_finish, view_is_position) leaves vector 0 as summed.
#include "ct_camera.hpp"      // camera_of, camera_gate, nan_grid, camera_args: shared with the light-stack forms (ct_camera_stack.hip)

namespace pbr {

// ------------------------------------------------------------------ forward
//   LIGHT / WF / TI / VEC as cook_torrance_kernel; the result is fp32.  VEC = 4 for widths that 4 divides, else 1.
//   LOOP: the uniform light loop (per-light clamp, sum, clamp: with one light the second clamp changes nothing) in packed pairs -- several
//   lights, fp16 maps and the one-pixel lanes (where R is float either way); !LOOP: one light over fp32 maps, four pixels one by one in
//   plain fp32, the body that streams fastest in the orthographic family (RealOf's comment) and shares its occupancy and store rules.
template <int LIGHT, int WF, typename TI, int VEC, bool LOOP>
__global__ __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu(3, LOOP ? 8 : 3)))
void cook_torrance_camera_kernel(const KArgs a) {
    constexpr bool NT = VEC > 1;
    constexpr bool PACKED = LOOP || sizeof(TI) == 2;
    using R = typename RealOf<VEC, PACKED>::type;
    constexpr int NG = RealOf<VEC, PACKED>::N;
    const uint32_t tile = tile_of_workgroup(a, blockIdx.x);
    const int ty = (int)a.div_tx.div(tile);
    const LanePos p = lane_pos<VEC>(a, (int)tile - ty * a.tiles_x, ty);
    if (!p.valid) return;
    Texels<VEC> t;
    load_texels<WF, TI, VEC, NT>(a, a.has_normal != 0, p, t);
    decode_texels<WF, VEC, PACKED>(a, t);

    const Vec3 C = camera_of(a);
    const float ys = linspace_at(a.y0, a.y1, a.ystep, a.H_total, p.y + a.y_offset);      // the grid is the camera's for both light types
    R xs[NG];
    x_grid<R, NG, VEC>(a, p.x, xs);
    R res[3][NG];
    if constexpr (!LOOP) {
        const LightU lu = light_of(a, 0);
#pragma unroll
        for (int g = 0; g < NG; ++g) {
            R rv;
            const PixelViewT<R> V = pixel_view(C, xs[g], ys, rv);
            PixelTermsT<R> pt;
            material_terms<WF, VEC, R>(t, g, V, pt);
            const LightGeomT<R> lg = light_geom<LIGHT, R>(lu, V, xs[g], ys);
            R col[3];
            shade_light(pt, lg, lu.inten, col);
#pragma unroll
            for (int c = 0; c < 3; ++c) res[c][g] = col[c];
        }
    } else {
        PixelTermsT<R> pt[NG];
        PixelViewT<R> V[NG];
#pragma unroll
        for (int g = 0; g < NG; ++g) {
            R rv;
            V[g] = pixel_view(C, xs[g], ys, rv);
            material_terms<WF, VEC, R>(t, g, V[g], pt[g]);
#pragma unroll
            for (int c = 0; c < 3; ++c) res[c][g] = splat<R>(0.0f);
        }
        for (int l = 0; l < a.n_lights; ++l) {
            const LightU lu = light_of(a, l);
#pragma unroll
            for (int g = 0; g < NG; ++g) {
                const LightGeomT<R> lg = light_geom<LIGHT, R>(lu, V[g], xs[g], ys);
                R col[3];
                shade_light(pt[g], lg, lu.inten, col);
#pragma unroll
                for (int c = 0; c < 3; ++c) res[c][g] += col[c];
            }
        }
#pragma unroll
        for (int c = 0; c < 3; ++c)                                         // sum of per-light clamped terms, clamped
#pragma unroll
            for (int g = 0; g < NG; ++g) res[c][g] = clamp01(res[c][g]);
    }
    if (a.out_srgb) {                                                       // :179-180
#pragma unroll
        for (int c = 0; c < 3; ++c)
#pragma unroll
            for (int g = 0; g < NG; ++g) res[c][g] = linear_to_srgb_unit(res[c][g]);
    }
    constexpr St P = result_store(NT, VEC == 4 && !LOOP && sizeof(TI) == 4);
    with_store_policy<P>(a.st_through != 0, [&](auto policy) {
        constexpr St Q = decltype(policy)::value;
#pragma unroll
        for (int c = 0; c < 3; ++c) {
            float o[VEC];
#pragma unroll
            for (int g = 0; g < NG; ++g) scatter(o, g, res[c][g]);
            if (p.sb) Ld<float, VEC>::template store_at<Q>(a.out, p.b0 * a.o_bs + c * a.o_cs, (uint32_t)p.pix, o);
            else Ld<float, VEC>::template store<Q>(a.out, p.b * a.o_bs + c * a.o_cs + p.pix, o);
        }
    });
}

// ------------------------------------------------------------------ backward
//   One pixel group per lane -- VEC = 2: a packed pair, for even widths; VEC = 1 otherwise -- in one-wave workgroups.  TM: storage type of
//   the maps and of their gradients.  PGRAD: also one row of [camera (3) | lights (L x 3) | intensities (L x 3)] sums per workgroup
//   (b.g_param_partials; NULL: the row stays in LDS).  MULTI: the uniform light loop, for any light count; !MULTI: one light, straight-line
//   -- the loop's carried state costs ~50 registers, i.e. a wave per SIMD (134-166 registers against 185-226).  Built: pairs with one light
//   with and without PGRAD; pairs under the loop and the one-pixel form under the loop with PGRAD only -- they serve the calls without
//   g_params too.  As in cook_torrance_backward_kernel no lane of a PGRAD kernel leaves early: a lane outside the map shades a clamped
//   position with a zero upstream gradient and stores nothing.  With one wave per workgroup the order of the LDS additions is fixed, and
//   the rows are added up in fp64 in a fixed order: deterministic.
template <int LIGHT, int WF, int VEC, typename TM, bool PGRAD, bool MULTI>
__global__ __launch_bounds__(64) __attribute__((amdgpu_waves_per_eu(MULTI ? 2 : 3)))
void cook_torrance_camera_backward_kernel(const KArgs a, const BArgs b) {
    using R = typename RealOf<VEC, true>::type;
    static_assert(RealOf<VEC, true>::N == 1, "one pixel group per lane");
    const uint32_t tile = tile_of_workgroup(a, blockIdx.x);
    const int ty = (int)a.div_tx.div(tile);
    const LanePos p = lane_pos<VEC, PGRAD>(a, (int)tile - ty * a.tiles_x, ty);
    if (!PGRAD && !p.valid) return;
    constexpr int kParamSlots = 3 + 6 * PBR_MAX_LIGHTS;
    __shared__ float s_param[PGRAD ? kParamSlots : 1];
    const int n_param = 3 + 6 * a.n_lights;
    if constexpr (PGRAD) {
        for (int i = threadIdx.x; i < n_param; i += blockDim.x) s_param[i] = 0.0f;
        __syncthreads();
    }
    Texels<VEC> t;
    float go[3][VEC];
    load_texels<WF, TM, VEC, true>(a, a.has_normal != 0, p, t);
#pragma unroll
    for (int c = 0; c < 3; ++c) {
        if (p.sb) Ld<float, VEC>::template load<true>(plane_at<float>(b.gout, p.b0 * a.o_bs + c * a.o_cs, (uint32_t)p.pix), 0, go[c]);
        else Ld<float, VEC>::template load<true>(b.gout, p.b * a.o_bs + p.pix + c * a.o_cs, go[c]);
    }
    if (PGRAD && !p.valid) {
#pragma unroll
        for (int c = 0; c < 3; ++c)
#pragma unroll
            for (int j = 0; j < VEC; ++j) go[c][j] = 0.0f;
    }
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
    const R up[3] = {gather<R>(go[0], 0), gather<R>(go[1], 0), gather<R>(go[2], 0)};
    R g_col[3];
    const bool srgb = a.out_srgb != 0;
    if constexpr (MULTI) colour_adjoint_lights<LIGHT>(a, srgb, x.pt, V, xs, ys, up, g_col);     // the summed colour decides the outer clamp: pass 1
    PixelAdjointT<R> adj;
    adj.clear();
    Vec3T<R> g_view = {splat<R>(0.0f), splat<R>(0.0f), splat<R>(0.0f)};                  // adjoint of the pixel's unit view vector
    const int nl = MULTI ? a.n_lights : 1;
    for (int l = 0; l < nl; ++l) {
        const LightU lu = light_of(a, l);
        const LightGeomT<R> lg = light_geom<LIGHT, R>(lu, V, xs, ys);
        LightEvalT<R> e;
        eval_light(x.pt, lg, lu.inten, e);
        if constexpr (!MULTI) colour_adjoint(srgb, e.uc, up, g_col);
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
        // v = e / |e|: g_C = (g_v - v (v . g_v)) / |e|, with N.V's direct share gv n in g_v (:163); rv = 1/|e| is pixel_view's v_rsq
        const Vec3T<R> gvw = {fma_(gv, x.pt.n.x, g_view.x), fma_(gv, x.pt.n.y, g_view.y), fma_(gv, x.pt.n.z, g_view.z)};
        const R radial = dotv(gvw, V);
        float v8[8] = {hsum(fma_(-V.x, radial, gvw.x) * rv), hsum(fma_(-V.y, radial, gvw.y) * rv), hsum(fma_(-V.z, radial, gvw.z) * rv),
                       0.0f, 0.0f, 0.0f, 0.0f, 0.0f};
        pgrad_add8(v8, 3, s_param, s_param + 3);
        __syncthreads();
        if (b.g_param_partials) {
            for (int i = threadIdx.x; i < n_param; i += blockDim.x) b.g_param_partials[(int64_t)blockIdx.x * n_param + i] = s_param[i];
        }
        if (!p.valid) return;
    }
    store_gradients<WF, VEC, TM>(a, b, p, ga, gn, gr, gm, gs);
}

// ------------------------------------------------------------------ launchers
template <int L, int W>
static KernelFn pick_camera_variant(bool half_maps, int vec, bool several) {
    if (vec == 1) return half_maps ? cook_torrance_camera_kernel<L, W, __half, 1, true> : cook_torrance_camera_kernel<L, W, float, 1, true>;
    if (half_maps) return cook_torrance_camera_kernel<L, W, __half, 4, true>;
    return several ? cook_torrance_camera_kernel<L, W, float, 4, true> : cook_torrance_camera_kernel<L, W, float, 4, false>;
}

using CameraBwdFn = void (*)(const KArgs, const BArgs);
template <int L, int W, typename T>
static CameraBwdFn pick_camera_bwd_variant(int vec, bool params, bool several) {
    if (vec == 1) return cook_torrance_camera_backward_kernel<L, W, 1, T, true, true>;
    if (several) return cook_torrance_camera_backward_kernel<L, W, 2, T, true, true>;
    return params ? cook_torrance_camera_backward_kernel<L, W, 2, T, true, false> : cook_torrance_camera_backward_kernel<L, W, 2, T, false, false>;
}

}  // namespace pbr

extern "C" {

int pbr_cook_torrance_camera(const pbr_render_desc *d, void *stream) {
    using namespace pbr;
    const TuningScope tuning(d);
    const int rc = camera_gate(d);
    if (rc != PBR_OK) return rc;
    hipStream_t st = static_cast<hipStream_t>(stream);
    if (nan_grid(d)) return fill_result_nan(d, st);
    const int vec = d->width % 4 == 0 ? 4 : 1;
    KArgs k;
    camera_args(d, vec, k, 0);
    if (k.n_tiles < 0) return PBR_ERR_SHAPE;
    const bool half_maps = d->map_dtype == PBR_F16, several = d->n_lights > 1;
    const KernelFn fn = with_light_workflow(d, [&](auto L, auto W) -> KernelFn { return pick_camera_variant<L(), W()>(half_maps, vec, several); });
    // the occupancy governor of the one-light fp32 kernels (ct_launch.hpp: kLdsFor11WavesPerCu), as pbr_cook_torrance applies it
    const bool fp32_one_light = !half_maps && !several && k.bt_log2 == 6;
    const size_t lds = g_lds_bytes >= 0 ? (size_t)g_lds_bytes : (fp32_one_light ? kLdsFor11WavesPerCu : 0);
    hipLaunchKernelGGL(fn, dim3((unsigned)k.n_tiles, 1, 1), dim3(1u << k.bt_log2, 1, 1), lds, st, k);
    return launch_status();
}

size_t pbr_camera_backward_workspace_bytes(const pbr_render_desc *d) {
    const pbr::TuningScope tuning(d);
    if (pbr::camera_gate(d) != PBR_OK) return 0;
    return pbr::max_tiles(d) < 0 ? 0 : pbr::param_rows_bytes(d) + pbr::param_stage_bytes(d);
}

int pbr_cook_torrance_camera_backward(const pbr_render_desc *d, const void *grad_out, void *g_albedo, void *g_normal, void *g_roughness,
                                      void *g_metallic, void *g_specular, void *g_params, void *workspace, void *stream) {
    using namespace pbr;
    const TuningScope tuning(d);
    const int rc = camera_gate(d);
    if (rc != PBR_OK) return rc;
    if (!grad_out) return PBR_ERR_NULL_MAP;
    if (g_params && !workspace) return PBR_ERR_NULL_MAP;
    if (nan_grid(d)) return PBR_ERR_UNSUPPORTED;
    const int vec = d->width % 2 == 0 ? 2 : 1;
    KArgs k;
    camera_args(d, vec, k, 6);                                       // one-wave workgroups: the kernel's comment
    if (k.n_tiles < 0) return PBR_ERR_SHAPE;
    if (g_params && k.n_tiles > max_tiles(d)) return PBR_ERR_SHAPE;   // one workspace row per workgroup: never past what the size query promised
    k.o_cs = (int64_t)d->height * d->width; k.o_bs = 3 * k.o_cs;     // grad_out and the g_* are contiguous, whatever `out` was
    const BArgs b = {grad_out, g_albedo, g_normal, g_roughness, g_metallic, g_specular, g_params ? static_cast<float *>(workspace) : nullptr};
    hipStream_t st = static_cast<hipStream_t>(stream);
    const bool half_maps = d->map_dtype == PBR_F16, params = g_params != nullptr;
    const CameraBwdFn fn = with_light_workflow(d, [&](auto L, auto W) -> CameraBwdFn {
        return half_maps ? pick_camera_bwd_variant<L(), W(), __half>(vec, params, d->n_lights > 1)
                         : pick_camera_bwd_variant<L(), W(), float>(vec, params, d->n_lights > 1);
    });
    hipLaunchKernelGGL(fn, dim3((unsigned)k.n_tiles, 1, 1), dim3(64, 1, 1), 0, st, k, b);
    const int e = launch_status();
    if (e != PBR_OK || !g_params) return e;
    return param_grad_finish(d, static_cast<const float *>(workspace), (int)k.n_tiles, k.dev, static_cast<float *>(g_params), st, true);
}

}  // extern "C"
