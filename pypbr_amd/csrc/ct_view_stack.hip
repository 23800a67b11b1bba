// ct_view_stack.hip -- light stacks with one camera position PER SHOT (C ABI: pbr_cook_torrance_view_stack,
// pbr_cook_torrance_view_mse_stack_step, pbr_cook_torrance_view_mse_stack_fit_step): the handheld capture -- a phone with the flash next to the
// lens, camera and light moving together from shot to shot, the photographs rectified to the texel grid afterwards.  ct_camera_stack.hip is the
// tripod: ONE position for all L shots.  Here image l of the stack is what pbr_cook_torrance_camera gives for camera l and light l alone: its
// own view vectors F.normalize(C_l - P(y, x)), its own clamp, its own encode.
//
// Layout and bytes are ct_stack.hip's: the stack is [B][L][3][H][W] fp32, contiguous; maps read once, the L targets once, the summed gradients
// written once, 64 + 12 L bytes per pixel (fp32 maps, metallic workflow).  What a shot costs more than in ct_camera_stack.hip is VALU work: the
// view's v_rsq and the six view-dependent pixel terms (brdf_math.hpp: view_terms), about a dozen operations.
//
// The kernels are the camera stack's with the view moved INTO the light loop.  The view-independent pixel terms (unit normal, a2, k, omk, kk,
// kb, f0) are formed once per pixel group -- material_terms / bwd_decode with a placeholder view, whose six view-dependent results are
// overwritten by view_terms before anything reads them --, then per shot pixel_view, view_terms, light_geom, shade_light / eval_light.
// In the chain rule N.V now depends on the shot, so its adjoint cannot wait for the light-independent tail: shot l's g_ndv is closed inside
// the loop -- gv_l = masked(in_unit(N.V_l), g_ndv_l), g_n += gv_l V_l -- and bwd_tail runs with nothing left in g_ndv.  The camera's adjoint is
// per shot too: g_C_l = (gvw_l - V_l (V_l . gvw_l)) / |C_l - P| with gvw_l = gv_l n + (the light's share of the view's adjoint), applied per
// pixel BEFORE the sum over pixels, as in ct_camera.hip.
//
// The positions come beside the descriptor (desc->view_dir and the device block's view are not read): [L][3] host values, which travel in the
// kernel arguments, or a plain fp32 [L][3] device pointer that the kernel reads, wave-uniformly, when it runs -- no read-back, nothing baked in,
// so a captured graph sees the positions' current values at every replay.  Lights and intensities: the descriptor or its device_params block.
#include "ct_stack_host.hpp"

namespace pbr {

// ------------------------------------------------------------------ forward: the stack itself
// cook_torrance_camera_stack_kernel with the view inside the light loop.
template <int LIGHT, int WF, typename TI, int VEC>
__global__ __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu(3, 8)))
void cook_torrance_view_stack_kernel(const KArgs a, const ViewArgs va) {
    using R = typename RealOf<VEC, true>::type;
    constexpr int NG = RealOf<VEC, true>::N;
    const uint32_t tile = tile_of_workgroup(a, blockIdx.x);
    const int ty = (int)a.div_tx.div(tile);
    const LanePos p = lane_pos<VEC>(a, (int)tile - ty * a.tiles_x, ty);
    if (!p.valid) return;
    Texels<VEC> t;
    load_texels<WF, TI, VEC, VEC != 1>(a, a.has_normal != 0, p, t);
    decode_texels<WF, VEC, true>(a, t);
    const float ys = linspace_at(a.y0, a.y1, a.ystep, a.H_total, p.y + a.y_offset);      // the grid is the camera's for both light types
    R xs[NG];
    x_grid<R, NG, VEC>(a, p.x, xs);
    PixelTermsT<R> pt[NG];
#pragma unroll
    for (int g = 0; g < NG; ++g) material_terms<WF, VEC, R>(t, g, no_view(), pt[g]);
    float *const first = static_cast<float *>(a.out) + ((int64_t)p.b * a.o_bs + p.pix);      // channel 0 of shot 0's image, this lane's pixels
    for (int l = 0; l < a.n_lights; ++l) {
        const LightU lu = light_of(a, l);
        const Vec3 C = camera_at(va, l);
        R res[3][NG];
#pragma unroll
        for (int g = 0; g < NG; ++g) {
            R rv;
            const PixelViewT<R> V = pixel_view(C, xs[g], ys, rv);
            view_terms(pt[g], V);
            const LightGeomT<R> lg = light_geom<LIGHT, R>(lu, V, xs[g], ys);
            R col[3];
            shade_light(pt[g], lg, lu.inten, col);
#pragma unroll
            for (int c = 0; c < 3; ++c) res[c][g] = a.out_srgb ? linear_to_srgb_unit(col[c]) : col[c];      // :179-180
        }
#pragma unroll
        for (int c = 0; c < 3; ++c) {
            float o[VEC];
#pragma unroll
            for (int g = 0; g < NG; ++g) scatter(o, g, res[c][g]);
            Ld<float, VEC>::template store<VEC != 1 ? St::hinted : St::plain>(first, ((int64_t)l * 3 + c) * a.o_cs, o);
        }
    }
}

// ------------------------------------------------------------------ the loss step over the stack
// cook_torrance_camera_mse_stack_step_kernel's frame: one-wave workgroups, one pixel group per lane (mse_vec), one partial sum of squared
// differences per workgroup; lanes outside the map shade a clamped position with scale 0, store nothing and add nothing.
// PGRAD (the fit step): the workgroup's LDS row is 9 L floats, [cameras L x 3 | lights L x 3 | intensities L x 3]; shot l's nine sums leave the
// lane inside the loop (pgrad_add8: the light's six, and the cameras' three of two shots together).  At L = 16 a row holds 144 floats, more
// than the wave has lanes: the zeroing and the copy-out stride.  One wave per workgroup, so the order of the LDS additions is fixed, and the
// rows are added up in fp64 in a fixed order: deterministic.
// The same statements over a loss policy are view_stack_step (ct_camera_stack.hpp: the weighted sibling is built from it); this kernel keeps
// them inline, because through that function it is scheduled differently.  Change the two together.
template <int LIGHT, int WF, int VEC, typename TM, bool PGRAD>
__global__ __launch_bounds__(64)
void cook_torrance_view_mse_stack_step_kernel(const KArgs a, const BArgs b, const ViewArgs va, const float *__restrict__ targets, float scale,
                                              float *__restrict__ partials) {
    static_assert(VEC == 1 || VEC == 2, "one pixel group per lane: StackMseLoss walks the lights once per lane");
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
    StackMseLoss<VEC> loss;
    loss.sq = 0.0f;
    loss.scale = p.valid ? scale : 0.0f;                                      // a lane outside the map: every adjoint it holds is exactly 0
    loss.plane = a.o_cs;
    loss.lane = targets + ((int64_t)p.b * nl * 3 * a.o_cs + p.pix);           // 64-bit: B L 3 H W passes 2^31 long before a plane does
    loss.prefetch(0);
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
        colour_adjoint<true>(srgb, e.uc, tgt, loss.scale, g_col, sqd);        // THIS image's clamp (backprop_light masks it) and encode
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

using ViewStackFn = void (*)(const KArgs, const ViewArgs);
using ViewStepFn = void (*)(const KArgs, const BArgs, const ViewArgs, const float *, float, float *);

template <int L, int W>
static ViewStackFn pick_view_stack(bool half_maps, int vec) {
    if (half_maps) return vec == 4 ? cook_torrance_view_stack_kernel<L, W, __half, 4> : cook_torrance_view_stack_kernel<L, W, __half, 1>;
    return vec == 4 ? cook_torrance_view_stack_kernel<L, W, float, 4> : cook_torrance_view_stack_kernel<L, W, float, 1>;
}

template <int L, int W, bool PGRAD>
static ViewStepFn pick_view_stack_step(bool half_maps, int vec) {
    if (half_maps) return vec == 2 ? cook_torrance_view_mse_stack_step_kernel<L, W, 2, __half, PGRAD> : cook_torrance_view_mse_stack_step_kernel<L, W, 1, __half, PGRAD>;
    return vec == 2 ? cook_torrance_view_mse_stack_step_kernel<L, W, 2, float, PGRAD> : cook_torrance_view_mse_stack_step_kernel<L, W, 1, float, PGRAD>;
}

static const auto view_stack_kernel = [](auto L, auto W, bool half_maps, int vec) { return pick_view_stack<L(), W()>(half_maps, vec); };
static const auto view_stack_step_kernel = [](auto L, auto W, auto PGRAD, bool half_maps, int vec) { return pick_view_stack_step<L(), W(), PGRAD()>(half_maps, vec); };

}  // namespace pbr

extern "C" {

int pbr_cook_torrance_view_stack(const pbr_render_desc *d, const float *cameras_host, const void *cameras_device, void *stream) {
    using namespace pbr;
    const TuningScope tuning(d);
    const int rc = camera_gate(d);
    if (rc != PBR_OK) return rc;
    if (!one_camera_source(cameras_host, cameras_device)) return PBR_ERR_NULL_MAP;
    return launch_stack(d, nan_grid(d), camera_args, view_stack_kernel, stream, view_args(d, cameras_host, cameras_device));
}

int pbr_cook_torrance_view_mse_stack_step(const pbr_render_desc *d, const float *cameras_host, const void *cameras_device, const void *targets,
                                          void *g_albedo, void *g_normal, void *g_roughness, void *g_metallic, void *g_specular, void *loss,
                                          void *workspace, void *stream) {
    using namespace pbr;
    return stack_loss_step<kShotCameras, false>(d, false, view_stack_step_kernel,
                                                {targets, g_albedo, g_normal, g_roughness, g_metallic, g_specular, nullptr, loss, workspace, stream,
                                                 {cameras_host, cameras_device}, {}});
}

size_t pbr_view_mse_stack_fit_workspace_bytes(const pbr_render_desc *d) {      // the camera fit layout with rows of 9 L floats
    using namespace pbr;
    const TuningScope tuning(d);
    return stack_fit_workspace_bytes(d, camera_step_gate(d, true) == PBR_OK && max_tiles(d) >= 0, 0, 9);
}

int pbr_cook_torrance_view_mse_stack_fit_step(const pbr_render_desc *d, const float *cameras_host, const void *cameras_device, const void *targets,
                                              void *g_albedo, void *g_normal, void *g_roughness, void *g_metallic, void *g_specular,
                                              void *g_params, void *loss, void *workspace, void *stream) {
    using namespace pbr;
    return stack_loss_step<kShotCameras, false>(d, true, view_stack_step_kernel,
                                                {targets, g_albedo, g_normal, g_roughness, g_metallic, g_specular, g_params, loss, workspace, stream,
                                                 {cameras_host, cameras_device}, {}});
}

}  // extern "C"
