// ct_camera_stack.hip -- light stacks under the perspective camera (C ABI: pbr_cook_torrance_camera_stack,
// pbr_cook_torrance_camera_mse_stack_step, pbr_cook_torrance_camera_mse_stack_fit_step): the capture ct_stack.hip describes -- L photographs
// from ONE camera position with the light moved between the shots -- taken from close by, where no single view direction reproduces it
// (ct_camera.hip).  The descriptor's view_dir is the camera POSITION C; the view vector of pixel (y, x) is F.normalize(C - P(y, x)) on the
// point light's grid, for both light types.  Image l of the stack is what pbr_cook_torrance_camera gives for light l alone: its own clamp,
// its own encode.
//
// Layout and bytes are ct_stack.hip's: the stack is [B][L][3][H][W] fp32, contiguous; the maps are read once, the L targets once and the summed
// gradients written once, 64 + 12 L bytes per pixel (fp32 maps, metallic workflow).
//
// The kernels are the orthographic stack's with the view a PixelViewT<R> per pixel group: every piece is the shared template over the view
// type (pixel_view, material_terms / bwd_decode, light_geom, shade_light / eval_light, colour_adjoint<true>, backprop_light, bwd_tail, the
// StackMseLoss policy); the frame loss_step / backward_body_to is not used, because it reads ONE view for the launch (view_of).  The gradient
// of the position is ct_camera.hip's: (g_v - v (v . g_v)) / |C - P| per pixel, applied BEFORE the sum over pixels.
#include "ct_stack_host.hpp"

namespace pbr {

// ------------------------------------------------------------------ forward: the stack itself
// cook_torrance_stack_kernel (ct_stack.hip) with the view of cook_torrance_camera_kernel's LOOP form: the grid is evaluated for both light
// types, material_terms runs once per pixel group with the group's own view, and the lights' loop hands that view to light_geom.
template <int LIGHT, int WF, typename TI, int VEC>
__global__ __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu(3, 8)))
void cook_torrance_camera_stack_kernel(const KArgs a) {
    using R = typename RealOf<VEC, true>::type;
    constexpr int NG = RealOf<VEC, true>::N;
    const uint32_t tile = tile_of_workgroup(a, blockIdx.x);
    const int ty = (int)a.div_tx.div(tile);
    const LanePos p = lane_pos<VEC>(a, (int)tile - ty * a.tiles_x, ty);
    if (!p.valid) return;
    Texels<VEC> t;
    load_texels<WF, TI, VEC, VEC != 1>(a, a.has_normal != 0, p, t);
    decode_texels<WF, VEC, true>(a, t);
    const Vec3 C = camera_of(a);
    const float ys = linspace_at(a.y0, a.y1, a.ystep, a.H_total, p.y + a.y_offset);      // the grid is the camera's for both light types
    R xs[NG];
    x_grid<R, NG, VEC>(a, p.x, xs);
    PixelTermsT<R> pt[NG];
    PixelViewT<R> V[NG];
#pragma unroll
    for (int g = 0; g < NG; ++g) {
        R rv;
        V[g] = pixel_view(C, xs[g], ys, rv);
        material_terms<WF, VEC, R>(t, g, V[g], pt[g]);
    }
    float *const first = static_cast<float *>(a.out) + ((int64_t)p.b * a.o_bs + p.pix);      // channel 0 of light 0's image, this lane's pixels
    for (int l = 0; l < a.n_lights; ++l) {
        const LightU lu = light_of(a, l);
        R res[3][NG];
#pragma unroll
        for (int g = 0; g < NG; ++g) {
            const LightGeomT<R> lg = light_geom<LIGHT, R>(lu, V[g], xs[g], ys);
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
// One-wave workgroups, one pixel group per lane (VEC = 2: a packed pair, for even widths; VEC = 1 otherwise: mse_vec -- no lane sees a pixel
// twice), one partial sum of squared differences per workgroup.  The body is cook_torrance_camera_backward_kernel's MULTI form (bwd_decode ...
// light loop ... bwd_tail) with the StackMseLoss policy inside the light loop, as backward_body_to has it for the orthographic stack: per
// light the target pixels loaded a light ahead, eval_light, the image's own clamp and encode (colour_adjoint<true>), backprop_light into the
// shared accumulators; the tail and the stores once.  No second pass over the lights: a stack has no summed colour.
// Lanes outside the map shade a clamped position, so that every lane reaches the wave sums; their scale is 0, hence every adjoint they hold
// is exactly 0, and they store nothing and add nothing to the loss.
// PGRAD (the fit step): light l's six sums leave the lane inside the loop (pgrad_add8 -> the workgroup's LDS row of 3 + 6 L floats:
// camera, lights L x 3, intensities L x 3); after the tail the camera's per-pixel Jacobian, then the row goes to b.g_param_partials.  With one
// wave per workgroup the order of the LDS additions is fixed, and the rows are added up in fp64 in a fixed order: deterministic.
// The same statements over a loss policy are camera_stack_step (ct_camera_stack.hpp: the weighted sibling is built from it); this kernel keeps
// them inline, because through that function it is scheduled differently.  Change the two together.
template <int LIGHT, int WF, int VEC, typename TM, bool PGRAD>
__global__ __launch_bounds__(64)
void cook_torrance_camera_mse_stack_step_kernel(const KArgs a, const BArgs b, const float *__restrict__ targets, float scale, float *__restrict__ partials) {
    static_assert(VEC == 1 || VEC == 2, "one pixel group per lane: StackMseLoss walks the lights once per lane");
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
    StackMseLoss<VEC> loss;
    loss.sq = 0.0f;
    loss.scale = p.valid ? scale : 0.0f;                                      // a lane outside the map: every adjoint it holds is exactly 0
    loss.plane = a.o_cs;
    loss.lane = targets + ((int64_t)p.b * a.n_lights * 3 * a.o_cs + p.pix);   // 64-bit: B L 3 H W passes 2^31 long before a plane does
    loss.prefetch(0);
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
        colour_adjoint<true>(srgb, e.uc, tgt, loss.scale, g_col, sqd);        // THIS image's clamp (backprop_light masks it) and encode
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

template <int L, int W>
static KernelFn pick_camera_stack(bool half_maps, int vec) {
    if (half_maps) return vec == 4 ? cook_torrance_camera_stack_kernel<L, W, __half, 4> : cook_torrance_camera_stack_kernel<L, W, __half, 1>;
    return vec == 4 ? cook_torrance_camera_stack_kernel<L, W, float, 4> : cook_torrance_camera_stack_kernel<L, W, float, 1>;
}

template <int L, int W, bool PGRAD>
static LossStepFn pick_camera_stack_step(bool half_maps, int vec) {
    if (half_maps) return vec == 2 ? cook_torrance_camera_mse_stack_step_kernel<L, W, 2, __half, PGRAD> : cook_torrance_camera_mse_stack_step_kernel<L, W, 1, __half, PGRAD>;
    return vec == 2 ? cook_torrance_camera_mse_stack_step_kernel<L, W, 2, float, PGRAD> : cook_torrance_camera_mse_stack_step_kernel<L, W, 1, float, PGRAD>;
}

static const auto camera_stack_kernel = [](auto L, auto W, bool half_maps, int vec) { return pick_camera_stack<L(), W()>(half_maps, vec); };
static const auto camera_stack_step_kernel = [](auto L, auto W, auto PGRAD, bool half_maps, int vec) { return pick_camera_stack_step<L(), W(), PGRAD()>(half_maps, vec); };

}  // namespace pbr

extern "C" {

int pbr_cook_torrance_camera_stack(const pbr_render_desc *d, void *stream) {
    using namespace pbr;
    const TuningScope tuning(d);
    const int rc = camera_gate(d);
    return rc != PBR_OK ? rc : launch_stack(d, nan_grid(d), camera_args, camera_stack_kernel, stream);
}

int pbr_cook_torrance_camera_mse_stack_step(const pbr_render_desc *d, const void *targets, void *g_albedo, void *g_normal, void *g_roughness,
                                            void *g_metallic, void *g_specular, void *loss, void *workspace, void *stream) {
    using namespace pbr;
    return stack_loss_step<kCamera, false>(d, false, camera_stack_step_kernel,
                                           {targets, g_albedo, g_normal, g_roughness, g_metallic, g_specular, nullptr, loss, workspace, stream, {}, {}});
}

size_t pbr_camera_mse_stack_fit_workspace_bytes(const pbr_render_desc *d) {      // the orthographic fit layout
    using namespace pbr;
    const TuningScope tuning(d);
    return stack_fit_workspace_bytes(d, camera_step_gate(d, true) == PBR_OK, 3, 6);
}

int pbr_cook_torrance_camera_mse_stack_fit_step(const pbr_render_desc *d, const void *targets, void *g_albedo, void *g_normal, void *g_roughness,
                                                void *g_metallic, void *g_specular, void *g_params, void *loss, void *workspace, void *stream) {
    using namespace pbr;
    return stack_loss_step<kCamera, false>(d, true, camera_stack_step_kernel,
                                           {targets, g_albedo, g_normal, g_roughness, g_metallic, g_specular, g_params, loss, workspace, stream, {}, {}});
}

}  // extern "C"
