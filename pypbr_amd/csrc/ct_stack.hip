// ct_stack.hip -- a light stack: L images of one material batch, one per light, out of ONE pass over the maps
// (C ABI: pbr_cook_torrance_stack, pbr_cook_torrance_mse_stack_step, pbr_cook_torrance_mse_stack_fit_step).
//
// A capture for SVBRDF fitting is a stack of photographs from one camera position with the light moved between the shots (a flash walked
// around a tripod, a light stage, photometric stereo); the loss is the mean squared error over ALL images.  Image l of the stack is exactly
// what the one-light evaluation gives for light l alone -- every image has its own clamp and its own encode -- which is not what the
// several-lights kernels compute: they sum the lights into one image.
//
// Layout: the stack is [B][L][3][H][W] fp32, contiguous; the lights share the view direction, the light type and light_size.
//
// Bytes per pixel (fp32 maps, metallic workflow).  L one-light loss steps read the eight map planes L times (32 L), their targets (12 L), write
// eight gradient planes L times (32 L), and autograd adds the L gradient sets up (read, read, write over 32 B for every light after the first):
// 76 L + 96 (L - 1).  Here the maps are read once, the L targets once, and the summed gradients are written once: 64 + 12 L.  At L = 8 that is
// 160 against 1280.
//
// The step is the frame of the one-wave loss steps (ct_backward.hpp: loss_step; host side ct_stack_host.hpp: stack_loss_step)
// around backward_body_to with the StackMseLoss policy: texels loaded and decoded once, pixel_terms once, then per light
// eval_light -> encode with slope -> difference to THAT light's target -> backprop_light into the shared accumulators, and the light-independent
// tail and the stores once.  No second pass over the lights: the summed-lights form needs one because the summed colour decides the outer clamp;
// in a stack every image is clamped and encoded by itself.  Light l + 1's target pixels are loaded before light l's arithmetic.
#include "ct_stack_host.hpp"

namespace pbr {

// ------------------------------------------------------------------ forward: the stack itself
// The several-lights branch of shade_and_store (ct_kernel.hpp) with the sum taken out: lights in the outer (uniform) loop, the lane's pixel
// groups inside it, and each light's clamped colour (shade_light clamps) encoded and stored to its own image.  Packed arithmetic, as for
// several lights everywhere; a.o_bs is the MATERIAL's stride in the stack (3 L planes), a.o_cs the plane.
template <int LIGHT, int WF, typename TI, int VEC>
__global__ __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu(4, 8)))
void cook_torrance_stack_kernel(const KArgs a) {
    using R = typename RealOf<VEC, true>::type;
    constexpr int NG = RealOf<VEC, true>::N;
    const uint32_t tile = tile_of_workgroup(a, blockIdx.x);
    const int ty = (int)a.div_tx.div(tile);
    const LanePos p = lane_pos<VEC>(a, (int)tile - ty * a.tiles_x, ty);
    if (!p.valid) return;
    Texels<VEC> t;
    load_texels<WF, TI, VEC, VEC != 1>(a, a.has_normal != 0, p, t);
    decode_texels<WF, VEC, true>(a, t);
    const Vec3 V = view_of(a);
    float ys = 0.0f;
    R xs[NG];
    if (LIGHT == PBR_LIGHT_POINT) {
        ys = linspace_at(a.y0, a.y1, a.ystep, a.H_total, p.y + a.y_offset);
        x_grid<R, NG, VEC>(a, p.x, xs);
    } else {
#pragma unroll
        for (int g = 0; g < NG; ++g) xs[g] = splat<R>(0.0f);
    }
    PixelTermsT<R> pt[NG];
#pragma unroll
    for (int g = 0; g < NG; ++g) material_terms<WF, VEC, R>(t, g, V, pt[g]);
    float *const first = static_cast<float *>(a.out) + ((int64_t)p.b * a.o_bs + p.pix);      // channel 0 of light 0's image, this lane's pixels
    for (int l = 0; l < a.n_lights; ++l) {
        const LightU lu = light_of(a, l);
        R res[3][NG];
#pragma unroll
        for (int g = 0; g < NG; ++g) {
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
// One kernel over the frame of the one-wave loss steps (ct_backward.hpp: loss_step) with the StackMseLoss policy: one partial sum per workgroup,
// no LDS reduction; lanes outside the map shade a clamped position (every lane reaches the wave sum), store nothing and contribute nothing.
// Pixels per lane: mse_vec.
//   PGRAD = false, the stack step.  Registers: the two-pixel body lands on 184-216 VGPRs (two waves per SIMD), the one-pixel body on 95-114
//   (four); held to three waves (168) every two-pixel instantiation spills 28-176 bytes per lane, so the allocation is left to the compiler
//   (DESIGN.md 3.14).
//   PGRAD = true, the stack-fit step: backward_body_to also forms the adjoints of view, light l and intensity l (backprop_light<LIGHT, true>),
//   light l's six sums leave the lane inside the run-time light loop (wave_sum8 -> the workgroup's LDS row), the view's three after the tail,
//   and the row -- 3 + 6 L floats: view, lights L x 3, intensities L x 3, the layout of pbr_cook_torrance_backward_params -- goes to
//   b.g_param_partials.  One wave per workgroup: the order of additions is fixed.  Lanes outside the map shade a clamped position and here,
//   unlike in the backward kernels, would form a real upstream gradient from a real target: their scale is 0, so every adjoint they hold is
//   exactly 0.  Registers: the two-pixel body lands on 200-236 VGPRs (two waves per SIMD, as the stack step's 184-216), the one-pixel body on
//   125-146 (three or four); no instantiation has scratch.
template <int LIGHT, int WF, int VEC, typename TM, bool PGRAD>
__global__ __launch_bounds__(64)
void cook_torrance_mse_stack_step_kernel(const KArgs a, const BArgs b, const float *__restrict__ targets, float scale, float *__restrict__ partials) {
    // one pixel group per lane (a packed pair or one pixel): the body's light loop runs once, so the one-light-ahead target loads stay in step
    static_assert(VEC == 1 || (VEC == 2 && PBR_MSE_PACKED), "StackMseLoss walks the lights once per lane");
    float *s_param = nullptr;
    int n_param = 0;
    if constexpr (PGRAD) {
        __shared__ float s_row[3 + 6 * PBR_MAX_LIGHTS];
        s_param = s_row;
        n_param = 3 + 6 * a.n_lights;
        for (int i = threadIdx.x; i < n_param; i += 64) s_param[i] = 0.0f;      // a 16-light row holds 99 floats: more than the wave has lanes
        __syncthreads();
    }
    loss_step<LIGHT, WF, VEC, false, TM, PGRAD, StackMseLoss<VEC>>(a, b, s_param, n_param, partials, [&](const LanePos &p, StackMseLoss<VEC> &loss) {
        loss.scale = scale;
        if constexpr (PGRAD) loss.scale = p.valid ? scale : 0.0f;                  // a lane outside the map: every adjoint it holds is exactly 0
        loss.plane = a.o_cs;
        loss.lane = targets + ((int64_t)p.b * a.n_lights * 3 * a.o_cs + p.pix);   // 64-bit: B L 3 H W passes 2^31 long before a plane does
        loss.prefetch(0);
    });
}

template <int L, int W, bool PGRAD>
static LossStepFn pick_stack_step(bool half_maps, int vec) {
    if (half_maps) return vec == 2 ? cook_torrance_mse_stack_step_kernel<L, W, 2, __half, PGRAD> : cook_torrance_mse_stack_step_kernel<L, W, 1, __half, PGRAD>;
    return vec == 2 ? cook_torrance_mse_stack_step_kernel<L, W, 2, float, PGRAD> : cook_torrance_mse_stack_step_kernel<L, W, 1, float, PGRAD>;
}

template <int L, int W>
static KernelFn pick_stack(bool half_maps, int vec) {
    if (half_maps) return vec == 4 ? cook_torrance_stack_kernel<L, W, __half, 4> : cook_torrance_stack_kernel<L, W, __half, 1>;
    return vec == 4 ? cook_torrance_stack_kernel<L, W, float, 4> : cook_torrance_stack_kernel<L, W, float, 1>;
}

// What the stack's entry point serves beyond a valid descriptor: an fp32 stack of untiled maps (contiguous: launch_stack asks).
static int stack_serves(const pbr_render_desc *d) {
    if (d->out_dtype != PBR_F32) return PBR_ERR_DTYPE;
    return is_tiled(d) ? PBR_ERR_UNSUPPORTED : PBR_OK;
}

static const auto stack_kernel = [](auto L, auto W, bool half_maps, int vec) { return pick_stack<L(), W()>(half_maps, vec); };
static const auto stack_step_kernel = [](auto L, auto W, auto PGRAD, bool half_maps, int vec) { return pick_stack_step<L(), W(), PGRAD()>(half_maps, vec); };

}  // namespace pbr

extern "C" {

int pbr_cook_torrance_stack(const pbr_render_desc *d, void *stream) {
    using namespace pbr;
    const TuningScope tuning(d);
    int rc = validate(d);
    if (rc == PBR_OK) rc = stack_serves(d);
    return rc != PBR_OK ? rc : launch_stack(d, nan_light_size(d), fill_args, stack_kernel, stream);
}

int pbr_cook_torrance_mse_stack_step(const pbr_render_desc *d, const void *targets, void *g_albedo, void *g_normal, void *g_roughness,
                                     void *g_metallic, void *g_specular, void *loss, void *workspace, void *stream) {
    using namespace pbr;
    return stack_loss_step<kOrthographic, false>(d, false, stack_step_kernel,
                                                 {targets, g_albedo, g_normal, g_roughness, g_metallic, g_specular, nullptr, loss, workspace, stream, {}, {}});
}

size_t pbr_mse_stack_fit_workspace_bytes(const pbr_render_desc *d) {
    using namespace pbr;
    const TuningScope tuning(d);
    return stack_fit_workspace_bytes(d, mse_gate(d, true, false) == PBR_OK, 3, 6);
}

int pbr_cook_torrance_mse_stack_fit_step(const pbr_render_desc *d, const void *targets, void *g_albedo, void *g_normal, void *g_roughness,
                                         void *g_metallic, void *g_specular, void *g_params, void *loss, void *workspace, void *stream) {
    using namespace pbr;
    return stack_loss_step<kOrthographic, false>(d, true, stack_step_kernel,
                                                 {targets, g_albedo, g_normal, g_roughness, g_metallic, g_specular, g_params, loss, workspace, stream, {}, {}});
}

}  // extern "C"
