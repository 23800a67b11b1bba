// ct_stack_weighted.hip -- the light-stack loss steps of ct_stack.hip with a weight per pixel (C ABI: pbr_cook_torrance_weighted_mse_stack_step,
// pbr_cook_torrance_weighted_mse_stack_fit_step): loss = mean(w (stack - targets)^2) over all 3 B L H W elements (ct_weighted_stack.hpp).
// The kernel is cook_torrance_mse_stack_step_kernel's sibling: the same frame (ct_backward.hpp: loss_step around backward_body_to), the
// WeightedStackMseLoss policy.  Workspaces are the unweighted steps': pbr_mse_step_workspace_bytes, pbr_mse_stack_fit_workspace_bytes.
#include "ct_weighted_stack.hpp"

namespace pbr {

template <int LIGHT, int WF, int VEC, typename TM, bool PGRAD>
__global__ __launch_bounds__(64)
void cook_torrance_weighted_mse_stack_step_kernel(const KArgs a, const BArgs b, const WArgs w, const float *__restrict__ targets, float scale,
                                                  float *__restrict__ partials) {
    static_assert(VEC == 1 || (VEC == 2 && PBR_MSE_PACKED), "the stack policies walk the lights once per lane");
    float *s_param = nullptr;
    int n_param = 0;
    if constexpr (PGRAD) {
        __shared__ float s_row[3 + 6 * PBR_MAX_LIGHTS];
        s_param = s_row;
        n_param = 3 + 6 * a.n_lights;
        for (int i = threadIdx.x; i < n_param; i += 64) s_param[i] = 0.0f;      // a 16-light row holds 99 floats: more than the wave has lanes
        __syncthreads();
    }
    loss_step<LIGHT, WF, VEC, false, TM, PGRAD, WeightedStackMseLoss<VEC>>(a, b, s_param, n_param, partials,
        [&](const LanePos &p, WeightedStackMseLoss<VEC> &loss) {
            loss.scale = p.valid ? scale : 0.0f;                                      // a lane outside the map: every adjoint it holds is exactly 0
            loss.plane = a.o_cs;
            loss.lane = targets + ((int64_t)p.b * a.n_lights * 3 * a.o_cs + p.pix);   // 64-bit: B L 3 H W passes 2^31 long before a plane does
            weighted_first_loads<VEC>(p, w, loss);
        });
}

using WeightedStepFn = void (*)(const KArgs, const BArgs, const WArgs, const float *, float, float *);

template <int L, int W, bool PGRAD>
static WeightedStepFn pick_weighted_stack_step(bool half_maps, int vec) {
    if (half_maps) return vec == 2 ? cook_torrance_weighted_mse_stack_step_kernel<L, W, 2, __half, PGRAD> : cook_torrance_weighted_mse_stack_step_kernel<L, W, 1, __half, PGRAD>;
    return vec == 2 ? cook_torrance_weighted_mse_stack_step_kernel<L, W, 2, float, PGRAD> : cook_torrance_weighted_mse_stack_step_kernel<L, W, 1, float, PGRAD>;
}

// launch_loss_step (ct_loss.hip) with the weights between BArgs and the targets.
static int launch_weighted_loss_step(const pbr_render_desc *d, WeightedStepFn fn, int vec, const BArgs &b, const WArgs &w, const void *targets,
                                     double count, float *partials, hipStream_t st, KArgs &k) {
    fill_args(d, vec, k, 6);
    if (k.n_tiles < 0) return PBR_ERR_SHAPE;
    if (b.g_param_partials) {
        const int64_t most = max_tiles(d);
        if (most < 0 || k.n_tiles > most) return PBR_ERR_SHAPE;
    }
    k.o_cs = (int64_t)d->height * d->width; k.o_bs = 3 * k.o_cs;
    hipLaunchKernelGGL(fn, dim3((unsigned)k.n_tiles, 1, 1), dim3(64, 1, 1), 0, st, k, b, w, static_cast<const float *>(targets), (float)(2.0 / count), partials);
    return launch_status();
}

// Both entry points: g_params = NULL is the step, else the fit step (`fit`: its pointer was asked for).
static int weighted_stack_step(const pbr_render_desc *d, const void *targets, const void *weights, int64_t w_batch_stride, int64_t w_light_stride,
                               void *g_albedo, void *g_normal, void *g_roughness, void *g_metallic, void *g_specular, bool fit, void *g_params,
                               void *loss, void *workspace, void *stream) {
    const TuningScope tuning(d);
    int rc = mse_gate(d, (!fit || g_params) && targets && weights && loss && workspace, false);
    if (rc == PBR_OK) rc = weights_shape(d, w_light_stride);
    if (rc != PBR_OK) return rc;
    const bool half_maps = d->map_dtype == PBR_F16;
    const int vec = mse_vec(d);
    const WeightedStepFn fn = with_light_workflow(d, [&](auto L, auto W) -> WeightedStepFn {
        return fit ? pick_weighted_stack_step<L(), W(), true>(half_maps, vec) : pick_weighted_stack_step<L(), W(), false>(half_maps, vec);
    });
    const double count = 3.0 * (double)d->batch * (double)d->n_lights * (double)d->height * (double)d->width;
    hipStream_t st = static_cast<hipStream_t>(stream);
    float *const partials = static_cast<float *>(workspace);
    float *const rows = fit ? reinterpret_cast<float *>(static_cast<char *>(workspace) + pbr_mse_step_workspace_bytes(d)) : nullptr;      // one row per workgroup
    const BArgs b = {nullptr, g_albedo, g_normal, g_roughness, g_metallic, g_specular, rows};
    const WArgs w = {static_cast<const float *>(weights), w_batch_stride, w_light_stride};
    KArgs k;
    int e = launch_weighted_loss_step(d, fn, vec, b, w, targets, count, partials, st, k);
    if (e == PBR_OK && fit) e = param_grad_finish(d, rows, k.n_tiles, k.dev, static_cast<float *>(g_params), st);
    return e != PBR_OK ? e : mse_finish(d, partials, k.n_tiles, count, static_cast<float *>(loss), st);
}

}  // namespace pbr

extern "C" {

int pbr_cook_torrance_weighted_mse_stack_step(const pbr_render_desc *d, const void *targets, const void *weights, int64_t w_batch_stride,
                                              int64_t w_light_stride, void *g_albedo, void *g_normal, void *g_roughness, void *g_metallic,
                                              void *g_specular, void *loss, void *workspace, void *stream) {
    return pbr::weighted_stack_step(d, targets, weights, w_batch_stride, w_light_stride, g_albedo, g_normal, g_roughness, g_metallic, g_specular,
                                    false, nullptr, loss, workspace, stream);
}

int pbr_cook_torrance_weighted_mse_stack_fit_step(const pbr_render_desc *d, const void *targets, const void *weights, int64_t w_batch_stride,
                                                  int64_t w_light_stride, void *g_albedo, void *g_normal, void *g_roughness, void *g_metallic,
                                                  void *g_specular, void *g_params, void *loss, void *workspace, void *stream) {
    return pbr::weighted_stack_step(d, targets, weights, w_batch_stride, w_light_stride, g_albedo, g_normal, g_roughness, g_metallic, g_specular,
                                    true, g_params, loss, workspace, stream);
}

}  // extern "C"
