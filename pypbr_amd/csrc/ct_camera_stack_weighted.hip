// ct_camera_stack_weighted.hip -- the camera's light-stack loss steps of ct_camera_stack.hip with a weight per pixel (C ABI:
// pbr_cook_torrance_camera_weighted_mse_stack_step, pbr_cook_torrance_camera_weighted_mse_stack_fit_step): loss = mean(w (stack - targets)^2)
// over all 3 B L H W elements (ct_weighted_stack.hpp).  The kernel is cook_torrance_camera_mse_stack_step_kernel's sibling: the same body
// (ct_camera_stack.hpp: camera_stack_step), the WeightedStackMseLoss policy.  Workspaces are the unweighted steps'.
#include "ct_camera_stack.hpp"
#include "ct_weighted_stack.hpp"

namespace pbr {

template <int LIGHT, int WF, int VEC, typename TM, bool PGRAD>
__global__ __launch_bounds__(64)
void cook_torrance_camera_weighted_mse_stack_step_kernel(const KArgs a, const BArgs b, const WArgs w, const float *__restrict__ targets, float scale,
                                                         float *__restrict__ partials) {
    camera_stack_step<LIGHT, WF, VEC, TM, PGRAD, WeightedStackMseLoss<VEC>>(a, b, targets, scale, partials,
        [&](const LanePos &p, WeightedStackMseLoss<VEC> &loss) { weighted_first_loads<VEC>(p, w, loss); });
}

using WeightedStepFn = void (*)(const KArgs, const BArgs, const WArgs, const float *, float, float *);

template <int L, int W, bool PGRAD>
static WeightedStepFn pick_weighted_stack_step(bool half_maps, int vec) {
    if (half_maps) return vec == 2 ? cook_torrance_camera_weighted_mse_stack_step_kernel<L, W, 2, __half, PGRAD> : cook_torrance_camera_weighted_mse_stack_step_kernel<L, W, 1, __half, PGRAD>;
    return vec == 2 ? cook_torrance_camera_weighted_mse_stack_step_kernel<L, W, 2, float, PGRAD> : cook_torrance_camera_weighted_mse_stack_step_kernel<L, W, 1, float, PGRAD>;
}

// Both entry points: g_params = NULL is the step, else the fit step (`fit`: its pointer was asked for).
static int weighted_camera_stack_step(const pbr_render_desc *d, const void *targets, const void *weights, int64_t w_batch_stride,
                                      int64_t w_light_stride, void *g_albedo, void *g_normal, void *g_roughness, void *g_metallic, void *g_specular,
                                      bool fit, void *g_params, void *loss, void *workspace, void *stream) {
    const TuningScope tuning(d);
    int rc = camera_step_gate(d, (!fit || g_params) && targets && weights && loss && workspace);
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
    int e = launch_camera_loss_step(d, fn, vec, b, targets, count, partials, st, k, w);
    if (e == PBR_OK && fit) e = param_grad_finish(d, rows, k.n_tiles, k.dev, static_cast<float *>(g_params), st, true);
    return e != PBR_OK ? e : mse_finish(d, partials, k.n_tiles, count, static_cast<float *>(loss), st);
}

}  // namespace pbr

extern "C" {

int pbr_cook_torrance_camera_weighted_mse_stack_step(const pbr_render_desc *d, const void *targets, const void *weights, int64_t w_batch_stride,
                                                     int64_t w_light_stride, void *g_albedo, void *g_normal, void *g_roughness, void *g_metallic,
                                                     void *g_specular, void *loss, void *workspace, void *stream) {
    return pbr::weighted_camera_stack_step(d, targets, weights, w_batch_stride, w_light_stride, g_albedo, g_normal, g_roughness, g_metallic,
                                           g_specular, false, nullptr, loss, workspace, stream);
}

int pbr_cook_torrance_camera_weighted_mse_stack_fit_step(const pbr_render_desc *d, const void *targets, const void *weights, int64_t w_batch_stride,
                                                         int64_t w_light_stride, void *g_albedo, void *g_normal, void *g_roughness, void *g_metallic,
                                                         void *g_specular, void *g_params, void *loss, void *workspace, void *stream) {
    return pbr::weighted_camera_stack_step(d, targets, weights, w_batch_stride, w_light_stride, g_albedo, g_normal, g_roughness, g_metallic,
                                           g_specular, true, g_params, loss, workspace, stream);
}

}  // extern "C"
