// ct_camera_stack_weighted.hip -- the camera's light-stack loss steps of ct_camera_stack.hip with a weight per pixel (C ABI:
// pbr_cook_torrance_camera_weighted_mse_stack_step, pbr_cook_torrance_camera_weighted_mse_stack_fit_step): loss = mean(w (stack - targets)^2)
// over all 3 B L H W elements (ct_weighted_stack.hpp).  The kernel is cook_torrance_camera_mse_stack_step_kernel's sibling: the same body
// (ct_camera_stack.hpp: camera_stack_step), the WeightedStackMseLoss policy.  Workspaces are the unweighted steps'.
#include "ct_stack_host.hpp"

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

static const auto weighted_step_kernel = [](auto L, auto W, auto PGRAD, bool half_maps, int vec) { return pick_weighted_stack_step<L(), W(), PGRAD()>(half_maps, vec); };

}  // namespace pbr

extern "C" {

int pbr_cook_torrance_camera_weighted_mse_stack_step(const pbr_render_desc *d, const void *targets, const void *weights, int64_t w_batch_stride,
                                                     int64_t w_light_stride, void *g_albedo, void *g_normal, void *g_roughness, void *g_metallic,
                                                     void *g_specular, void *loss, void *workspace, void *stream) {
    using namespace pbr;
    return stack_loss_step<kCamera, true>(d, false, weighted_step_kernel,
                                          {targets, g_albedo, g_normal, g_roughness, g_metallic, g_specular, nullptr, loss, workspace, stream, {},
                                           {static_cast<const float *>(weights), w_batch_stride, w_light_stride}});
}

int pbr_cook_torrance_camera_weighted_mse_stack_fit_step(const pbr_render_desc *d, const void *targets, const void *weights, int64_t w_batch_stride,
                                                         int64_t w_light_stride, void *g_albedo, void *g_normal, void *g_roughness, void *g_metallic,
                                                         void *g_specular, void *g_params, void *loss, void *workspace, void *stream) {
    using namespace pbr;
    return stack_loss_step<kCamera, true>(d, true, weighted_step_kernel,
                                          {targets, g_albedo, g_normal, g_roughness, g_metallic, g_specular, g_params, loss, workspace, stream, {},
                                           {static_cast<const float *>(weights), w_batch_stride, w_light_stride}});
}

}  // extern "C"
