// ct_stack_weighted.hip -- the light-stack loss steps of ct_stack.hip with a weight per pixel (C ABI: pbr_cook_torrance_weighted_mse_stack_step,
// pbr_cook_torrance_weighted_mse_stack_fit_step): loss = mean(w (stack - targets)^2) over all 3 B L H W elements (ct_weighted_stack.hpp).
// The kernel is cook_torrance_mse_stack_step_kernel's sibling: the same frame (ct_backward.hpp: loss_step around backward_body_to), the
// WeightedStackMseLoss policy.  Workspaces are the unweighted steps': pbr_mse_step_workspace_bytes, pbr_mse_stack_fit_workspace_bytes.
#include "ct_stack_host.hpp"

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

static const auto weighted_step_kernel = [](auto L, auto W, auto PGRAD, bool half_maps, int vec) { return pick_weighted_stack_step<L(), W(), PGRAD()>(half_maps, vec); };

}  // namespace pbr

extern "C" {

int pbr_cook_torrance_weighted_mse_stack_step(const pbr_render_desc *d, const void *targets, const void *weights, int64_t w_batch_stride,
                                              int64_t w_light_stride, void *g_albedo, void *g_normal, void *g_roughness, void *g_metallic,
                                              void *g_specular, void *loss, void *workspace, void *stream) {
    using namespace pbr;
    return stack_loss_step<kOrthographic, true>(d, false, weighted_step_kernel,
                                                {targets, g_albedo, g_normal, g_roughness, g_metallic, g_specular, nullptr, loss, workspace, stream, {},
                                                 {static_cast<const float *>(weights), w_batch_stride, w_light_stride}});
}

int pbr_cook_torrance_weighted_mse_stack_fit_step(const pbr_render_desc *d, const void *targets, const void *weights, int64_t w_batch_stride,
                                                  int64_t w_light_stride, void *g_albedo, void *g_normal, void *g_roughness, void *g_metallic,
                                                  void *g_specular, void *g_params, void *loss, void *workspace, void *stream) {
    using namespace pbr;
    return stack_loss_step<kOrthographic, true>(d, true, weighted_step_kernel,
                                                {targets, g_albedo, g_normal, g_roughness, g_metallic, g_specular, g_params, loss, workspace, stream, {},
                                                 {static_cast<const float *>(weights), w_batch_stride, w_light_stride}});
}

}  // extern "C"
