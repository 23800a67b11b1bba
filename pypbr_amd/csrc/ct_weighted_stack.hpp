// ct_weighted_stack.hpp -- what the weighted light-stack loss steps share (ct_stack_weighted.hip, ct_camera_stack_weighted.hip,
// ct_view_stack_weighted.hip): a capture with a mask.  loss = mean over all 3 B L H W elements of w (image - target)^2, with one weight per
// pixel and shot (or one plane for all shots), the same for the three channels; N stays 3 B L H W, the sum of the weights is not used.
//
// The kernels are siblings of the unweighted steps: the same bodies (ct_backward.hpp: loss_step; ct_camera_stack.hpp) with the
// WeightedStackMseLoss policy, in translation units of their own.  The weights travel beside the descriptor: a pointer and two strides in
// elements, kernel arguments.  Bytes per pixel (fp32 maps, metallic workflow): 64 + 16 L with a plane per shot, 68 + 12 L with one plane.
#pragma once
#include "ct_backward.hpp"
#include "ct_launch.hpp"

namespace pbr {

// weights + b * bs + l * ls + pix, fp32, in 64-bit arithmetic; ls is H W, or 0 for one plane shared by all shots
struct WArgs {
    const float *w;
    int64_t bs, ls;
};

// The light stride the kernels serve: a dense stack of planes, or one plane.
static int weights_shape(const pbr_render_desc *d, int64_t w_light_stride) {
    return w_light_stride == 0 || w_light_stride == (int64_t)d->height * d->width ? PBR_OK : PBR_ERR_SHAPE;
}

// What the weighted kernels of the camera families hand their body as `first_targets`: the weights' lane and the first loads.  A lane outside
// the map reads its clamped position (p.pix), the targets' and the weights' alike: in bounds.
template <int VEC>
__device__ __forceinline__ void weighted_first_loads(const LanePos &p, const WArgs &w, WeightedStackMseLoss<VEC> &loss) {
    loss.wlane = w.w + ((int64_t)p.b * w.bs + p.pix);
    loss.wstep = w.ls;
    loss.prefetch_first();
}

}  // namespace pbr
