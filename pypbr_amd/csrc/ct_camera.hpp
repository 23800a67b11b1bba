// ct_camera.hpp -- what the perspective camera's translation units share (ct_camera.hip: the render and its backward; ct_camera_stack.hip:
// the light-stack forms): where a kernel reads the camera position, and on the host the gate, the NaN-grid test and the kernel arguments
// with the view left as the position.
#pragma once
#include "ct_backward.hpp"
#include "ct_launch.hpp"

namespace pbr {

// The camera position of a launch: the kernel arguments' V (which the launchers fill with the position AS GIVEN, not normalised), or the
// device block's raw_view when the parameters live in device memory.  Wave-uniform.
__device__ __forceinline__ Vec3 camera_of(const KArgs &a) {
    if (a.dev) { const DevParamsPtr d = dev_params(a.dev); return Vec3{d->raw_view[0], d->raw_view[1], d->raw_view[2]}; }
    return Vec3{a.V[0], a.V[1], a.V[2]};
}

// What the camera's entry points ask before any launch: a valid descriptor, untiled maps (there is no tiled or blended camera form), an fp32 result.
static int camera_gate(const pbr_render_desc *d) {
    const int rc = validate(d);
    if (rc != PBR_OK) return rc;
    if (d->map_height || d->map_width) return PBR_ERR_UNSUPPORTED;
    if (d->out_dtype != PBR_F32) return PBR_ERR_DTYPE;
    return PBR_OK;
}
// A NaN light_size makes the grid, hence every view vector, NaN whatever the light type (ct_launch.hpp: nan_light_size is the point light's).
static bool nan_grid(const pbr_render_desc *d) { return d->light_size != d->light_size; }

// What the camera's loss steps (ct_camera_stack.hip, ct_view_stack.hip) ask before any launch: the loss steps' gate (valid descriptor, the caller's pointers, an fp32 result, untiled maps) and
// what the camera adds to it -- no map size at all (camera_gate), no NaN grid whatever the light type.
static int camera_step_gate(const pbr_render_desc *d, bool pointers_given) {
    int rc = mse_gate(d, pointers_given, false);
    if (rc == PBR_OK) rc = camera_gate(d);
    if (rc != PBR_OK) return rc;
    return nan_grid(d) ? PBR_ERR_UNSUPPORTED : PBR_OK;
}

// fill_args, with the view as the kernels read it here: the position as given (fill_args normalises it for the orthographic kernels)
static void camera_args(const pbr_render_desc *d, int vec, KArgs &k, int block_log2) {
    fill_args(d, vec, k, block_log2);
    for (int c = 0; c < 3; ++c) k.V[c] = d->view_dir[c];
}

}  // namespace pbr
