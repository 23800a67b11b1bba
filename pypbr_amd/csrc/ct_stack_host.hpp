// ct_stack_host.hpp -- the host side that the loss steps and the light stacks share, once: the launch of a one-wave loss step
// (launch_loss_step: ct_loss.hip's single-image step and every light-stack step), the body of the twelve light-stack loss steps
// (stack_loss_step), of the three forward stacks (launch_stack) and of the three fit-size queries (stack_fit_workspace_bytes).  A translation
// unit keeps its kernels, its pick_* functions and its extern "C" signatures; an entry point names its family and forwards.  A new form of the
// step is a kernel, its pick and such a forward -- not another copy of this sequence.
#pragma once
#include "ct_camera_stack.hpp"
#include "ct_weighted_stack.hpp"

namespace pbr {

// How a launch fills its kernel arguments: fill_args (ct_launch.hpp: the view normalised, for the orthographic kernels) or camera_args
// (ct_camera.hpp: the view left as the position).
using ArgsFn = void (*)(const pbr_render_desc *, int, KArgs &, int);

// The launch of a one-wave loss step (ct_backward.hpp: loss_step; ct_camera_stack.hpp): `vec` pixels per lane (mse_vec) in 64-lane workgroups,
// one partial sum per workgroup, no LDS reduction; target and gradient planes are contiguous (the stack's strides follow from o_cs and
// n_lights); scale = 2 / count.  With a row of light / view sums per workgroup (b.g_param_partials) never more workgroups than the size query
// promised.  `beside`: what the kernel takes between BArgs and the targets (the shots' positions, the weights), as kernel arguments of their
// own.  Leaves the launch's KArgs in `k` (n_tiles = the partial sums to finish, dev for the rows' finish).
template <class Fn, class... Beside>
static int launch_loss_step(const pbr_render_desc *d, ArgsFn args, Fn fn, int vec, const BArgs &b, const void *targets, double count,
                            float *partials, hipStream_t st, KArgs &k, const Beside &...beside) {
    args(d, vec, k, 6);
    if (k.n_tiles < 0) return PBR_ERR_SHAPE;
    if (b.g_param_partials) {
        const int64_t most = max_tiles(d);
        if (most < 0 || k.n_tiles > most) return PBR_ERR_SHAPE;
    }
    k.o_cs = (int64_t)d->height * d->width; k.o_bs = 3 * k.o_cs;
    hipLaunchKernelGGL(fn, dim3((unsigned)k.n_tiles, 1, 1), dim3(64, 1, 1), 0, st, k, b, beside..., static_cast<const float *>(targets), (float)(2.0 / count), partials);
    return launch_status();
}

// ------------------------------------------------------------------ the twelve light-stack loss steps
// A family is its view and whether the call has weights; the view says which gate, which kernel arguments and which rows finish:
//   kOrthographic  one view direction: mse_gate, fill_args, rows of 3 + 6 L (param_grad_finish)
//   kCamera        view_dir is the camera position: camera_step_gate, camera_args, the same rows with the view's taken as a position
//   kShotCameras   one position per shot, beside the descriptor (exactly one of host / device): ViewArgs, rows of 9 L (param_rows_finish)
enum StackView { kOrthographic, kCamera, kShotCameras };

// What a step's caller hands over beside the descriptor.  g_params: the fit step's; cameras: kShotCameras'; weights: the weighted forms'.
struct ShotCameras { const float *host; const void *device; };
struct StepCall {
    const void *targets;
    void *g_albedo, *g_normal, *g_roughness, *g_metallic, *g_specular, *g_params, *loss, *workspace, *stream;
    ShotCameras cameras;
    WArgs weights;
};

// `pick(L, W, PGRAD, half_maps, vec)`: the family's kernel for integral constants L, W and PGRAD (the translation unit's pick_* function).
// `fit`: the fit step -- g_params is asked for, the kernel leaves rows behind the loss part of the workspace, and they are finished.
template <int VIEW, bool WEIGHTED, class Pick>
static int stack_loss_step(const pbr_render_desc *d, bool fit, Pick pick, const StepCall &c) {
    const TuningScope tuning(d);
    const bool pointers = (!fit || c.g_params) && c.targets && (!WEIGHTED || c.weights.w) && c.loss && c.workspace &&
                          (VIEW != kShotCameras || one_camera_source(c.cameras.host, c.cameras.device));
    int rc = VIEW == kOrthographic ? mse_gate(d, pointers, false) : camera_step_gate(d, pointers);
    if (rc == PBR_OK && WEIGHTED) rc = weights_shape(d, c.weights.ls);
    if (rc != PBR_OK) return rc;
    const int vec = mse_vec(d);
    const bool half_maps = d->map_dtype == PBR_F16;
    const auto fn = with_light_workflow(d, [&](auto L, auto W) {
        return fit ? pick(L, W, std::true_type{}, half_maps, vec) : pick(L, W, std::false_type{}, half_maps, vec);
    });
    const double count = 3.0 * (double)d->batch * (double)d->n_lights * (double)d->height * (double)d->width;
    hipStream_t st = static_cast<hipStream_t>(c.stream);
    float *const partials = static_cast<float *>(c.workspace);
    float *const rows = fit ? reinterpret_cast<float *>(static_cast<char *>(c.workspace) + pbr_mse_step_workspace_bytes(d)) : nullptr;      // one row per workgroup
    const BArgs b = {nullptr, c.g_albedo, c.g_normal, c.g_roughness, c.g_metallic, c.g_specular, rows};
    KArgs k;
    const auto launch = [&](const auto &...beside) {
        return launch_loss_step(d, VIEW == kOrthographic ? ArgsFn(fill_args) : ArgsFn(camera_args), fn, vec, b, c.targets, count, partials, st, k, beside...);
    };
    int e;
    if constexpr (VIEW == kShotCameras && WEIGHTED) e = launch(view_args(d, c.cameras.host, c.cameras.device), c.weights);
    else if constexpr (VIEW == kShotCameras) e = launch(view_args(d, c.cameras.host, c.cameras.device));
    else if constexpr (WEIGHTED) e = launch(c.weights);
    else e = launch();
    if (e == PBR_OK && fit) {
        float *const g_params = static_cast<float *>(c.g_params);
        e = VIEW == kShotCameras ? param_rows_finish(d, rows, k.n_tiles, 3 * d->n_lights, d->n_lights, k.dev, g_params, st)
                                 : param_grad_finish(d, rows, k.n_tiles, k.dev, g_params, st, VIEW == kCamera);
    }
    return e != PBR_OK ? e : mse_finish(d, partials, k.n_tiles, count, static_cast<float *>(c.loss), st);
}

// The three fit-size queries: the loss partials and their stage sums, then one row of `fixed + per_light L` floats per workgroup of the largest
// decomposition, then the rows' stage sums.  `served`: the family's gate passes with every pointer given; 0 bytes for what the step refuses.
static size_t stack_fit_workspace_bytes(const pbr_render_desc *d, bool served, int fixed, int per_light) {
    if (!served) return 0;
    const size_t loss_part = pbr_mse_step_workspace_bytes(d);
    const int n_param = fixed + per_light * d->n_lights;
    return loss_part == 0 ? 0 : loss_part + param_rows_bytes_of(d, n_param) + param_stage_bytes_of(n_param);
}

// ------------------------------------------------------------------ the three forward stacks
// Behind the entry point's own gate: the stack is one contiguous block of [B][L][3][H][W] fp32; `nan`: every value of every image is NaN
// upstream (a NaN grid: ct_launch.hpp nan_light_size, ct_camera.hpp nan_grid), written directly; else four pixels per lane where a row holds
// them -- ragged widths: the last lane of a row overlaps its neighbour (lane_pos) -- and a.o_bs the MATERIAL's stride in the stack.
// `pick(L, W, half_maps, vec)`: the family's kernel; `beside`: what it takes behind KArgs (the shots' positions).
template <class Pick, class... Beside>
static int launch_stack(const pbr_render_desc *d, bool nan, ArgsFn args, Pick pick, void *stream, const Beside &...beside) {
    if (d->out_batch_stride != 0 || d->out_channel_stride != 0) return PBR_ERR_UNSUPPORTED;
    hipStream_t st = static_cast<hipStream_t>(stream);
    const int64_t plane = (int64_t)d->height * d->width;
    if (nan) return call_status(hipMemsetD32Async((hipDeviceptr_t)d->out, 0x7fc00000, (size_t)(plane * 3 * d->n_lights * d->batch), st));
    const int vec = (g_max_vec == 1 || d->width < 4) ? 1 : 4;
    KArgs k;
    args(d, vec, k, 0);
    if (k.n_tiles < 0) return PBR_ERR_SHAPE;
    k.o_cs = plane; k.o_bs = 3 * plane * d->n_lights;
    const bool half_maps = d->map_dtype == PBR_F16;
    const auto fn = with_light_workflow(d, [&](auto L, auto W) { return pick(L, W, half_maps, vec); });
    hipLaunchKernelGGL(fn, dim3((unsigned)k.n_tiles, 1, 1), dim3(1u << k.bt_log2, 1, 1), 0, st, k, beside...);
    return launch_status();
}

}  // namespace pbr
