// ct_loss.hip -- the rendering-loss step as ONE kernel (C ABI: pbr_cook_torrance_mse_step).
//
// The documented training use of the reference (docs/source/tutorials/06_advanced.rst:73-107) is
//     loss = nn.MSELoss()(brdf(predicted_material, ...), brdf(ground_truth_material, ...))
// followed by loss.backward().  The ground-truth rendering is a constant of the step (rendered once, by pbr_cook_torrance);
// what a step repeats for the PREDICTED material is: evaluate (44 B/pixel), subtract / square / mean and its backward
// (36 B/pixel of elementwise torch kernels), the backward kernel (76 B/pixel).  Here it is one pass: the predicted maps and the
// target image are read once (32 + 12 B/pixel), the colour is formed in registers, its difference to the target gives the
// pixel's share of the loss AND its upstream gradient 2 (out - target) / N, the chain rule runs back through the shading (the
// very code of cook_torrance_backward_kernel: backward_body_to with the MseLoss policy), and the four map gradients are
// written (32 B/pixel): 76 B/pixel instead of 156.
//
// The loss itself: every workgroup (one wave) leaves its sum of squared differences in a workspace row; a second small kernel
// adds the rows in fp64 in a fixed order (deterministic) and writes mean = sum / N.
//
// This file is also the home of what every loss step shares on the host -- this one and the two over light stacks (ct_stack.hip): an entry
// point is mse_gate, pick the kernel, launch_loss_step (ct_stack_host.hpp), mse_finish (declared in ct_launch.hpp).  What they share on the
// device is the frame loss_step (ct_backward.hpp, beside the loss policies): a step kernel is that frame with its policy and its first target loads.
#include "ct_backward_stream.hpp"
#include "ct_stack_host.hpp"

namespace pbr {


// Waves per SIMD the register allocation must leave room for: the packed pair for fp16 maps fits 128 VGPRs (four waves) in the
// backward kernel, not here -- the target pixels and the squared differences come on top (56 bytes of scratch): three waves.
template <int VEC, bool MULTI, typename TM>
constexpr int mse_min_waves() { return VEC == 2 && !MULTI && sizeof(TM) == 2 ? 3 : 1; }

template <int LIGHT, int WF, int VEC, bool MULTI, typename TM>
__global__ __launch_bounds__(64) __attribute__((amdgpu_waves_per_eu(mse_min_waves<VEC, MULTI, TM>())))
void cook_torrance_mse_step_kernel(const KArgs a, const BArgs b, const float *__restrict__ target, float scale, float *__restrict__ partials) {
    loss_step<LIGHT, WF, VEC, MULTI, TM, false, MseLoss<VEC>>(a, b, nullptr, 0, partials, [&](const LanePos &p, MseLoss<VEC> &loss) {
        loss.scale = scale;
        const int64_t opix = p.b * a.o_bs + p.pix;
#pragma unroll
        for (int c = 0; c < 3; ++c) Ld<float, VEC>::template load<true>(target, opix + c * a.o_cs, loss.tgt[c]);
    });
}

// The streamed form (fp16 maps, one light, whole 128-pixel tiles: ct_backward.hip stream_run): cook_torrance_backward_stream_kernel's schedule --
// persistent one-wave workgroups, the next tile's texels AND target pixels prefetched global -> LDS by DMA -- with the MseLoss policy.
// The target image takes the upstream gradient's three fp32 planes in the tile buffer; a wave keeps ONE running sum over all its tiles.
// Two waves per SIMD: with the target pixels and the squared differences on top, the point-light / converted body does not fit the 168 VGPRs of
// three (8 bytes of scratch, and a compiler-inserted wait on the reload: tools/check_isa.py rejects it).
#ifndef PBR_MSE_STREAM_WAVES
#define PBR_MSE_STREAM_WAVES 2
#endif
template <int LIGHT, int WF, bool FULL>
__global__ __launch_bounds__(64) __attribute__((amdgpu_waves_per_eu(PBR_MSE_STREAM_WAVES)))
void cook_torrance_mse_stream_kernel(const KArgs a, const BArgs b, const int tiles_per_material, const int n_stores, float scale, float *__restrict__ partials) {
    __shared__ uint32_t buf[kStreamLdsWords];
    MseLoss<2> loss;
    loss.scale = scale;
    loss.sq = 0.0f;
    backward_stream_body<LIGHT, WF, FULL>(a, b, tiles_per_material, n_stores, buf, loss);
    const float total = wave_sum(loss.sq);
    if (threadIdx.x == 0) partials[blockIdx.y * gridDim.x + blockIdx.x] = total;
}

// partials[n] (fp32, one per workgroup of the step kernel) -> *loss = sum / count, in two stages, fp64, fixed order:
// kMseStageGroups workgroups each add a contiguous block of the partials (coalesced: lane t takes elements t, t + 256, ...) into
// stage[blockIdx]; then one workgroup adds the stage sums.  (One workgroup walking all 131 072 partials of a 4096^2 launch by
// itself took longer than the step kernel: the same lesson as the light-gradient finish kernel, ct_backward.hip.)
constexpr int kMseStageGroups = 256;
__device__ __forceinline__ double block_sum_256(double s, double *red) {
    red[threadIdx.x] = s;
    __syncthreads();
    for (int o = 128; o > 0; o >>= 1) {
        if ((int)threadIdx.x < o) red[threadIdx.x] += red[threadIdx.x + o];
        __syncthreads();
    }
    return red[0];
}
__global__ __launch_bounds__(256) void mse_stage_kernel(const float *__restrict__ partials, int n, double *__restrict__ stage) {
    __shared__ double red[256];
    const int per = (n + kMseStageGroups - 1) / kMseStageGroups;
    const int i0 = blockIdx.x * per, i1 = min(n, i0 + per);
    double s = 0.0;
    for (int i = i0 + threadIdx.x; i < i1; i += 256) s += partials[i];
    const double total = block_sum_256(s, red);
    if (threadIdx.x == 0) stage[blockIdx.x] = total;
}
__global__ __launch_bounds__(256) void mse_finish_kernel(const double *__restrict__ stage, double inv_count, float *__restrict__ loss) {
    __shared__ double red[256];
    const double total = block_sum_256(threadIdx.x < kMseStageGroups ? stage[threadIdx.x] : 0.0, red);
    if (threadIdx.x == 0) *loss = (float)(total * inv_count);
}

// x *= *scalar (device scalar), in place; returns at once when the scalar is exactly 1 (the usual upstream gradient of a loss)
template <typename T>
__global__ __launch_bounds__(256) void scale_by_device_scalar_kernel(T *__restrict__ x, size_t n, const float *__restrict__ scalar) {
    const float k = *scalar;
    if (k == 1.0f) return;
    const size_t stride = (size_t)gridDim.x * blockDim.x;
    for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += stride) x[i] = (T)((float)x[i] * k);
}

// few partials (the streamed step leaves one per resident wave, ~3 000): ONE workgroup adds them, fp64, fixed order -- one launch instead of two
__global__ __launch_bounds__(256) void mse_reduce_small_kernel(const float *__restrict__ partials, int n, double inv_count, float *__restrict__ loss) {
    __shared__ double red[256];
    double s = 0.0;
    for (int i = threadIdx.x; i < n; i += 256) s += partials[i];
    const double total = block_sum_256(s, red);
    if (threadIdx.x == 0) *loss = (float)(total * inv_count);
}
constexpr int kMseSmall = 16384;

// x_i *= *scalar for up to five buffers in ONE launch (the gradients of a step); returns at once when the scalar is exactly 1
struct ScaleList { void *data[5]; size_t n[5]; };
template <typename T>
__global__ __launch_bounds__(256) void scale_list_kernel(ScaleList l, const float *__restrict__ scalar) {
    const float k = *scalar;
    if (k == 1.0f) return;
    const size_t stride = (size_t)gridDim.x * blockDim.x, first = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
#pragma unroll
    for (int j = 0; j < 5; ++j) {
        T *x = static_cast<T *>(l.data[j]);
        for (size_t i = first; i < l.n[j]; i += stride) x[i] = (T)((float)x[i] * k);
    }
}

template <int L, int W>
static LossStepFn pick_mse(bool half_maps, int vec, bool multi) {
    if (half_maps) {
        if (vec == 2) return multi ? cook_torrance_mse_step_kernel<L, W, 2, true, __half> : cook_torrance_mse_step_kernel<L, W, 2, false, __half>;
        return multi ? cook_torrance_mse_step_kernel<L, W, 1, true, __half> : cook_torrance_mse_step_kernel<L, W, 1, false, __half>;
    }
    if (vec == 2) return multi ? cook_torrance_mse_step_kernel<L, W, 2, true, float> : cook_torrance_mse_step_kernel<L, W, 2, false, float>;
    return multi ? cook_torrance_mse_step_kernel<L, W, 1, true, float> : cook_torrance_mse_step_kernel<L, W, 1, false, float>;
}

using MseStreamFn = void (*)(const KArgs, const BArgs, int, int, float, float *);
static MseStreamFn pick_mse_stream(const pbr_render_desc *d, bool full) {
    return with_light_workflow(d, [&](auto L, auto W) -> MseStreamFn {
        return full ? cook_torrance_mse_stream_kernel<L(), W(), true> : cook_torrance_mse_stream_kernel<L(), W(), false>;
    });
}
// Pixels per lane: the loss is a sum over pixels, so no lane may see a pixel twice (the overlapping last lane of a ragged row,
// lane_pos: dup): two when the width is even, else one.  Two also for fp32 maps with one light, where the backward kernel takes
// four: with the target pixels on top the four-pixel body needs 256 VGPRs + 21 AGPRs (one wave per SIMD; held to two waves it
// spills 72-88 bytes), and measured on a 4096^2 material it loses -- point light 295 against 228 us, directional 225 against 219
// (tools/loss_step_probe.py, round 3).
int mse_vec(const pbr_render_desc *d) { return g_max_vec == 1 || (d->width & 1) ? 1 : 2; }

// workspace: the step kernel's partial sums (fp32, one per workgroup), then kMseStageGroups stage sums (fp64, 8-byte aligned)
static size_t mse_stage_offset(size_t tiles) { return (tiles * sizeof(float) + 7) & ~(size_t)7; }

static int64_t mse_tiles(const pbr_render_desc *d, int vec) {
    KArgs k;
    fill_args(d, vec, k, 6);
    return k.n_tiles;
}

// The step kernel's partial sums -> *loss = their sum / count (fp64, fixed order): one workgroup for few partials, else the stage sums and
// their sum.  Where the stage sums go does not depend on n_partials: the stage block sits behind the partials of the LARGEST
// decomposition of the descriptor -- mse_tiles(d, 1), or repeat_backward_tiles(d) for tiled maps -- which is what
// pbr_mse_step_workspace_bytes reserves.  `stage_offset_tiles()` returns that count; it is asked only when the stage block is used.
template <typename StageTiles>
static int finish_mse(float *partials, int64_t n_partials, StageTiles &&stage_offset_tiles, double count, float *loss, hipStream_t st) {
    if (n_partials <= kMseSmall) {
        hipLaunchKernelGGL(mse_reduce_small_kernel, dim3(1), dim3(256), 0, st, partials, (int)n_partials, 1.0 / count, loss);
    } else {
        double *stage = reinterpret_cast<double *>(reinterpret_cast<char *>(partials) + mse_stage_offset((size_t)stage_offset_tiles()));
        hipLaunchKernelGGL(mse_stage_kernel, dim3(kMseStageGroups), dim3(256), 0, st, partials, (int)n_partials, stage);
        hipLaunchKernelGGL(mse_finish_kernel, dim3(1), dim3(256), 0, st, stage, 1.0 / count, loss);
    }
    return launch_status();
}

// For untiled maps, the light-stack steps (ct_stack.hip) included: the stage block behind the partials of one pixel per lane, the most workgroups
// any launch of this descriptor has.
int mse_finish(const pbr_render_desc *d, float *partials, int64_t n_partials, double count, float *loss, hipStream_t st) {
    return finish_mse(partials, n_partials, [&] { return mse_tiles(d, 1); }, count, loss, st);
}

// What every loss step asks before anything else, in this order: a valid descriptor, the caller's pointers, an fp32 result (the target image and
// the colour it is compared with are fp32), no NaN grid, and untiled maps -- unless the step has a tiled form (`tiled_form`) that serves them.
int mse_gate(const pbr_render_desc *d, bool pointers_given, bool tiled_form) {
    const int rc = validate(d);
    if (rc != PBR_OK) return rc;
    if (!pointers_given) return PBR_ERR_NULL_MAP;
    if (d->out_dtype != PBR_F32) return PBR_ERR_DTYPE;
    if (nan_light_size(d) || (is_tiled(d) && !(tiled_form && repeat_loss_serves(d)))) return PBR_ERR_UNSUPPORTED;
    return PBR_OK;
}

}  // namespace pbr

extern "C" {

size_t pbr_mse_step_workspace_bytes(const pbr_render_desc *d) {
    const pbr::TuningScope tuning(d);
    if (pbr::validate(d) != PBR_OK) return 0;
    if (pbr::is_tiled(d) && !pbr::repeat_loss_serves(d)) return 0;
    // tiled maps: one partial sum per workgroup of the repeat-inner kernel; else one pixel per lane: the most workgroups any launch of this descriptor has
    const int64_t tiles = pbr::is_tiled(d) ? pbr::repeat_backward_tiles(d) : pbr::mse_tiles(d, 1);
    return tiles < 0 ? 0 : pbr::mse_stage_offset((size_t)tiles) + (size_t)pbr::kMseStageGroups * sizeof(double);
}

int pbr_cook_torrance_mse_step(const pbr_render_desc *d, const void *target, void *g_albedo, void *g_normal, void *g_roughness,
                               void *g_metallic, void *g_specular, void *loss, void *workspace, void *stream) {
    const pbr::TuningScope tuning(d);
    using namespace pbr;
    const int rc = mse_gate(d, target && loss && workspace, true);
    if (rc != PBR_OK) return rc;
    KArgs k;
    const double count = 3.0 * (double)d->batch * (double)d->height * (double)d->width;
    hipStream_t st = static_cast<hipStream_t>(stream);
    float *const partials = static_cast<float *>(workspace);      // one per workgroup of the step kernel; the stage sums behind them (finish_mse)
    if (is_tiled(d)) {
        // MaterialBase.tile fused (base.py:524-537): the repeat-inner kernel walks the maps, compares every repeat with the target and leaves
        // MAP-sized gradients (ct_repeat_backward.hpp); launches it does not serve are the caller's to split (render, loss, folded backward)
        const int64_t tiles = repeat_backward_tiles(d);
        if (tiles < 0) return PBR_ERR_SHAPE;
        const int e = launch_repeat_backward(d, target, g_albedo, g_normal, g_roughness, g_metallic, g_specular, true, (float)(2.0 / count),
                                             partials, st);
        if (e != PBR_OK) return e;
        return finish_mse(partials, tiles, [&] { return tiles; }, count, static_cast<float *>(loss), st);      // (tiles = repeat_backward_tiles(d))
    }
    void *const gs[5] = {g_albedo, g_normal, g_roughness, g_metallic, g_specular};
    int e;
    int64_t n_partials;
    if (const int rounds = g_mse_stream ? stream_run(d, target, gs) : 0) {      // fp16 maps, one light: the streamed form
        // (the allocator is ALLOWED two waves per SIMD and lands on 138-167 VGPRs: three fit, and the grid is sized for three)
        const StreamLaunch s = stream_launch_shape(d, gs, rounds, k);
        const BArgs b = {target, g_albedo, g_normal, g_roughness, g_metallic, g_specular, nullptr};
        n_partials = s.per_material * d->batch;                         // <= tiles * batch <= the workgroups of the one-tile form
        hipLaunchKernelGGL(pick_mse_stream(d, s.full), dim3((unsigned)s.per_material, (unsigned)d->batch, 1), dim3(64, 1, 1), 0, st, k, b, s.tiles,
                           s.n_stores, (float)(2.0 / count), partials);
        e = launch_status();
    } else {
        const BArgs b = {nullptr, g_albedo, g_normal, g_roughness, g_metallic, g_specular, nullptr};
        const int vec = mse_vec(d);
        const bool multi = d->n_lights > 1, half_maps = d->map_dtype == PBR_F16;
        const LossStepFn fn = with_light_workflow(d, [&](auto L, auto W) -> LossStepFn { return pick_mse<L(), W()>(half_maps, vec, multi); });
        e = launch_loss_step(d, fill_args, fn, vec, b, target, count, partials, st, k);
        n_partials = k.n_tiles;
    }
    return e != PBR_OK ? e : mse_finish(d, partials, n_partials, count, static_cast<float *>(loss), st);
}

int pbr_scale_by_device_scalar(void *data, size_t n, int dtype, const void *scalar, void *stream) {
    using namespace pbr;
    if (!data || !scalar) return PBR_ERR_NULL_MAP;
    if (dtype != PBR_F32 && dtype != PBR_F16) return PBR_ERR_DTYPE;
    if (n == 0) return PBR_OK;
    const unsigned grid = stream_grid(n);
    hipStream_t st = static_cast<hipStream_t>(stream);
    if (dtype == PBR_F32) hipLaunchKernelGGL((scale_by_device_scalar_kernel<float>), dim3(grid), dim3(256), 0, st, static_cast<float *>(data), n, static_cast<const float *>(scalar));
    else hipLaunchKernelGGL((scale_by_device_scalar_kernel<_Float16>), dim3(grid), dim3(256), 0, st, static_cast<_Float16 *>(data), n, static_cast<const float *>(scalar));
    return launch_status();
}

int pbr_scale_list_by_device_scalar(void *const *data, const size_t *n, int count, int dtype, const void *scalar, void *stream) {
    using namespace pbr;
    if (!data || !n || !scalar) return PBR_ERR_NULL_MAP;
    if (count < 0 || count > 5) return PBR_ERR_SHAPE;
    if (dtype != PBR_F32 && dtype != PBR_F16) return PBR_ERR_DTYPE;
    ScaleList l = {};
    size_t most = 0;
    for (int j = 0; j < count; ++j) {
        if (n[j] && !data[j]) return PBR_ERR_NULL_MAP;
        l.data[j] = data[j]; l.n[j] = n[j];
        most = n[j] > most ? n[j] : most;
    }
    if (most == 0) return PBR_OK;
    const unsigned grid = stream_grid(most);
    hipStream_t st = static_cast<hipStream_t>(stream);
    if (dtype == PBR_F32) hipLaunchKernelGGL((scale_list_kernel<float>), dim3(grid), dim3(256), 0, st, l, static_cast<const float *>(scalar));
    else hipLaunchKernelGGL((scale_list_kernel<_Float16>), dim3(grid), dim3(256), 0, st, l, static_cast<const float *>(scalar));
    return launch_status();
}

}  // extern "C"
