// ct_backward.hip -- launchers of the backward kernels (C ABI: pbr_cook_torrance_backward, pbr_cook_torrance_backward_params);
// device code in ct_backward.hpp (the one-tile kernel) and ct_backward_stream.hpp (the streamed one); the two reduction kernels behind the
// light / view gradients are not templates and live here.
#include "ct_backward_stream.hpp"
#include "ct_launch.hpp"

namespace pbr {

// Adds up the per-workgroup rows of the PGRAD kernels (fp64 sums, fixed order: deterministic) and applies the part of
// the chain rule that sits in front of the kernel: view_dir and a directional light enter through F.normalize
// (cooktorrance.py:95, :126), whose Jacobian is (I - v v^T) / max(|x|, 1e-12).  One workgroup per 3-vector:
// vector 0 = view, 1..L = lights, L+1..2L = intensities.  out: [3 + 6 L] floats in that order.
// Stage 1 of the row sum: kParamStageRows workgroups, each adds a contiguous block of rows.  The rows are read as one flat
// array, lane t taking elements t, t + T, t + 2 T ... with T the largest multiple of n_param <= 256, so a lane always
// meets the same parameter and the loads are coalesced; fp64, fixed order.  (One workgroup per 3-vector walking all
// 131 072 rows of a 4096^2 launch by itself took 155 us -- as long as the kernel that produced them.)
constexpr int kParamStageRows = 256;
__global__ __launch_bounds__(256) void param_grad_stage_kernel(const float *__restrict__ partials, double *__restrict__ stage,
                                                               int n_rows, int n_param) {
    const int T = (256 / n_param) * n_param, per = (n_rows + kParamStageRows - 1) / kParamStageRows;
    const int r0 = blockIdx.x * per, r1 = min(n_rows, r0 + per);
    __shared__ double part[256];
    double s = 0.0;
    if ((int)threadIdx.x < T && r0 < r1) {
        const float *p = partials + (int64_t)r0 * n_param;
        const int64_t n = (int64_t)(r1 - r0) * n_param;
        for (int64_t e = threadIdx.x; e < n; e += T) s += p[e];
    }
    part[threadIdx.x] = s;
    __syncthreads();
    if ((int)threadIdx.x < n_param) {
        double t = 0.0;
        for (int k = threadIdx.x; k < T; k += n_param) t += part[k];
        stage[(int64_t)blockIdx.x * n_param + threadIdx.x] = t;
    }
}

struct ParamFinishArgs {
    const double *stage; float *out; int32_t n_rows, n_lights, light_type;      // n_rows = kParamStageRows rows of stage sums
    float view[3]; float lights[PBR_MAX_LIGHTS][3];
    uint64_t dev;                     // parameters in device memory (address of the DevParams block): the raw vectors come from it
};
// VIEW_IS_POSITION: vector 0 is a camera position (ct_camera.hip) -- its normalisation Jacobian depends on the pixel and was applied there,
// before the sum: the rows hold the finished gradient, only summed here.
template <bool VIEW_IS_POSITION>
__global__ __launch_bounds__(256) void param_grad_finish_kernel(const ParamFinishArgs a) {
    const int vec = blockIdx.x, n_param = 3 + 6 * a.n_lights;
    double s[3] = {0.0, 0.0, 0.0};
    for (int r = threadIdx.x; r < a.n_rows; r += 256) {
        const double *row = a.stage + (int64_t)r * n_param + 3 * vec;
        s[0] += row[0]; s[1] += row[1]; s[2] += row[2];
    }
    __shared__ double red[3][256];
#pragma unroll
    for (int j = 0; j < 3; ++j) red[j][threadIdx.x] = s[j];
    __syncthreads();
    for (int o = 128; o > 0; o >>= 1) {
        if ((int)threadIdx.x < o) {
#pragma unroll
            for (int j = 0; j < 3; ++j) red[j][threadIdx.x] += red[j][threadIdx.x + o];
        }
        __syncthreads();
    }
    if (threadIdx.x != 0) return;
    double g[3] = {red[0][0], red[1][0], red[2][0]};
    const bool normalised = vec == 0 ? !VIEW_IS_POSITION : (vec <= a.n_lights && a.light_type == PBR_LIGHT_DIRECTIONAL);
    if (normalised) {
        float x[3];
        if (a.dev) {
            const DevParams *d = reinterpret_cast<const DevParams *>(a.dev);
            for (int j = 0; j < 3; ++j) x[j] = vec == 0 ? d->raw_view[j] : d->raw_lights[vec - 1][j];
        } else {
            for (int j = 0; j < 3; ++j) x[j] = vec == 0 ? a.view[j] : a.lights[vec - 1][j];
        }
        const double nrm = sqrt((double)x[0] * x[0] + (double)x[1] * x[1] + (double)x[2] * x[2]);
        if (nrm > 1e-12) {
            const double u[3] = {x[0] / nrm, x[1] / nrm, x[2] / nrm};
            const double ug = u[0] * g[0] + u[1] * g[1] + u[2] * g[2];
            for (int j = 0; j < 3; ++j) g[j] = (g[j] - u[j] * ug) / nrm;
        } else {                     // F.normalize divides by the clamp there: d(x / 1e-12)/dx
            for (int j = 0; j < 3; ++j) g[j] *= 1e12;
        }
    }
    for (int j = 0; j < 3; ++j) a.out[3 * vec + j] = (float)g[j];
}

using BwdFn = void (*)(const KArgs, const BArgs);

// Pixels per lane are a RULE since ABI 8 (launch_backward): four for the map gradients alone -- two for fp16 maps under one light --, two with the
// light / view adjoints (PG), one for rows shorter than four pixels.  The bodies only the closed A/B knob reached (two pixels for fp32 maps
// without PG, four for fp16 maps under one light) and the one nothing reached (four pixels with PG: 256 VGPRs + 40 AGPRs) are not built.
template <int L, int W, typename T, bool PG>
static BwdFn pick_bwd_variant(int vec, bool multi) {
    if (vec == 1) return multi ? cook_torrance_backward_kernel<L, W, 1, true, T, PG> : cook_torrance_backward_kernel<L, W, 1, false, T, PG>;
    if constexpr (PG) {
        return multi ? cook_torrance_backward_kernel<L, W, 2, true, T, PG> : cook_torrance_backward_kernel<L, W, 2, false, T, PG>;
    } else if constexpr (sizeof(T) == 2) {
        if (multi) return cook_torrance_backward_kernel<L, W, 4, true, T, PG>;
        return cook_torrance_backward_kernel<L, W, 2, false, T, PG>;
    } else {
        return multi ? cook_torrance_backward_kernel<L, W, 4, true, T, PG> : cook_torrance_backward_kernel<L, W, 4, false, T, PG>;
    }
}

template <bool PG>
static BwdFn pick_bwd(const pbr_render_desc *d, int vec) {
    const bool multi = d->n_lights > 1, half_maps = d->map_dtype == PBR_F16;
    return with_light_workflow(d, [&](auto L, auto W) -> BwdFn {
        return half_maps ? pick_bwd_variant<L(), W(), __half, PG>(vec, multi) : pick_bwd_variant<L(), W(), float, PG>(vec, multi);
    });
}

using BwdStreamFn = void (*)(const KArgs, const BArgs, int, int);
static BwdStreamFn pick_bwd_stream(const pbr_render_desc *d, bool full) {
    return with_light_workflow(d, [&](auto L, auto W) -> BwdStreamFn {
        return full ? cook_torrance_backward_stream_kernel<L(), W(), true> : cook_torrance_backward_stream_kernel<L(), W(), false>;
    });
}

// Rounds of the streamed backward kernel (ct_backward_stream.hpp: its grid is rounds x the waves the chip holds at once), or 0 when
// the launch does not qualify: fp16 maps, one light, untiled, rows a whole number of 128-pixel tiles, 4-byte aligned planes
// with even strides (its loads and stores move two fp16 values per lane).  g_bwd_run: -1 = rule, 0 = never, N = N rounds (A/B).
int stream_run(const pbr_render_desc *d, const void *grad_out, void *const g[5]) {
    if (g_bwd_run == 0 || d->map_dtype != PBR_F16 || d->n_lights != 1 || is_tiled(d) || d->width % 128) return 0;
    if ((int64_t)d->height * d->width >= (1ll << 30) || d->batch > 65535) return 0;
    auto ok = [](const pbr_map &m) {
        return !m.data || (is_aligned(m.data, 4) && m.batch_stride % 2 == 0 && m.channel_stride % 2 == 0);
    };
    if (!ok(d->albedo) || !ok(d->normal) || !ok(d->roughness) || !ok(d->metallic) || !ok(d->specular)) return 0;
    if (!is_aligned(grad_out, 4)) return 0;
    for (int i = 0; i < 5; ++i)
        if (!is_aligned(g[i], 4)) return 0;
    return g_bwd_run > 0 ? g_bwd_run : 4;          // 4096^2: 1 round 144-146 us, 2: 140-141, 4: 137-139, 6: 138, 8: 139-140 (tools/bwd_stream_ab.sh)
}

// The shape of a streamed launch that stream_run admitted, for the backward kernel and the loss step alike: `k` for two pixels per lane with
// contiguous upstream / target and gradient planes; g = the five gradient pointers (NULL = not wanted).
StreamLaunch stream_launch_shape(const pbr_render_desc *d, void *const g[5], int rounds, KArgs &k) {
    fill_args(d, 2, k, 6);
    k.o_cs = (int64_t)d->height * d->width; k.o_bs = 3 * k.o_cs;
    StreamLaunch s;
    s.tiles = (int)(k.o_cs / 128);
    const bool spec = d->workflow == PBR_WORKFLOW_SPECULAR;
    s.n_stores = (g[0] ? 3 : 0) + (g[1] && d->normal.data ? 3 : 0) + (g[2] ? 1 : 0) + (spec ? (g[4] ? 3 : 0) : (g[3] ? 1 : 0));
    // every run-time flag on and every gradient wanted: the instantiation without flag branches
    s.full = d->albedo_is_srgb && d->return_srgb && d->normal.data && g[0] && g[1] && g[2] &&
             (spec ? (g[4] && d->specular_is_srgb) : (g[3] && (d->workflow == PBR_WORKFLOW_METALLIC || d->specular_is_srgb)));
    // one-wave workgroups, kStreamWavesPerSimd of them per SIMD: the grid covers the chip `rounds` times, split over the materials
    const int64_t slots = (int64_t)resident_cus() * 4 * kStreamWavesPerSimd * rounds;
    s.per_material = (slots + d->batch - 1) / d->batch;
    if (s.per_material > s.tiles) s.per_material = s.tiles;
    if (s.per_material < 1) s.per_material = 1;
    return s;
}

// Tiles of the decomposition with the smallest tiles -- one pixel per lane, 64-lane workgroups: the most any launch of
// this descriptor can have whatever the tuning knobs say (more pixels per lane or larger workgroups only merge tiles).
// Same geometry as fill_args: bx = lanes along x (a power of two covering the row, at most 64), 64 / bx rows per tile.
int64_t max_tiles(const pbr_render_desc *d) {
    int lg = 0;
    while ((1 << lg) < d->width && lg < 6) ++lg;
    const int64_t bx = 1ll << lg, by = 64 >> lg, rows = (int64_t)d->batch * d->height;
    const int64_t tiles = ((d->width + bx - 1) / bx) * ((rows + by - 1) / by);
    return tiles > INT32_MAX ? -1 : tiles;
}

// Workspace of the light / view gradients: max_tiles rows of partial sums (fp32), then kParamStageRows rows of stage sums (fp64).
size_t param_rows_bytes(const pbr_render_desc *d) {
    const size_t rows = (size_t)max_tiles(d) * (size_t)(3 + 6 * d->n_lights) * sizeof(float);
    return (rows + 7) & ~(size_t)7;
}
size_t param_stage_bytes(const pbr_render_desc *d) { return (size_t)kParamStageRows * (size_t)(3 + 6 * d->n_lights) * sizeof(double); }

// The finish of the light / view gradients, for every kernel that leaves rows (pbr_cook_torrance_backward_params, the stack-fit step of
// ct_stack.hip): `rows` = n_rows rows of 3 + 6 L partial sums with their stage block param_rows_bytes(d) further on -> g_params, through the two
// reduction kernels (fp64, fixed order, the F.normalize Jacobians; `dev`: KArgs::dev, the parameters in device memory;
// `view_is_position`: param_grad_finish_kernel's VIEW_IS_POSITION).
int param_grad_finish(const pbr_render_desc *d, const float *rows, int n_rows, uint64_t dev, float *g_params, hipStream_t st, bool view_is_position) {
    ParamFinishArgs f;
    std::memset(&f, 0, sizeof(f));
    const int n_param = 3 + 6 * d->n_lights;
    double *stage = reinterpret_cast<double *>(reinterpret_cast<char *>(const_cast<float *>(rows)) + param_rows_bytes(d));
    hipLaunchKernelGGL(param_grad_stage_kernel, dim3(kParamStageRows), dim3(256), 0, st, rows, stage, n_rows, n_param);
    f.stage = stage; f.out = g_params;
    f.n_rows = kParamStageRows; f.n_lights = d->n_lights; f.light_type = d->light_type;
    f.dev = dev;
    for (int c = 0; c < 3; ++c) f.view[c] = d->view_dir[c];
    for (int i = 0; i < d->n_lights; ++i)
        for (int c = 0; c < 3; ++c) f.lights[i][c] = d->lights[i][c];
    hipLaunchKernelGGL(view_is_position ? param_grad_finish_kernel<true> : param_grad_finish_kernel<false>, dim3(1u + 2u * (unsigned)d->n_lights),
                       dim3(256), 0, st, f);
    return launch_status();
}

// ------------------------------------------------------------------ rows of any length (ct_view_stack.hip: 9 L floats, one camera per shot)
// param_grad_finish's sibling: a row is n_vec 3-vectors, of which vectors [first_light, first_light + L) are the lights' -- directional ones
// pass through F.normalize's Jacobian as above -- and every other vector is only summed (camera positions: their Jacobian depends on the pixel
// and was applied before the sum; intensities).  Stage 1 is param_grad_stage_kernel itself: it takes the row length as an argument.
struct RowsFinishArgs {
    const double *stage; float *out; int32_t n_rows, n_vec, first_light, n_lights, light_type;
    float lights[PBR_MAX_LIGHTS][3];
    uint64_t dev;
};
__global__ __launch_bounds__(256) void param_rows_finish_kernel(const RowsFinishArgs a) {
    const int vec = blockIdx.x, n_param = 3 * a.n_vec;
    double s[3] = {0.0, 0.0, 0.0};
    for (int r = threadIdx.x; r < a.n_rows; r += 256) {
        const double *row = a.stage + (int64_t)r * n_param + 3 * vec;
        s[0] += row[0]; s[1] += row[1]; s[2] += row[2];
    }
    __shared__ double red[3][256];
#pragma unroll
    for (int j = 0; j < 3; ++j) red[j][threadIdx.x] = s[j];
    __syncthreads();
    for (int o = 128; o > 0; o >>= 1) {
        if ((int)threadIdx.x < o) {
#pragma unroll
            for (int j = 0; j < 3; ++j) red[j][threadIdx.x] += red[j][threadIdx.x + o];
        }
        __syncthreads();
    }
    if (threadIdx.x != 0) return;
    double g[3] = {red[0][0], red[1][0], red[2][0]};
    const int light = vec - a.first_light;
    if (light >= 0 && light < a.n_lights && a.light_type == PBR_LIGHT_DIRECTIONAL) {
        float x[3];
        for (int j = 0; j < 3; ++j) x[j] = a.dev ? reinterpret_cast<const DevParams *>(a.dev)->raw_lights[light][j] : a.lights[light][j];
        const double nrm = sqrt((double)x[0] * x[0] + (double)x[1] * x[1] + (double)x[2] * x[2]);
        if (nrm > 1e-12) {
            const double u[3] = {x[0] / nrm, x[1] / nrm, x[2] / nrm};
            const double ug = u[0] * g[0] + u[1] * g[1] + u[2] * g[2];
            for (int j = 0; j < 3; ++j) g[j] = (g[j] - u[j] * ug) / nrm;
        } else {
            for (int j = 0; j < 3; ++j) g[j] *= 1e12;
        }
    }
    for (int j = 0; j < 3; ++j) a.out[3 * vec + j] = (float)g[j];
}

size_t param_rows_bytes_of(const pbr_render_desc *d, int n_param) {
    const size_t rows = (size_t)max_tiles(d) * (size_t)n_param * sizeof(float);
    return (rows + 7) & ~(size_t)7;
}
size_t param_stage_bytes_of(int n_param) { return (size_t)kParamStageRows * (size_t)n_param * sizeof(double); }

int param_rows_finish(const pbr_render_desc *d, const float *rows, int n_rows, int n_vec, int first_light, uint64_t dev, float *out, hipStream_t st) {
    RowsFinishArgs f;
    std::memset(&f, 0, sizeof(f));
    const int n_param = 3 * n_vec;
    double *stage = reinterpret_cast<double *>(reinterpret_cast<char *>(const_cast<float *>(rows)) + param_rows_bytes_of(d, n_param));
    hipLaunchKernelGGL(param_grad_stage_kernel, dim3(kParamStageRows), dim3(256), 0, st, rows, stage, n_rows, n_param);
    f.stage = stage; f.out = out;
    f.n_rows = kParamStageRows; f.n_vec = n_vec; f.first_light = first_light; f.n_lights = d->n_lights; f.light_type = d->light_type;
    f.dev = dev;
    for (int i = 0; i < d->n_lights; ++i)
        for (int c = 0; c < 3; ++c) f.lights[i][c] = d->lights[i][c];
    hipLaunchKernelGGL(param_rows_finish_kernel, dim3((unsigned)n_vec), dim3(256), 0, st, f);
    return launch_status();
}

static int launch_backward(const pbr_render_desc *d, const void *grad_out, void *g_albedo, void *g_normal, void *g_roughness,
                           void *g_metallic, void *g_specular, void *g_params, void *workspace, void *stream) {
    const int rc = validate(d);
    if (rc != PBR_OK) return rc;
    if (!grad_out) return PBR_ERR_NULL_MAP;
    if (g_params && !workspace) return PBR_ERR_NULL_MAP;
    if (d->out_dtype != PBR_F32) return PBR_ERR_DTYPE;        // the upstream gradient is fp32; maps (and their gradients) fp32 | fp16
    int vec = pick_vec(d);                                    // grad_out and the g_* only need element alignment (f32x4_e)
    if (vec == 8) vec = 4;
    // Two pixels per lane (one packed pair): (a) with the light / view adjoints (PGRAD) the four-pixel body needs 256 VGPRs +
    // 40 AGPRs = one wave per SIMD, the two-pixel body 155 = three; (b) with fp16 maps and one light the launch is VALU-bound
    // and the two-pixel body (125 VGPRs, 4 waves per SIMD) runs 155.6 us against 162.6 us on a 4096^2 material (steady state,
    // tools/bwd_ab.sh of its round); with fp32 maps the four-pixel body wins (209 vs 218 us).  A rule since ABI 8 (pick_bwd_variant).
    const bool f16_one_light = d->map_dtype == PBR_F16 && d->n_lights == 1;
    if (vec == 4 && (g_params || f16_one_light)) vec = 2;
    // The light / view adjoints are sums over pixels: the overlapping last lane of a ragged row (lane_pos: dup) would
    // count its shared pixels twice, so odd widths take the one-pixel body there.
    if (g_params && (d->width & 1)) vec = 1;
    KArgs k;
    void *const gs[5] = {g_albedo, g_normal, g_roughness, g_metallic, g_specular};
    if (const int rounds = g_params ? 0 : stream_run(d, grad_out, gs)) {
        const StreamLaunch s = stream_launch_shape(d, gs, rounds, k);
        const BArgs b = {grad_out, g_albedo, g_normal, g_roughness, g_metallic, g_specular, nullptr};
        hipLaunchKernelGGL(pick_bwd_stream(d, s.full), dim3((unsigned)s.per_material, (unsigned)d->batch, 1), dim3(64, 1, 1), 0,
                               static_cast<hipStream_t>(stream), k, b, s.tiles, s.n_stores);
        return launch_status();
    }
    // Light / view adjoints: a workgroup adds its waves' sums into LDS with atomics -- with ONE wave per workgroup the
    // order of additions is fixed and the result deterministic run to run (the rows are added in fp64 in a fixed order).
    fill_args(d, vec, k, g_params ? 6 : 0);
    if (k.n_tiles < 0) return PBR_ERR_SHAPE;
    if (g_params && k.n_tiles > max_tiles(d)) return PBR_ERR_SHAPE;   // one workspace row per workgroup: never past what the size query promised
    k.o_cs = (int64_t)d->height * d->width; k.o_bs = 3 * k.o_cs;     // grad_out and the g_* are contiguous, whatever `out` was
    const BArgs b = {grad_out, g_albedo, g_normal, g_roughness, g_metallic, g_specular, static_cast<float *>(workspace)};
    hipStream_t st = static_cast<hipStream_t>(stream);
    const BwdFn fn = g_params ? pick_bwd<true>(d, vec) : pick_bwd<false>(d, vec);
    hipLaunchKernelGGL(fn, dim3((unsigned)k.n_tiles, 1, 1), dim3(1u << k.bt_log2, 1, 1), 0, st, k, b);
    const int e = launch_status();
    if (e != PBR_OK || !g_params) return e;
    return param_grad_finish(d, static_cast<const float *>(workspace), (int)k.n_tiles, k.dev, static_cast<float *>(g_params), st);
}

}  // namespace pbr

extern "C" {

int pbr_cook_torrance_backward(const pbr_render_desc *d, const void *grad_out, void *g_albedo, void *g_normal,
                               void *g_roughness, void *g_metallic, void *g_specular, void *stream) {
    const pbr::TuningScope tuning(d);
    return pbr::launch_backward(d, grad_out, g_albedo, g_normal, g_roughness, g_metallic, g_specular, nullptr, nullptr, stream);
}

size_t pbr_param_grad_workspace_bytes(const pbr_render_desc *d) {
    const pbr::TuningScope tuning(d);
    if (pbr::validate(d) != PBR_OK) return 0;
    const int64_t tiles = pbr::max_tiles(d);
    return tiles < 0 ? 0 : pbr::param_rows_bytes(d) + pbr::param_stage_bytes(d);
}

int pbr_cook_torrance_backward_params(const pbr_render_desc *d, const void *grad_out, void *g_albedo, void *g_normal,
                                      void *g_roughness, void *g_metallic, void *g_specular, void *g_params,
                                      void *workspace, void *stream) {
    const pbr::TuningScope tuning(d);
    if (!g_params) return PBR_ERR_NULL_MAP;
    return pbr::launch_backward(d, grad_out, g_albedo, g_normal, g_roughness, g_metallic, g_specular, g_params, workspace, stream);
}

}  // extern "C"
