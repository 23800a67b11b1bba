// adam.hip -- the optimiser step of a fit: projected Adam for every map of a material in ONE launch (pbr_adam_step), and the one-lane
// kernel that advances the device step counters of a capturable optimiser (pbr_adam_advance).  include/pbr_hip.h has the definition;
// tools/adam_oracle.py is its yardstick in float64 and float32 numpy.
//
// No reference function is replaced: upstream has no optimiser.  In exact arithmetic the update is torch.optim.Adam's (weight_decay 0, no
// amsgrad, no maximize); the projection behind it (box, unit normal with a floor on z) and the rule that an element whose update is exactly
// zero keeps its bits are this library's.
//
// A launch carries at most PBR_MAX_ADAM_TENSORS entries (pbr_adam_tensor) and as many coefficient rows as kernel arguments: the entry is
// blockIdx.y, the same for every lane of a workgroup, so its fields are scalar loads from the argument segment.  The coefficient row comes
// from the arguments (host values) or, when the launch was given a device table, from that table when the kernel runs (a uniform load).
// Grid: (min(quads of the largest plane / 256, PBR_ADAM_MAX_BLOCKS), entries).  A workgroup walks the planes of its entry one after the
// other (a uniform loop: no per-lane division), its lanes the quads of a plane with the grid's stride; the unit projection walks images
// instead and takes the three planes of a pixel in one lane.  State (m, v, master) is dense, so its offset is the plane's number times
// `pixels`.  Offsets are 64-bit.
//
// Arithmetic: every product, sum and difference is rounded on its own, in the oracle's order (__fmul_rn / __fadd_rn / __fsub_rn: the
// build's -ffp-contract=on would fuse m + (g - m) k) -- the norm of the unit projection alone is the fused chain the oracle names -- the
// square roots and divisions are IEEE.  The kernel therefore computes what the
// oracle computes in float32, and the launch is bound by memory: 28 bytes per fp32 element, 30 per fp16 element with its master.
//
// Cache policy (PBR_ADAM_POLICY, a build-time choice; profiles/EXPERIMENTS.md has the A/B): bit 0 the parameter's load and store, bit 1
// the gradient's load, bit 2 the loads of m, v and master, bit 3 their stores carry the non-temporal hint.  The parameter is read again by
// the next loss step; m, v and master only by the next update.
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstdint>
#include <vector>

#include "../../include/pbr_hip.h"
#include "table_launch.hpp"

#ifndef PBR_ADAM_POLICY
#define PBR_ADAM_POLICY 14
#endif

namespace pbr {
namespace {

constexpr bool kNtParam = (PBR_ADAM_POLICY & 1) != 0, kNtGrad = (PBR_ADAM_POLICY & 2) != 0;
constexpr bool kNtStateLoad = (PBR_ADAM_POLICY & 4) != 0, kNtStateStore = (PBR_ADAM_POLICY & 8) != 0;

// What a launch carries: the caller's entries, which of them take the quad path (the launcher's alignment test), the coefficient rows.
struct AdamTable {
    pbr_adam_tensor t[PBR_MAX_ADAM_TENSORS];
    pbr_adam_coeffs k[PBR_MAX_ADAM_TENSORS];
    const pbr_adam_coeffs *k_device;               // not NULL: the rows are read from here when the kernel runs
    uint8_t quads[PBR_MAX_ADAM_TENSORS];
};

// One element: m, v updated in place, the step delta returned.
__device__ __forceinline__ float adam_delta(const pbr_adam_coeffs &k, float g, float &m, float &v) {
    m = __fadd_rn(m, __fmul_rn(__fsub_rn(g, m), k.one_minus_beta1));
    v = __fadd_rn(__fmul_rn(k.beta2, v), __fmul_rn(__fmul_rn(k.one_minus_beta2, g), g));
    return __fdiv_rn(__fmul_rn(k.a, m), __fadd_rn(__fmul_rn(__builtin_sqrtf(v), k.c), k.eps));
}

// torch.clamp's comparisons: a NaN stays a NaN.
__device__ __forceinline__ float clamp_lo(float x, float lo) { return x < lo ? lo : x; }
__device__ __forceinline__ float clamp_hi(float x, float hi) { return x > hi ? hi : x; }

// V elements of one plane.  `P` is the parameter's storage type; `w` (the master, or the fp32 parameter itself) is what the update runs on.
template <typename P, int V> struct Lane {
    float p[V], g[V], m[V], v[V], w[V];
    static constexpr bool kMaster = !std::is_same<P, float>::value;

    __device__ __forceinline__ void load(const pbr_adam_tensor &e, int64_t po, int64_t go, int64_t so) {
        Span<P, V>::template load<kNtParam>(e.param, po, p);
        Span<P, V>::template load<kNtGrad>(e.grad, go, g);
        Span<float, V>::template load<kNtStateLoad>(e.exp_avg, so, m);
        Span<float, V>::template load<kNtStateLoad>(e.exp_avg_sq, so, v);
        if constexpr (kMaster) {
            Span<float, V>::template load<kNtStateLoad>(e.master, so, w);
        } else {
#pragma unroll
            for (int j = 0; j < V; ++j) w[j] = p[j];
        }
    }
    // `keep[j]`: element j keeps the bits it had (p was loaded exactly, so storing it back writes the same bits)
    __device__ __forceinline__ void store(const pbr_adam_tensor &e, int64_t po, int64_t so, const float (&out)[V], const bool (&keep)[V]) {
        float q[V];
        if constexpr (kMaster) {
            float wn[V];
#pragma unroll
            for (int j = 0; j < V; ++j) {
                wn[j] = keep[j] ? w[j] : out[j];
                q[j] = keep[j] ? p[j] : out[j];                 // Span's store rounds to nearest even
            }
            Span<float, V>::template store<kNtStateStore>(e.master, so, wn);
        } else {
#pragma unroll
            for (int j = 0; j < V; ++j) q[j] = keep[j] ? p[j] : out[j];
        }
        Span<P, V>::template store<kNtParam>(e.param, po, q);
        Span<float, V>::template store<kNtStateStore>(e.exp_avg, so, m);
        Span<float, V>::template store<kNtStateStore>(e.exp_avg_sq, so, v);
    }
};

template <typename P, int V> __device__ __forceinline__ void adam_entry(const pbr_adam_tensor &e, const pbr_adam_coeffs &k) {
    const int64_t units = e.pixels / V;                                 // V = 4: the launcher checked that pixels is whole quads
    const int64_t stride = (int64_t)gridDim.x * PBR_ADAM_BLOCK;
    const int64_t first = (int64_t)blockIdx.x * PBR_ADAM_BLOCK + threadIdx.x;
    if (first >= units) return;
    if (e.project == PBR_ADAM_UNIT) {
        for (int32_t b = 0; b < e.batch; ++b) {
            const int64_t p0 = (int64_t)b * e.param_batch_stride, g0 = (int64_t)b * e.grad_batch_stride, s0 = (int64_t)b * 3 * e.pixels;
            for (int64_t u = first; u < units; u += stride) {
                Lane<P, V> x, y, z;
                x.load(e, p0 + u * V, g0 + u * V, s0 + u * V);
                y.load(e, p0 + e.param_plane_stride + u * V, g0 + e.grad_plane_stride + u * V, s0 + e.pixels + u * V);
                z.load(e, p0 + 2 * e.param_plane_stride + u * V, g0 + 2 * e.grad_plane_stride + u * V, s0 + 2 * e.pixels + u * V);
                float ox[V], oy[V], oz[V];
                bool keep[V];
#pragma unroll
                for (int j = 0; j < V; ++j) {
                    const float dx = adam_delta(k, x.g[j], x.m[j], x.v[j]);
                    const float dy = adam_delta(k, y.g[j], y.m[j], y.v[j]);
                    const float dz = adam_delta(k, z.g[j], z.m[j], z.v[j]);
                    keep[j] = dx == 0.0f && dy == 0.0f && dz == 0.0f;
                    const float nx = __fsub_rn(x.w[j], dx), ny = __fsub_rn(y.w[j], dy), nz = clamp_lo(__fsub_rn(z.w[j], dz), e.min_z);
                    const float len = __builtin_sqrtf(__fmaf_rn(nz, nz, __fmaf_rn(ny, ny, __fmul_rn(nx, nx))));     // the oracle's |p|: F.normalize's on the host
                    const float d = clamp_lo(len, 1e-12f);
                    ox[j] = __fdiv_rn(nx, d); oy[j] = __fdiv_rn(ny, d); oz[j] = __fdiv_rn(nz, d);
                }
                x.store(e, p0 + u * V, s0 + u * V, ox, keep);
                y.store(e, p0 + e.param_plane_stride + u * V, s0 + e.pixels + u * V, oy, keep);
                z.store(e, p0 + 2 * e.param_plane_stride + u * V, s0 + 2 * e.pixels + u * V, oz, keep);
            }
        }
        return;
    }
    const bool box = e.project == PBR_ADAM_BOX;
    int32_t b = 0, c = 0;
    for (int64_t q = 0, planes = (int64_t)e.batch * e.channels; q < planes; ++q) {
        const int64_t p0 = (int64_t)b * e.param_batch_stride + (int64_t)c * e.param_plane_stride;
        const int64_t g0 = (int64_t)b * e.grad_batch_stride + (int64_t)c * e.grad_plane_stride, s0 = q * e.pixels;
        for (int64_t u = first; u < units; u += stride) {
            Lane<P, V> x;
            x.load(e, p0 + u * V, g0 + u * V, s0 + u * V);
            float o[V];
            bool keep[V];
#pragma unroll
            for (int j = 0; j < V; ++j) {
                const float d = adam_delta(k, x.g[j], x.m[j], x.v[j]);
                keep[j] = d == 0.0f;
                const float n = __fsub_rn(x.w[j], d);
                o[j] = box ? clamp_hi(clamp_lo(n, e.lo), e.hi) : n;
            }
            x.store(e, p0 + u * V, s0 + u * V, o, keep);
        }
        if (++c == e.channels) { c = 0; ++b; }
    }
}

__global__ __launch_bounds__(PBR_ADAM_BLOCK) void adam_step_kernel(AdamTable tab) {
    const pbr_adam_tensor &e = tab.t[blockIdx.y];
    const pbr_adam_coeffs k = tab.k_device ? tab.k_device[e.group] : tab.k[e.group];
    const bool quads = tab.quads[blockIdx.y] != 0;
    if (e.dtype == PBR_F32) {
        if (quads) adam_entry<float, 4>(e, k); else adam_entry<float, 1>(e, k);
    } else {
        if (quads) adam_entry<__half, 4>(e, k); else adam_entry<__half, 1>(e, k);
    }
}

struct GroupTable { pbr_adam_group g[PBR_MAX_ADAM_TENSORS]; };

// One lane: the counters and the coefficient rows of a capturable optimiser.
__global__ void adam_advance_kernel(GroupTable tab, int32_t n, pbr_adam_coeffs *out) {
    if (blockIdx.x != 0 || threadIdx.x != 0) return;
    for (int32_t i = 0; i < n; ++i) {
        const pbr_adam_group &g = tab.g[i];
        float *step = static_cast<float *>(g.step);
        const float t = *step + 1.0f;
        *step = t;
        const double lr = g.lr_device ? (double)*static_cast<const float *>(g.lr_device) : g.lr;
        pbr_adam_coeffs k;
        k.a = (float)(lr / (1.0 - pow(g.beta1, (double)t)));
        k.c = (float)(1.0 / sqrt(1.0 - pow(g.beta2, (double)t)));
        k.one_minus_beta1 = (float)(1.0 - g.beta1);
        k.beta2 = (float)g.beta2;
        k.one_minus_beta2 = (float)(1.0 - g.beta2);
        k.eps = (float)g.eps;
        out[i] = k;
    }
}

// Nothing that is written -- the parameter, m, v, the master -- may overlap anything else the launch touches (p and g of one entry
// included); the gradients, only read, may overlap themselves (table_launch.hpp: written_overlaps).
bool launch_overlaps(const pbr_adam_tensor *t, int32_t n) {
    std::vector<Interval> iv;
    for (int32_t i = 0; i < n; ++i) {
        const pbr_adam_tensor &e = t[i];
        const size_t esz = elem_bytes(e.dtype);
        const int64_t dense = (int64_t)e.batch * e.channels * e.pixels;   // state: [batch][channels][pixels], back to back
        add_planes(iv, e.param, e.batch, e.channels, e.pixels, e.param_batch_stride, e.param_plane_stride, esz, true);
        add_planes(iv, e.grad, e.batch, e.channels, e.pixels, e.grad_batch_stride, e.grad_plane_stride, esz, false);
        for (const void *state : {e.exp_avg, e.exp_avg_sq, e.master})
            if (state) add_planes(iv, state, 1, 1, dense, 0, 0, sizeof(float), true);
    }
    return written_overlaps(iv);
}

int check_entry(const pbr_adam_tensor &e, int32_t n_groups) {
    if (!e.param || !e.grad || !e.exp_avg || !e.exp_avg_sq) return PBR_ERR_NULL_MAP;
    if (e.dtype != PBR_F32 && e.dtype != PBR_F16) return PBR_ERR_DTYPE;
    if (e.dtype == PBR_F16 && !e.master) return PBR_ERR_NULL_MAP;
    if (e.dtype == PBR_F32 && e.master) return PBR_ERR_UNSUPPORTED;
    if (e.project != PBR_ADAM_NONE && e.project != PBR_ADAM_BOX && e.project != PBR_ADAM_UNIT) return PBR_ERR_UNSUPPORTED;
    if (e.batch < 1 || e.channels < 1 || e.pixels < 1) return PBR_ERR_SHAPE;
    if (e.project == PBR_ADAM_UNIT && e.channels != 3) return PBR_ERR_CHANNELS;
    if (e.param_batch_stride < 0 || e.param_plane_stride < 0 || e.grad_batch_stride < 0 || e.grad_plane_stride < 0) return PBR_ERR_SHAPE;
    // planes and images of the parameter, which is written, may not lie on top of each other
    if (e.channels > 1 && e.param_plane_stride < e.pixels) return PBR_ERR_SHAPE;
    if (e.batch > 1 && e.param_batch_stride < (int64_t)(e.channels - 1) * e.param_plane_stride + e.pixels) return PBR_ERR_SHAPE;
    if (e.project == PBR_ADAM_BOX && e.lo > e.hi) return PBR_ERR_SHAPE;
    if (e.group < 0 || e.group >= n_groups) return PBR_ERR_SHAPE;
    if (!all_aligned(elem_bytes(e.dtype), {e.param, e.grad}) || !all_aligned(4, {e.exp_avg, e.exp_avg_sq, e.master})) return PBR_ERR_SHAPE;
    return PBR_OK;
}

// Whole quads everywhere: 16-byte accesses of the fp32 planes, 8-byte ones of the fp16 planes.
inline bool takes_quads(const pbr_adam_tensor &e) {
    return whole_quads({e.pixels, e.param_batch_stride, e.param_plane_stride, e.grad_batch_stride, e.grad_plane_stride}) &&
           all_aligned(quad_bytes(e.dtype), {e.param, e.grad}) && all_aligned(16, {e.exp_avg, e.exp_avg_sq, e.master});
}

}  // namespace
}  // namespace pbr

extern "C" {

size_t pbr_adam_tensor_size(void) { return sizeof(pbr_adam_tensor); }

int pbr_adam_check(const pbr_adam_tensor *tensors, int32_t n_tensors, int32_t n_groups) {
    using namespace pbr;
    if (!tensors) return PBR_ERR_NULL_MAP;
    if (n_tensors < 1 || n_tensors > PBR_MAX_ADAM_TENSORS || n_groups < 1 || n_groups > PBR_MAX_ADAM_TENSORS) return PBR_ERR_SHAPE;
    for (int32_t i = 0; i < n_tensors; ++i) {
        const int rc = check_entry(tensors[i], n_groups);
        if (rc != PBR_OK) return rc;
    }
    return launch_overlaps(tensors, n_tensors) ? PBR_ERR_SHAPE : PBR_OK;
}

int pbr_adam_step(const pbr_adam_tensor *tensors, int32_t n_tensors, const pbr_adam_coeffs *coeffs_host, const void *coeffs_device,
                  int32_t n_groups, void *stream) {
    using namespace pbr;
    if (!tensors || (coeffs_host == nullptr) == (coeffs_device == nullptr)) return PBR_ERR_NULL_MAP;
    const int rc = pbr_adam_check(tensors, n_tensors, n_groups);
    if (rc != PBR_OK) return rc;
    AdamTable tab{};                                                    // (the rows stay zeros when the kernel reads them from the device)
    int64_t blocks = 1;
    pad_table(tab.t, tensors, n_tensors);
    for (int32_t i = 0; i < PBR_MAX_ADAM_TENSORS; ++i) {
        tab.quads[i] = takes_quads(tab.t[i]) ? 1 : 0;
        const int64_t units = tab.t[i].pixels / (tab.quads[i] ? 4 : 1);
        const int64_t need = (units + PBR_ADAM_BLOCK - 1) / PBR_ADAM_BLOCK;
        if (i < n_tensors && need > blocks) blocks = need;
    }
    if (blocks > PBR_ADAM_MAX_BLOCKS) blocks = PBR_ADAM_MAX_BLOCKS;
    if (coeffs_host) pad_table(tab.k, coeffs_host, n_groups);
    tab.k_device = static_cast<const pbr_adam_coeffs *>(coeffs_device);
    hipLaunchKernelGGL(adam_step_kernel, dim3((uint32_t)blocks, (uint32_t)n_tensors), dim3(PBR_ADAM_BLOCK), 0, static_cast<hipStream_t>(stream), tab);
    return launch_status();
}

int pbr_adam_advance(const pbr_adam_group *groups, int32_t n_groups, void *coeffs_device, void *stream) {
    using namespace pbr;
    if (!groups || !coeffs_device) return PBR_ERR_NULL_MAP;
    if (n_groups < 1 || n_groups > PBR_MAX_ADAM_TENSORS) return PBR_ERR_SHAPE;
    GroupTable tab;
    pad_table(tab.g, groups, n_groups);
    for (int32_t i = 0; i < n_groups; ++i)
        if (!tab.g[i].step) return PBR_ERR_NULL_MAP;
    hipLaunchKernelGGL(adam_advance_kernel, dim3(1), dim3(64), 0, static_cast<hipStream_t>(stream), tab, n_groups, static_cast<pbr_adam_coeffs *>(coeffs_device));
    return launch_status();
}

}  // extern "C"
