// smoothness.hip -- the smoothness prior of a fit: vectorial total variation (Charbonnier) or Tikhonov (L2) over the maps of a material,
// value and gradients of all of them in ONE launch (pbr_smoothness_step) and a small finish launch.  include/pbr_hip.h has the
// definition; tools/smoothness_oracle.py is its yardstick in float64 and float32 numpy.
//
// No reference function is replaced: upstream has no prior.
//
// A launch carries at most PBR_MAX_SMOOTH_TENSORS entries (pbr_smooth_tensor) as kernel arguments.  The grid is 1-D: the workgroups of
// entry 0, then entry 1's, ... (SmoothTable::first); a workgroup finds its entry by comparing its index with at most eight scalars, so the
// entry's fields are scalar loads.  Inside an entry a workgroup is (image, band, strip group): a band is PBR_SMOOTH_BAND_ROWS rows --
// halved, down to PBR_SMOOTH_MIN_BAND_ROWS, while the launch has fewer than PBR_SMOOTH_MIN_BLOCKS workgroups: a wave walks its rows one
// after the other, and a small map divided into few long walks leaves the chip idle (profiles/EXPERIMENTS.md) -- a
// strip group four adjacent strips, one per wave.  A strip is 63 units of a row -- a unit is a quad of pixels on the quad path, one pixel
// on the element path (takes_quads, per entry) -- and lane 0 of the wave holds the unit LEFT of the strip (the halo; with wrap, the row's
// last unit in front of its first).  A lane takes all C channels of its pixels, because q couples them.
//
// The walk (normal_ops.hip's backward): a wave goes down its strip from the row above the band to the band's last row holding rows r and
// r + 1 (r + 2 is on its way).  For row r it forms (q dx_c, q dy_c) ONCE per pixel; the gradient of row r needs that row's pairs, q dy_c of
// row r - 1 (kept from the trip before) and q dx_c of the pixel to the left (the unit's own, or the neighbour lane's last).  The row above
// the band and the halo unit only form pairs: they write nothing and their phi is not added, so no pair is needed from another wave and
// every gradient value is written once.  p(y, x + 1) for a unit's last pixel comes from the neighbour lane; lane 63 and the lane of the
// row's last unit read that one element themselves.  Offsets are 64-bit.
//
// Arithmetic, in the float32 oracle's order -- every product, sum and difference rounded on its own (__fmul_rn / __fadd_rn / __fsub_rn:
// the build's -ffp-contract=on would fuse s + dx dx), square root and divisions IEEE:
//   s = 0; for c = 0 .. C-1: s = (s + dx_c dx_c) + dy_c dy_c
//   L2:           phi = s                   q = (k w) 2
//   Charbonnier:  r = sqrt(s + eps eps)     phi = s / (r + eps)     q = (k w) / r
//   g_c = (left + up) - (q dx_c + q dy_c),  left = (q dx_c)(y, x-1), up = (q dy_c)(y-1, x)
// The value: a lane adds w phi of its pixels in fp64, the lanes of a wave and the four waves are added in a fixed order, the workgroup
// writes ONE fp32 partial; the finish kernel adds an entry's partials in fp64 in a fixed order, multiplies by the entry's k (fp64) and
// writes terms[i] and the sum of the terms.  No atomics: two runs give the same bits.
//
// No cache hints: the gradients are read next by the optimiser, the parameters again by the next loss step.
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstdint>
#include <vector>

#include "../../include/pbr_hip.h"
#include "table_launch.hpp"

namespace pbr {
namespace {

constexpr int kStripUnits = 63;                                        // interior units of a wave's strip (lane 0: the halo)
constexpr int kWaves = PBR_SMOOTH_BLOCK / 64;

// What a launch carries: the caller's entries, which of them take the quad path, where each entry's workgroups start and how they divide.
struct SmoothTable {
    pbr_smooth_tensor t[PBR_MAX_SMOOTH_TENSORS];
    int32_t first[PBR_MAX_SMOOTH_TENSORS + 1];
    int32_t strip_groups[PBR_MAX_SMOOTH_TENSORS], bands[PBR_MAX_SMOOTH_TENSORS];
    uint8_t quads[PBR_MAX_SMOOTH_TENSORS];
    int32_t n, rows;                                                   // rows of a band, the same for every entry of the launch
};

// One row of a strip as a lane holds it: the C x V values of its unit, the value right of the unit (read only by the lanes that cannot
// take it from the neighbour lane) and the V weights.  A row or a unit outside the map is zeros with weight 0.
template <int C, int V> struct SRow {
    float v[C][V], rt[C], w[V];
};

template <typename T, int C, int V>
__device__ __forceinline__ void load_row(SRow<C, V> &o, const T *p, int64_t ps, const float *wp, int r, int H, int W, bool wrap, int64_t x0,
                                         bool live, bool edge, bool rt_ok) {
#pragma unroll
    for (int c = 0; c < C; ++c) {
#pragma unroll
        for (int j = 0; j < V; ++j) o.v[c][j] = 0.0f;
        o.rt[c] = 0.0f;
    }
#pragma unroll
    for (int j = 0; j < V; ++j) o.w[j] = 0.0f;
    if (!live || !(wrap || (r >= 0 && r < H))) return;
    const int row = r < 0 ? r + H : (r >= H ? r - H : r);
    const int64_t at = (int64_t)row * W + x0;
#pragma unroll
    for (int c = 0; c < C; ++c) Span<T, V>::ld(p, c * ps + at, o.v[c]);
    if (wp) {
        Span<float, V>::ld(wp, at, o.w);
    } else {
#pragma unroll
        for (int j = 0; j < V; ++j) o.w[j] = 1.0f;
    }
    if (edge && rt_ok) {
        const int64_t right = (int64_t)row * W + (x0 + V < W ? x0 + V : 0);
#pragma unroll
        for (int c = 0; c < C; ++c) o.rt[c] = Elem<T>::ld(p, c * ps + right);
    }
}

// One wave, one strip of one band of one image of entry `e`; returns the lane's sum of w phi over the pixels it owns.
template <typename T, int C, int V>
__device__ __forceinline__ double smooth_strip(const pbr_smooth_tensor &e, int blk, int strip_groups, int bands, int rows) {
    const int lane = threadIdx.x & 63;
    const int sg = blk % strip_groups;
    blk /= strip_groups;
    const int band = blk % bands, b = blk / bands;
    const int H = e.height, W = e.width, units = W / V;               // V = 4: the launcher checked that W is whole quads
    const bool wrap = e.wrap != 0;
    const int strip = sg * kWaves + (int)(threadIdx.x >> 6);
    if ((int64_t)strip * kStripUnits >= units) return 0.0;             // the whole wave is beyond the row
    int u = strip * kStripUnits + lane - 1;
    bool live = u >= 0 && u < units;
    if (u < 0 && wrap) { u = units - 1; live = true; }                 // the halo of the first strip: the row's last unit
    const bool owns = lane >= 1 && live;
    const int y0 = band * rows, y1 = min(H, y0 + rows);
    const int64_t x0 = (int64_t)u * V;
    const bool edge = lane == 63 || u == units - 1;                    // no neighbour lane holds p(y, x0 + V)
    const bool rt_ok = wrap || x0 + V < W;                             // ... and whether the definition has it at all
    const T *p = static_cast<const T *>(e.param) + (int64_t)b * e.param_batch_stride;
    T *g = e.grad ? static_cast<T *>(e.grad) + (int64_t)b * e.grad_batch_stride : nullptr;
    const float *wp = e.weights ? e.weights + (int64_t)b * e.weights_batch_stride : nullptr;
    const int64_t ps = e.param_plane_stride, gs = e.grad_plane_stride;
    const float k = (float)e.k, eps = e.eps, eps2 = __fmul_rn(eps, eps);
    const bool l2 = e.kind == PBR_SMOOTH_L2;

    SRow<C, V> cur, nxt, pre;                                          // rows r, r + 1, r + 2
    load_row<T, C, V>(cur, p, ps, wp, y0 - 1, H, W, wrap, x0, live, edge, rt_ok);
    load_row<T, C, V>(nxt, p, ps, wp, y0, H, W, wrap, x0, live, edge, rt_ok);
    float up[C][V];                                                    // q dy_c of row r - 1
#pragma unroll
    for (int c = 0; c < C; ++c) {
#pragma unroll
        for (int j = 0; j < V; ++j) up[c][j] = 0.0f;
    }
    double acc = 0.0;
    for (int r = y0 - 1; r < y1; ++r) {
        load_row<T, C, V>(pre, p, ps, wp, r + 2, H, W, wrap, x0, live && r + 2 <= y1, edge, rt_ok);       // rows y0 - 1 ... y1 are all the band needs
        const bool row_live = live && (wrap || r >= 0);
        const bool dy_ok = wrap || r + 1 < H;
        float right[C];
#pragma unroll
        for (int c = 0; c < C; ++c) {
            const float from_lane = __shfl_down(cur.v[c][0], 1, 64);
            right[c] = edge ? cur.rt[c] : from_lane;
        }
        float qdx[C][V], qdy[C][V];
#pragma unroll
        for (int j = 0; j < V; ++j) {
            float dx[C], dy[C], s = 0.0f;
#pragma unroll
            for (int c = 0; c < C; ++c) {
                const float beside = j == V - 1 ? right[c] : cur.v[c][j == V - 1 ? j : j + 1];
                dx[c] = (j == V - 1 && !rt_ok) ? 0.0f : __fsub_rn(beside, cur.v[c][j]);
                dy[c] = dy_ok ? __fsub_rn(nxt.v[c][j], cur.v[c][j]) : 0.0f;
                s = __fadd_rn(__fadd_rn(s, __fmul_rn(dx[c], dx[c])), __fmul_rn(dy[c], dy[c]));
            }
            const float kw = __fmul_rn(k, cur.w[j]);
            float q, phi;
            if (l2) {
                q = __fmul_rn(kw, 2.0f);
                phi = s;
            } else {
                const float root = __builtin_sqrtf(__fadd_rn(s, eps2));          // IEEE (__fsqrt_rn is the native square root in this build)
                q = __fdiv_rn(kw, root);
                phi = __fdiv_rn(s, __fadd_rn(root, eps));
            }
            if (owns && r >= y0) acc += (double)__fmul_rn(cur.w[j], phi);
#pragma unroll
            for (int c = 0; c < C; ++c) {
                qdx[c][j] = row_live ? __fmul_rn(q, dx[c]) : 0.0f;
                qdy[c][j] = row_live ? __fmul_rn(q, dy[c]) : 0.0f;
            }
        }
        if (r >= y0) {                                                 // emit row r
#pragma unroll
            for (int c = 0; c < C; ++c) {
                const float from_left = __shfl_up(qdx[c][V - 1], 1, 64);
                float out[V];
#pragma unroll
                for (int j = 0; j < V; ++j) {
                    const float left = j == 0 ? from_left : qdx[c][j == 0 ? j : j - 1];
                    out[j] = __fsub_rn(__fadd_rn(left, up[c][j]), __fadd_rn(qdx[c][j], qdy[c][j]));
                }
                if (g && owns) Span<T, V>::st(g, c * gs + (int64_t)r * W + x0, out);
            }
        }
#pragma unroll
        for (int c = 0; c < C; ++c) {
#pragma unroll
            for (int j = 0; j < V; ++j) up[c][j] = qdy[c][j];
        }
        cur = nxt;
        nxt = pre;
    }
    return acc;
}

template <typename T, int V>
__device__ __forceinline__ double smooth_channels(const pbr_smooth_tensor &e, int blk, int strip_groups, int bands, int rows) {
    switch (e.channels) {
    case 1: return smooth_strip<T, 1, V>(e, blk, strip_groups, bands, rows);
    case 2: return smooth_strip<T, 2, V>(e, blk, strip_groups, bands, rows);
    case 3: return smooth_strip<T, 3, V>(e, blk, strip_groups, bands, rows);
    default: return smooth_strip<T, 4, V>(e, blk, strip_groups, bands, rows);
    }
}

__global__ __launch_bounds__(PBR_SMOOTH_BLOCK) void smoothness_step_kernel(SmoothTable tab, float *__restrict__ partials) {
    __shared__ double red[kWaves];
    int i = 0;
    while (i + 1 < tab.n && (int32_t)blockIdx.x >= tab.first[i + 1]) ++i;
    const pbr_smooth_tensor &e = tab.t[i];
    const int blk = (int)blockIdx.x - tab.first[i], sg = tab.strip_groups[i], bands = tab.bands[i];
    const bool quads = tab.quads[i] != 0;
    double acc;
    if (e.dtype == PBR_F32) {
        acc = quads ? smooth_channels<float, 4>(e, blk, sg, bands, tab.rows) : smooth_channels<float, 1>(e, blk, sg, bands, tab.rows);
    } else {
        acc = quads ? smooth_channels<__half, 4>(e, blk, sg, bands, tab.rows) : smooth_channels<__half, 1>(e, blk, sg, bands, tab.rows);
    }
    for (int o = 32; o > 0; o >>= 1) acc += __shfl_down(acc, o, 64);
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = acc;
    __syncthreads();
    if (threadIdx.x == 0) {
        double total = red[0];
        for (int w = 1; w < kWaves; ++w) total += red[w];
        partials[blockIdx.x] = (float)total;
    }
}

struct FinishTable {
    double k[PBR_MAX_SMOOTH_TENSORS];
    int32_t first[PBR_MAX_SMOOTH_TENSORS + 1];
    int32_t n;
};

// One workgroup: entry after entry, the entry's partials in fp64 (lane t takes partials t, t + 256, ...; then a tree), times k.
__global__ __launch_bounds__(256) void smoothness_finish_kernel(FinishTable f, const float *__restrict__ partials, float *__restrict__ terms,
                                                                float *__restrict__ loss) {
    __shared__ double red[256];
    double sum = 0.0;
    for (int i = 0; i < f.n; ++i) {
        double s = 0.0;
        for (int j = f.first[i] + (int)threadIdx.x; j < f.first[i + 1]; j += 256) s += partials[j];
        red[threadIdx.x] = s;
        __syncthreads();
        for (int o = 128; o > 0; o >>= 1) {
            if ((int)threadIdx.x < o) red[threadIdx.x] += red[threadIdx.x + o];
            __syncthreads();
        }
        const double term = red[0] * f.k[i];
        __syncthreads();
        if (threadIdx.x == 0 && terms) terms[i] = (float)term;
        sum += term;
    }
    if (threadIdx.x == 0) *loss = (float)sum;
}

// Whole quads everywhere: 16-byte accesses of fp32 planes and weights, 8-byte ones of fp16 planes.
inline bool takes_quads(const pbr_smooth_tensor &e) {
    return whole_quads({e.width, e.param_batch_stride, e.param_plane_stride, e.grad_batch_stride, e.grad_plane_stride, e.weights_batch_stride}) &&
           all_aligned(quad_bytes(e.dtype), {e.param, e.grad}) && all_aligned(16, {e.weights});
}

// Workgroups of one entry: images x bands x strip groups.
inline int64_t entry_blocks(const pbr_smooth_tensor &e, bool quads, int32_t rows, int32_t &strip_groups, int32_t &bands) {
    const int64_t units = e.width / (quads ? 4 : 1);
    const int64_t strips = (units + kStripUnits - 1) / kStripUnits;
    strip_groups = (int32_t)((strips + kWaves - 1) / kWaves);
    bands = (e.height + rows - 1) / rows;
    return (int64_t)e.batch * bands * strip_groups;
}

// A gradient, which is written, may overlap nothing else the launch touches; parameters and weights, only read, may overlap each other
// (table_launch.hpp: written_overlaps).  Weights with batch stride 0 are one plane, counted once.
bool launch_overlaps(const pbr_smooth_tensor *t, int32_t n) {
    std::vector<Interval> iv;
    bool any_grad = false;
    for (int32_t i = 0; i < n; ++i) {
        const pbr_smooth_tensor &e = t[i];
        const size_t esz = elem_bytes(e.dtype);
        const int64_t pixels = (int64_t)e.height * e.width;
        add_planes(iv, e.param, e.batch, e.channels, pixels, e.param_batch_stride, e.param_plane_stride, esz, false);
        if (e.weights) add_planes(iv, e.weights, e.weights_batch_stride ? e.batch : 1, 1, pixels, e.weights_batch_stride, 0, sizeof(float), false);
        if (e.grad) {
            add_planes(iv, e.grad, e.batch, e.channels, pixels, e.grad_batch_stride, e.grad_plane_stride, esz, true);
            any_grad = true;
        }
    }
    return any_grad && written_overlaps(iv);
}

int check_entry(const pbr_smooth_tensor &e) {
    if (!e.param) return PBR_ERR_NULL_MAP;
    if (e.dtype != PBR_F32 && e.dtype != PBR_F16) return PBR_ERR_DTYPE;
    if (e.kind != PBR_SMOOTH_L2 && e.kind != PBR_SMOOTH_CHARBONNIER) return PBR_ERR_UNSUPPORTED;
    if (e.channels < 1 || e.channels > 4) return PBR_ERR_CHANNELS;
    if (e.batch < 1 || e.height < 1 || e.width < 1) return PBR_ERR_SHAPE;
    if (e.height > (1 << 30) || e.width > (1 << 30) || (int64_t)e.height * e.width > ((int64_t)1 << 40)) return PBR_ERR_SHAPE;
    if (e.kind == PBR_SMOOTH_CHARBONNIER && !(e.eps > 0.0f && std::isfinite(e.eps))) return PBR_ERR_SHAPE;
    if (!std::isfinite(e.k)) return PBR_ERR_SHAPE;
    if (e.param_batch_stride < 0 || e.param_plane_stride < 0 || e.grad_batch_stride < 0 || e.grad_plane_stride < 0 || e.weights_batch_stride < 0)
        return PBR_ERR_SHAPE;
    if (!all_aligned(elem_bytes(e.dtype), {e.param, e.grad}) || !all_aligned(4, {e.weights})) return PBR_ERR_SHAPE;
    return PBR_OK;
}

// The table a checked launch runs from; returns its workgroups (0: more than the grid holds).  The bands are as long as they may be
// unless that leaves the launch under PBR_SMOOTH_MIN_BLOCKS workgroups: then half as long, and so on.
int64_t fill_table(const pbr_smooth_tensor *tensors, int32_t n, SmoothTable &tab) {
    tab.n = n;
    pad_table(tab.t, tensors, n);
    for (int32_t i = 0; i < PBR_MAX_SMOOTH_TENSORS; ++i) tab.quads[i] = takes_quads(tab.t[i]) ? 1 : 0;
    for (int32_t rows = PBR_SMOOTH_BAND_ROWS;; rows /= 2) {
        int64_t blocks = 0;
        tab.rows = rows;
        for (int32_t i = 0; i < PBR_MAX_SMOOTH_TENSORS; ++i) {
            tab.first[i] = (int32_t)blocks;
            const int64_t mine = entry_blocks(tab.t[i], tab.quads[i] != 0, rows, tab.strip_groups[i], tab.bands[i]);
            if (i < n) blocks += mine;
            if (blocks > INT32_MAX) return 0;
        }
        tab.first[PBR_MAX_SMOOTH_TENSORS] = (int32_t)blocks;
        if (blocks >= PBR_SMOOTH_MIN_BLOCKS || rows <= PBR_SMOOTH_MIN_BAND_ROWS) return blocks;
    }
}

}  // namespace
}  // namespace pbr

extern "C" {

size_t pbr_smooth_tensor_size(void) { return sizeof(pbr_smooth_tensor); }

int pbr_smoothness_check(const pbr_smooth_tensor *tensors, int32_t n_tensors) {
    using namespace pbr;
    if (!tensors) return PBR_ERR_NULL_MAP;
    if (n_tensors < 1 || n_tensors > PBR_MAX_SMOOTH_TENSORS) return PBR_ERR_SHAPE;
    for (int32_t i = 0; i < n_tensors; ++i) {
        const int rc = check_entry(tensors[i]);
        if (rc != PBR_OK) return rc;
    }
    SmoothTable tab;
    if (fill_table(tensors, n_tensors, tab) == 0) return PBR_ERR_SHAPE;
    return launch_overlaps(tensors, n_tensors) ? PBR_ERR_SHAPE : PBR_OK;
}

size_t pbr_smoothness_workspace_bytes(const pbr_smooth_tensor *tensors, int32_t n_tensors) {
    using namespace pbr;
    if (pbr_smoothness_check(tensors, n_tensors) != PBR_OK) return 0;
    SmoothTable tab;
    return (size_t)fill_table(tensors, n_tensors, tab) * sizeof(float);
}

int pbr_smoothness_step(const pbr_smooth_tensor *tensors, int32_t n_tensors, void *loss, void *terms, void *workspace, size_t workspace_bytes,
                        void *stream) {
    using namespace pbr;
    if (!tensors || !loss || !workspace) return PBR_ERR_NULL_MAP;
    const int rc = pbr_smoothness_check(tensors, n_tensors);
    if (rc != PBR_OK) return rc;
    SmoothTable tab;
    const int64_t blocks = fill_table(tensors, n_tensors, tab);
    if (workspace_bytes < (size_t)blocks * sizeof(float) || !is_aligned(workspace, 4) || !all_aligned(4, {loss, terms})) return PBR_ERR_SHAPE;
    FinishTable fin;
    fin.n = n_tensors;
    for (int32_t i = 0; i <= PBR_MAX_SMOOTH_TENSORS; ++i) fin.first[i] = tab.first[i];
    for (int32_t i = 0; i < PBR_MAX_SMOOTH_TENSORS; ++i) fin.k[i] = tab.t[i].k;
    hipStream_t st = static_cast<hipStream_t>(stream);
    float *partials = static_cast<float *>(workspace);
    hipLaunchKernelGGL(smoothness_step_kernel, dim3((uint32_t)blocks), dim3(PBR_SMOOTH_BLOCK), 0, st, tab, partials);
    hipLaunchKernelGGL(smoothness_finish_kernel, dim3(1), dim3(256), 0, st, fin, partials, static_cast<float *>(terms), static_cast<float *>(loss));
    return launch_status();
}

}  // extern "C"
