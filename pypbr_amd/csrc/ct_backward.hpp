// ct_backward.hpp -- gradient of the fused Cook-Torrance evaluation w.r.t. the material maps
// (the documented ML use of the reference is a rendering loss,
// /root/reference/docs/source/tutorials/06_advanced.rst:73-107, where autograd differentiates
// pypbr/models/cooktorrance.py:92-182 back to albedo / normal / roughness / metallic|specular).
//
// One streaming kernel: per pixel it re-evaluates the forward terms from the maps (cheaper than storing ~20 intermediates per pixel:
// 32 B of maps + 12 B of upstream gradient in, 32 B of gradients out) and applies the chain rule by hand: the mathematics and its
// sub-gradient conventions are ct_chain_rule.hpp's.  Here: the kernel arguments, the loss policies, the body every untiled kernel shares
// (backward_body_to), the frame of the loss steps and the one-tile kernel.  The streamed form is ct_backward_stream.hpp; the two
// reduction kernels behind the light / view sums are ct_backward.hip's.  With fp16 maps the kernel moves half the bytes and takes the
// same time, i.e. it is bound by instruction issue -- which is what the chain rule's packed form (two pixels per instruction) halves.
#pragma once
#include "ct_chain_rule.hpp"

namespace pbr {

struct BArgs {
    const void *gout;                      // upstream gradient, [B][3][H][W] contiguous fp32
    void *g_albedo, *g_normal, *g_rough, *g_metal, *g_spec;   // contiguous, NULL = not wanted
    float *g_param_partials;               // PGRAD kernels: [n_tiles][3 + 6 L] per-workgroup sums of the adjoints of
                                           // V (3), the lights' L | position (L x 3) and their intensities (L x 3)
};

// Everything after the loads: forward re-evaluation, chain rule, stores.  `t` holds the lane's texels (as floats), `go` the
// upstream gradient.  s_param / n_param: the PGRAD instantiations' LDS accumulators.
//   `sink(ga, gn, gr, gm, gs)`: what happens to the lane's gradients w.r.t. the texels the shading read -- by default they are
//   stored (backward_body below); the fused blend's backward (ct_blend_backward.hpp) carries them on through the blend.
//   `loss`: NoLoss -- the upstream gradient is `go`, as loaded; MseLoss<VEC> -- the fused rendering-loss step (ct_loss.hip): the
//   upstream gradient of a pixel is formed by the colour adjoint from the colour the forward re-evaluation just produced, 2 (out - target) * scale,
//   and the squared differences it hands back are summed into loss.sq.
//   StackMseLoss<VEC> -- the light-stack step (ct_stack.hip): every light is an image of its own with its own target, so the one-light form
//   (clamp, encode, difference) runs INSIDE the light loop, once per light, and the adjoints of all lights add up in the shared accumulators
//   before the light-independent tail runs once.  `stack` selects that: the light loop runs over a.n_lights although MULTI is false.
//   With PGRAD (the stack-fit step) light l's six sums leave the lane inside the loop, as for MULTI; a lane outside the map carries scale = 0.
//   WeightedStackMseLoss<VEC> -- StackMseLoss with a weight per pixel and shot (ct_stack_weighted.hip): `weighted` selects the colour
//   adjoint that forms d (scale w) and hands back w d d (loss_colour_adjoint).
struct NoLoss { static constexpr bool on = false, stack = false, weighted = false; };
template <int VEC> struct MseLoss {
    static constexpr bool on = true, stack = false, weighted = false;
    float tgt[3][VEC];      // the lane's pixels of the target image
    float scale;            // 2 / N  (d mean((out - target)^2) / d out = scale * (out - target))
    float sq;               // sum of squared differences over the lane's pixels
};
template <int VEC> struct StackMseLoss {
    static constexpr bool on = true, stack = true, weighted = false;
    float tgt[3][VEC];      // the lane's pixels of the CURRENT light's target image
    float scale;            // 2 / N, N = 3 B L H W
    float sq;               // sum of squared differences over the lane's pixels and all lights
    float nxt[3][VEC];      // ... of the NEXT light's image: loaded one light ahead, so that their latency hides behind a light's arithmetic
    const float *lane;      // the lane's first pixel in channel 0 of light 0's image of its material: targets + b L 3 HW + pix (64-bit, by the kernel)
    int64_t plane;          // H W: the images' channel stride; light l's image starts 3 l planes further on
    __device__ __forceinline__ void prefetch(int l) {
#pragma unroll
        for (int c = 0; c < 3; ++c) Ld<float, VEC>::template load<true>(lane, ((int64_t)l * 3 + c) * plane, nxt[c]);
    }
    // light l begins: its pixels were loaded a light ago; the next light's leave now (the last light loads its own again: in bounds, no branch)
    __device__ __forceinline__ void begin_light(int l, int n_lights) {
#pragma unroll
        for (int c = 0; c < 3; ++c)
#pragma unroll
            for (int j = 0; j < VEC; ++j) tgt[c][j] = nxt[c][j];
        prefetch(l + 1 < n_lights ? l + 1 : l);
    }
};
// StackMseLoss with a weight per pixel and shot, one value for the three channels (the weighted light-stack steps: masked captures): the loss
// is mean(w (out - target)^2) over the same 3 B L H W elements.  Shot l + 1's weights leave together with shot l + 1's target pixels, one shot
// ahead, through the same loads; with one plane for all shots (wstep = 0) the one load before the loop is all there is.  A lane outside the map
// reads its clamped position's weight, as it reads that position's targets: every load is in bounds.
template <int VEC> struct WeightedStackMseLoss : StackMseLoss<VEC> {
    static constexpr bool weighted = true;
    float w[VEC];           // the lane's pixels of the CURRENT shot's weight plane
    float wnxt[VEC];        // ... of the NEXT shot's
    const float *wlane;     // the lane's first pixel in shot 0's plane of its material: weights + b w_batch_stride + pix (64-bit, by the kernel)
    int64_t wstep;          // elements from one shot's plane to the next: H W, or 0 for one plane shared by all shots
    __device__ __forceinline__ void prefetch_first() {
        StackMseLoss<VEC>::prefetch(0);
        Ld<float, VEC>::template load<true>(wlane, 0, wnxt);
    }
    __device__ __forceinline__ void begin_light(int l, int n_lights) {
        const int nxt_l = l + 1 < n_lights ? l + 1 : l;
        StackMseLoss<VEC>::begin_light(l, n_lights);
#pragma unroll
        for (int j = 0; j < VEC; ++j) w[j] = wnxt[j];
        if (wstep) Ld<float, VEC>::template load<true>(wlane, (int64_t)nxt_l * wstep, wnxt);      // wave-uniform
    }
};
// The colour adjoint of one image under a loss policy, weighted or not: group g's pixels against `ref`, their targets.
template <class R, class Loss>
__device__ __forceinline__ void loss_colour_adjoint(bool srgb, const R (&uc)[3], const R (&ref)[3], const Loss &loss, int g, R (&g_col)[3], float (&sqd)[3]) {
    if constexpr (Loss::weighted) colour_adjoint(srgb, uc, ref, loss.scale, gather<R>(loss.w, g), g_col, sqd);
    else colour_adjoint<true>(srgb, uc, ref, loss.scale, g_col, sqd);
}

// The way of the light / view sums (PGRAD) out of the lanes: eight of the lane's sums -> their wave totals (wave_sum8: lane l holds value
// (l >> 3) & 7) -> the first n of them added to the workgroup's LDS row, values 0..2 at first3[0..2], values 3.. at rest[0..].
__device__ __forceinline__ void pgrad_add8(float (&v8)[8], int n, float *first3, float *rest) {
    const float w = wave_sum8(v8);
    const int j = (threadIdx.x >> 3) & 7;                    // the value this lane holds the wave total of
    if ((threadIdx.x & 7) == 0 && j < n) atomicAdd(j < 3 ? first3 + j : rest + (j - 3), w);
}

#ifndef PBR_MSE_PACKED
#define PBR_MSE_PACKED 1      // the loss step with fp32 maps in packed pairs too (A/B: build with -DPBR_MSE_PACKED=0)
#endif
template <int LIGHT, int WF, int VEC, bool MULTI, typename TM, bool PGRAD, class Sink, class Loss>
__device__ __forceinline__ void backward_body_to(const KArgs &a, const BArgs &b, const LanePos &p, Texels<VEC> &t, float (&go)[3][VEC],
                                                 float *s_param, int n_param, Sink &&sink, Loss &loss) {
    constexpr bool kPacked = sizeof(TM) == 2 || MULTI || (Loss::on && PBR_MSE_PACKED);
    using R = typename RealOf<VEC, kPacked>::type;
    constexpr int NG = RealOf<VEC, kPacked>::N;
    float accV[3] = {0.0f, 0.0f, 0.0f}, accL[3] = {0.0f, 0.0f, 0.0f}, accI[3] = {0.0f, 0.0f, 0.0f};   // one-light PGRAD
    if (!a.has_normal) {
#pragma unroll
        for (int j = 0; j < VEC; ++j) { t.nm[0][j] = 0.0f; t.nm[1][j] = 0.0f; t.nm[2][j] = 1.0f; }
    }
    const Vec3 V = view_of(a);
    float ys = 0.0f;
    if (LIGHT == PBR_LIGHT_POINT) ys = linspace_at(a.y0, a.y1, a.ystep, a.H_total, p.y + a.y_offset);

    float ga[3][VEC], gn[3][VEC], gr[VEC], gm[VEC], gs[3][VEC];
    R xgrid[NG];
    if (LIGHT == PBR_LIGHT_POINT) x_grid<R, NG, VEC>(a, p.x, xgrid);
#pragma unroll
    for (int g = 0; g < NG; ++g) {
        // ---- forward: decoded colours and their derivatives.  This block and the "light-independent tail" below are bwd_decode's and bwd_tail's
        // statements (ct_chain_rule.hpp: the tiled walk calls them), kept INLINE: handed over through BwdTexelT or a function, in every form tried,
        // the fp32 one-light bodies are scheduled differently and run 0.4-1.4 % slower (profiles/EXPERIMENTS.md).  Change the two together.
        R base[3], dbase[3], f0[3], df0[3], alin[3], kd_scale = splat<R>(1.0f);
        const R m = WF != PBR_WORKFLOW_SPECULAR ? gather<R>(t.me, g) : splat<R>(0.0f);
        const R om = splat<R>(1.0f) - m;
#pragma unroll
        for (int c = 0; c < 3; ++c) {
            const R al = gather<R>(t.al[c], g);
            alin[c] = base[c] = al; dbase[c] = splat<R>(1.0f);
            if (a.albedo_srgb) srgb_to_linear_and_grad(al, base[c], dbase[c]);
            alin[c] = base[c];
            if (WF == PBR_WORKFLOW_METALLIC) {
                f0[c] = fma_(m, base[c], om * kDielectricF0);                  // lerp(0.04, base, m) :107
                df0[c] = splat<R>(0.0f);
            } else if (WF == PBR_WORKFLOW_SPECULAR) {
                const R sp = gather<R>(t.sp[c], g);
                f0[c] = sp; df0[c] = splat<R>(1.0f);
                if (a.spec_srgb) srgb_to_linear_and_grad(sp, f0[c], df0[c]);
            } else {   // CONVERTED: to_diffuse_specular_material (metallic.py:98-108), then the specular workflow
                const R sp = fma_(alin[c], m, om * kDielectricF0);
                base[c] = alin[c] * om;
                f0[c] = sp; df0[c] = splat<R>(1.0f);
                if (a.spec_srgb) srgb_to_linear_and_grad(sp, f0[c], df0[c]);
            }
        }
        if (WF == PBR_WORKFLOW_METALLIC) kd_scale = om;
        const Vec3T<R> nraw = {gather<R>(t.nm[0], g), gather<R>(t.nm[1], g), gather<R>(t.nm[2], g)};
        const R rough = gather<R>(t.ro, g);
        PixelTermsT<R> pt;
        pixel_terms(nraw, V, rough, base, f0, kd_scale, pt);
        const R xs = LIGHT == PBR_LIGHT_POINT ? xgrid[g] : splat<R>(0.0f);
        R ref[3], g_col[3];                          // the upstream value of the group's pixels, with a loss their target; the colour adjoint
        auto load_ref = [&]() {
#pragma unroll
            for (int c = 0; c < 3; ++c) {
                if constexpr (Loss::on) ref[c] = gather<R>(loss.tgt[c], g); else ref[c] = gather<R>(go[c], g);
            }
        };
        const int nl = (MULTI || Loss::stack) ? a.n_lights : 1;
        if constexpr (MULTI) {
            load_ref();
            if constexpr (Loss::on) {
                float sqd[3];
                colour_adjoint_lights<LIGHT, true>(a, a.out_srgb != 0, pt, V, xs, ys, ref, loss.scale, g_col, sqd);
                loss.sq += sqd[0]; loss.sq += sqd[1]; loss.sq += sqd[2];
            } else {
                colour_adjoint_lights<LIGHT>(a, a.out_srgb != 0, pt, V, xs, ys, ref, g_col);
            }
        }
        PixelAdjointT<R> adj;
        adj.clear();
        for (int l = 0; l < nl; ++l) {
            const LightU lu = light_of(a, l);
            const LightGeomT<R> lg = light_geom<LIGHT, R>(lu, V, xs, ys);
            if constexpr (Loss::stack) loss.begin_light(l, nl);
            LightEvalT<R> e;
            eval_light(pt, lg, lu.inten, e);
            if constexpr (!MULTI) {
                load_ref();
                if constexpr (Loss::on) {
                    float sqd[3];
                    loss_colour_adjoint(a.out_srgb != 0, e.uc, ref, loss, g, g_col, sqd);
                    loss.sq += sqd[0]; loss.sq += sqd[1]; loss.sq += sqd[2];
                } else {
                    colour_adjoint(a.out_srgb != 0, e.uc, ref, g_col);
                }
            }
            LightParamAdjT<R> pa;
            backprop_light<LIGHT, PGRAD>(pt, lg, lu.inten, e, g_col, adj, V, pa);
            if constexpr (PGRAD) {
                accV[0] += hsum(pa.g_V.x); accV[1] += hsum(pa.g_V.y); accV[2] += hsum(pa.g_V.z);
                if constexpr (MULTI || Loss::stack) {        // per-light sums leave the lane here: the light loop is a run-time loop
                    float v8[8] = {hsum(pa.g_L.x), hsum(pa.g_L.y), hsum(pa.g_L.z), hsum(pa.g_I[0]), hsum(pa.g_I[1]), hsum(pa.g_I[2]), 0.0f, 0.0f};
                    pgrad_add8(v8, 6, s_param + 3 + 3 * l, s_param + 3 + 3 * a.n_lights + 3 * l);
                } else {
                    accL[0] += hsum(pa.g_L.x); accL[1] += hsum(pa.g_L.y); accL[2] += hsum(pa.g_L.z);
                    accI[0] += hsum(pa.g_I[0]); accI[1] += hsum(pa.g_I[1]); accI[2] += hsum(pa.g_I[2]);
                }
            }
        }
        // ---- light-independent tail
        // kb = kd_scale * base / pi ; kd_scale = 1 - m  (:169-174)
        R g_m = splat<R>(0.0f);
#pragma unroll
        for (int c = 0; c < 3; ++c) {
            R g_base = adj.g_kb[c] * (kd_scale * kInvPi);
            if (WF == PBR_WORKFLOW_METALLIC) {                               // kd_scale = 1 - m; lerp(0.04, base, m)  (:107)
                g_m = fma_(adj.g_kb[c], base[c] * (-kInvPi), g_m);
                g_base = fma_(adj.g_f0[c], m, g_base);
                g_m = fma_(adj.g_f0[c], base[c] - kDielectricF0, g_m);
            } else if (WF == PBR_WORKFLOW_SPECULAR) {
                scatter(gs[c], g, adj.g_f0[c] * df0[c]);
            } else {   // diffuse = a (1-m) ; specular = 0.04 (1-m) + a m
                const R g_sp = adj.g_f0[c] * df0[c], g_diff = adj.g_kb[c] * kInvPi;
                g_base = fma_(g_diff, om, g_sp * m);
                g_m = fma_(g_sp, alin[c] - kDielectricF0, fma_(-g_diff, alin[c], g_m));
            }
            scatter(ga[c], g, g_base * dbase[c]);
        }
        scatter(gm, g, g_m);
        scatter(gr, g, fma_(adj.g_k, (rough + 1.0f) * 0.25f, adj.g_a2 * (rough * 2.0f)));   // k = (r+1)^2/8, a2 = r^2
        // N.V clamp, then F.normalize: g_n = (g - n (n.g)) / |n|
        const R gv = masked(in_unit(pt.ndv_raw, pt.ndv), adj.g_ndv);
        if constexpr (PGRAD) {                                                // N.V (:163): the direct share of V
            accV[0] += hsum(gv * pt.n.x); accV[1] += hsum(gv * pt.n.y); accV[2] += hsum(gv * pt.n.z);
        }
        const Vec3T<R> gnh = {fma_(gv, splat<R>(V.x), adj.g_n.x), fma_(gv, splat<R>(V.y), adj.g_n.y), fma_(gv, splat<R>(V.z), adj.g_n.z)};
        const R rn = rsq(dot_plus(nraw, nraw, 1e-24f));
        const R radial = dot(pt.n, gnh);
        scatter(gn[0], g, (gnh.x - pt.n.x * radial) * rn);
        scatter(gn[1], g, (gnh.y - pt.n.y * radial) * rn);
        scatter(gn[2], g, (gnh.z - pt.n.z * radial) * rn);
    }
    if constexpr (PGRAD) {
        {   // slots 0..2 = V; one light: 3..5 = L, 6..8 = I (n_param = 9), so values 0..7 of the first batch map to slots 0..7
            constexpr bool kPerLight = MULTI || Loss::stack;          // the lights' sums left inside the loop: only V remains
            float v8[8] = {accV[0], accV[1], accV[2], kPerLight ? 0.0f : accL[0], kPerLight ? 0.0f : accL[1], kPerLight ? 0.0f : accL[2],
                           kPerLight ? 0.0f : accI[0], kPerLight ? 0.0f : accI[1]};
            pgrad_add8(v8, kPerLight ? 3 : 8, s_param, s_param + 3);
            if constexpr (!kPerLight) {
                const float wi = wave_sum(accI[2]);
                if ((threadIdx.x & 63) == 0) atomicAdd(&s_param[8], wi);
            }
        }
        __syncthreads();
        for (int i = threadIdx.x; i < n_param; i += blockDim.x) b.g_param_partials[(int64_t)blockIdx.x * n_param + i] = s_param[i];
        if (!p.valid) return;
    }
    sink(ga, gn, gr, gm, gs);
}

template <int LIGHT, int WF, int VEC, bool MULTI, typename TM, bool PGRAD, class Sink>
__device__ __forceinline__ void backward_body_to(const KArgs &a, const BArgs &b, const LanePos &p, Texels<VEC> &t, float (&go)[3][VEC],
                                                 float *s_param, int n_param, Sink &&sink) {
    NoLoss none;
    backward_body_to<LIGHT, WF, VEC, MULTI, TM, PGRAD>(a, b, p, t, go, s_param, n_param, sink, none);
}

// The default sink: the lane's gradients go to the dense gradient planes [B][C][H*W] (the result's channel stride).
template <int WF, int VEC, typename TM>
__device__ __forceinline__ void store_gradients(const KArgs &a, const BArgs &b, const LanePos &p, float (&ga)[3][VEC], float (&gn)[3][VEC],
                                                float (&gr)[VEC], float (&gm)[VEC], float (&gs)[3][VEC]) {
    auto put = [&](void *plane, int channels, int c, const float *v) {
        if (p.sb) Ld<TM, VEC>::template store<St::hinted>(plane_at<TM>(plane, ((int64_t)p.b0 * channels + c) * a.o_cs, (uint32_t)p.pix), 0, v);
        else Ld<TM, VEC>::template store<St::hinted>(plane, ((int64_t)p.b * channels + c) * a.o_cs + p.pix, v);
    };
    if (b.g_albedo) {
#pragma unroll
        for (int c = 0; c < 3; ++c) put(b.g_albedo, 3, c, ga[c]);
    }
    if (b.g_normal && a.has_normal) {
#pragma unroll
        for (int c = 0; c < 3; ++c) put(b.g_normal, 3, c, gn[c]);
    }
    if (b.g_rough) put(b.g_rough, 1, 0, gr);
    if (WF != PBR_WORKFLOW_SPECULAR) {
        if (b.g_metal) put(b.g_metal, 1, 0, gm);
    } else if (b.g_spec) {
#pragma unroll
        for (int c = 0; c < 3; ++c) put(b.g_spec, 3, c, gs[c]);
    }
}

template <int LIGHT, int WF, int VEC, bool MULTI, typename TM, bool PGRAD>
__device__ __forceinline__ void backward_body(const KArgs &a, const BArgs &b, const LanePos &p, Texels<VEC> &t, float (&go)[3][VEC],
                                              float *s_param, int n_param) {
    backward_body_to<LIGHT, WF, VEC, MULTI, TM, PGRAD>(a, b, p, t, go, s_param, n_param,
        [&](float (&ga)[3][VEC], float (&gn)[3][VEC], float (&gr)[VEC], float (&gm)[VEC], float (&gs)[3][VEC]) {
            store_gradients<WF, VEC, TM>(a, b, p, ga, gn, gr, gm, gs);
        });
}

// The frame of every one-wave loss step (cook_torrance_mse_step_kernel in ct_loss.hip, cook_torrance_mse_stack_step_kernel in ct_stack.hip):
// the workgroup's tile -> the lane's position (lanes outside the map shade a clamped position: every lane reaches the wave sum, stores
// nothing and contributes nothing) -> the texels -> `first_targets(p, loss)`, the kernel's own part: it fills the policy's fields and issues
// the loads of the first target pixels, behind the texels' -> backward_body_to with the storing sink -> the wave's sum of squared differences,
// one partial per workgroup, no LDS reduction.  PGRAD: the kernel owns the LDS row s_param[n_param], zeroed before the call; the body
// returns before the sink for lanes outside the map, so the sink needs no guard of its own.
template <int LIGHT, int WF, int VEC, bool MULTI, typename TM, bool PGRAD, class Loss, class FirstTargets>
__device__ __forceinline__ void loss_step(const KArgs &a, const BArgs &b, float *s_param, int n_param, float *partials, FirstTargets &&first_targets) {
    const uint32_t tile = tile_of_workgroup(a, blockIdx.x);
    const int ty = (int)a.div_tx.div(tile);
    const LanePos p = lane_pos<VEC, true>(a, (int)tile - ty * a.tiles_x, ty);
    Texels<VEC> t;
    Loss loss;
    loss.sq = 0.0f;
    float go[3][VEC];                                                              // unused by the loss policies
    load_texels<WF, TM, VEC, true>(a, a.has_normal != 0, p, t);
    first_targets(p, loss);
#pragma unroll
    for (int c = 0; c < 3; ++c)
#pragma unroll
        for (int j = 0; j < VEC; ++j) go[c][j] = 0.0f;
    backward_body_to<LIGHT, WF, VEC, MULTI, TM, PGRAD>(a, b, p, t, go, s_param, n_param,
        [&](float (&ga)[3][VEC], float (&gn)[3][VEC], float (&gr)[VEC], float (&gm)[VEC], float (&gs)[3][VEC]) {
            if (PGRAD || p.valid) store_gradients<WF, VEC, TM>(a, b, p, ga, gn, gr, gm, gs);
        }, loss);
    const float mine = p.valid ? loss.sq : 0.0f;
    const float total = wave_sum(mine);
    if (threadIdx.x == 0) partials[blockIdx.x] = total;
}

//   LIGHT: PBR_LIGHT_*    WF: PBR_WORKFLOW_*    VEC: 4 | 2 | 1    TM: storage type of the maps AND of their gradients
//   (float | __half; arithmetic and the upstream gradient are fp32)
//   PGRAD: also the adjoints of view / light / intensity, summed over the workgroup's pixels into b.g_param_partials
//   (one row per workgroup; param_grad_finish_kernel adds the rows up).  In these instantiations no lane leaves early:
//   lanes outside the map shade a clamped (valid) position with a zero upstream gradient, so that every lane takes
//   part in the wave reductions.
#ifndef PBR_BWD_F16_WAVES
#define PBR_BWD_F16_WAVES 4
#endif
// Two-pixel lanes, one light, fp16 maps: the allocator lands on 129 VGPRs = 3 waves per SIMD, one register past 4 waves.
// (The point-light / converted-workflow body needs four registers more: held to 128 it spilled 20 bytes per lane -- found by the resource scan
// of tools/check_isa.py in round 6, present since round 4 -- so that one instantiation runs three waves per SIMD, without scratch.)
template <int LIGHT, int WF, int VEC, bool MULTI, typename TM, bool PGRAD>
constexpr int bwd_min_waves() {
    if (!(VEC == 2 && !MULTI && !PGRAD && sizeof(TM) == 2)) return 1;
    return LIGHT == PBR_LIGHT_POINT && WF == PBR_WORKFLOW_CONVERTED ? 3 : PBR_BWD_F16_WAVES;
}

template <int LIGHT, int WF, int VEC, bool MULTI, typename TM = float, bool PGRAD = false>
__global__ __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu(bwd_min_waves<LIGHT, WF, VEC, MULTI, TM, PGRAD>())))
void cook_torrance_backward_kernel(const KArgs a, const BArgs b) {
    // Packed two-pixel arithmetic for fp16 maps and for several lights, as in the forward kernels: A/B on 4096^2 maps --
    // fp16 maps 182 us packed vs 194 us scalar; 4 lights fp32 423 us vs 491 us; one light fp32 221 us packed vs 206 us
    // scalar (that launch is bound by the memory system, and there the shorter arithmetic phases only make its 19
    // streams burstier).
    const uint32_t tile = tile_of_workgroup(a, blockIdx.x);
    const int ty = (int)a.div_tx.div(tile);
    const LanePos p = lane_pos<VEC, PGRAD>(a, (int)tile - ty * a.tiles_x, ty);
    if (!PGRAD && !p.valid) return;
    constexpr int kParamSlots = 3 + 6 * PBR_MAX_LIGHTS;
    __shared__ float s_param[PGRAD ? kParamSlots : 1];
    const int n_param = 3 + 6 * a.n_lights;
    if constexpr (PGRAD) {
        for (int i = threadIdx.x; i < n_param; i += blockDim.x) s_param[i] = 0.0f;
        __syncthreads();
    }
    // Texels and upstream gradient in ONE branch-free block per (scalar addresses, normal map) combination: with the flags
    // tested between the loads, the fp16 instantiations close every block with the conversions of its values, i.e. with a wait,
    // and a wave pays three memory round trips (albedo | normal | roughness, metallic | upstream gradient) instead of one.
    Texels<VEC> t;
    float go[3][VEC];
    const int64_t opix = p.b * a.o_bs + p.pix;
    auto load_all = [&](auto sb, auto hn) {
        load_texels_fixed<WF, TM, VEC, true, decltype(sb)::value, decltype(hn)::value>(a, p, t);
#pragma unroll
        for (int c = 0; c < 3; ++c) {
            if constexpr (decltype(sb)::value) Ld<float, VEC>::template load<true>(plane_at<float>(b.gout, p.b0 * a.o_bs + c * a.o_cs, (uint32_t)p.pix), 0, go[c]);
            else Ld<float, VEC>::template load<true>(b.gout, opix + c * a.o_cs, go[c]);
        }
    };
    if constexpr (sizeof(TM) == 4) {            // fp32 maps: no conversions, no waits -- and the paced form measures 1 % faster (ct_kernel.hpp)
        load_texels<WF, TM, VEC, true>(a, a.has_normal != 0, p, t);
#pragma unroll
        for (int c = 0; c < 3; ++c) {
            if (p.sb) Ld<float, VEC>::template load<true>(plane_at<float>(b.gout, p.b0 * a.o_bs + c * a.o_cs, (uint32_t)p.pix), 0, go[c]);
            else Ld<float, VEC>::template load<true>(b.gout, opix + c * a.o_cs, go[c]);
        }
    } else if (p.sb) {
        if (a.has_normal) load_all(std::true_type{}, std::true_type{}); else load_all(std::true_type{}, std::false_type{});
    } else {
        if (a.has_normal) load_all(std::false_type{}, std::true_type{}); else load_all(std::false_type{}, std::false_type{});
    }
    if (PGRAD && !p.valid) {
#pragma unroll
        for (int c = 0; c < 3; ++c)
#pragma unroll
            for (int j = 0; j < VEC; ++j) go[c][j] = 0.0f;
    }
    backward_body<LIGHT, WF, VEC, MULTI, TM, PGRAD>(a, b, p, t, go, s_param, n_param);
}

}  // namespace pbr
