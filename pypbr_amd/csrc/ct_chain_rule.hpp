// ct_chain_rule.hpp -- the hand-written chain rule of the fused Cook-Torrance evaluation: the mathematics only, no kernel, no loads, no stores.
// Every kernel that differentiates the render runs on these functions, through backward_body_to (ct_backward.hpp) or the walk over tiled
// maps (ct_repeat_backward.hpp).  One exception, on purpose: backward_body_to carries bwd_decode's and bwd_tail's statements inline (its
// comment says why).  Per pixel group: bwd_decode (light-independent forward terms and the decodes' slopes), colour_adjoint (one light) or
// colour_adjoint_lights (several), backprop_light per light into a PixelAdjointT, bwd_tail (-> gradients w.r.t. the stored texels).
//
// Sub-gradient conventions are torch's, because that is what the reference's autograd graph uses: clamp passes the gradient on the closed
// interval [min, max]; the piecewise sRGB functions differentiate the branch the value takes; lerp(0.04, base, m) gives m to base and
// sum_c(base_c - 0.04) to the single-channel metallic map; F.normalize projects out the radial component.  Light geometry does not depend on
// the maps.
//
// Like brdf_math.hpp the chain rule is written over the real type R: float, or f32x2 = the lane's pixels two at a
// time, so that its adds / multiplies / fmas are packed instructions; branches on per-pixel conditions are selects.
#pragma once
#include "ct_kernel.hpp"

namespace pbr {

// Adjoints of one light's parameters, for the lane's pixel group (the reference's autograd reaches view_dir,
// light_dir_or_position and light_intensity: cooktorrance.py:95-96, :126-140 are plain torch ops on them).
template <class R> struct LightParamAdjT {
    Vec3T<R> g_L;     // directional: adjoint of the normalised L; point: of the light position
    Vec3T<R> g_V;     // this light's share of the adjoint of the normalised view vector (through h = V + L and Hv.V)
    R g_I[3];
};

__device__ __forceinline__ float hsum(float v) { return v; }
__device__ __forceinline__ float hsum(f32x2 v) { return v.x + v.y; }
__device__ __forceinline__ float wave_sum(float v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
    return v;
}
// Sums EIGHT values over the wave with 10 exchanges instead of 48: three halving steps (lanes whose bit 5 / 4 / 3 is set keep
// the upper half of the values and send the lower one, the others the opposite), then a 3-step butterfly on the one value
// left.  Lane l ends up with the wave total of value number (l >> 3) & 7, the same in all 8 lanes that share those bits.
template <int C, int M>
__device__ __forceinline__ void wave_halve(float (&v)[8], bool up) {     // C values -> C / 2: exchange across lane bit M
#pragma unroll
    for (int j = 0; j < C / 2; ++j) {
        const float keep = up ? v[j + C / 2] : v[j], send = up ? v[j] : v[j + C / 2];
        v[j] = keep + __shfl_xor(send, M, 64);
    }
}
__device__ __forceinline__ float wave_sum8(float (&v)[8]) {
    const int lane = threadIdx.x & 63;
    wave_halve<8, 32>(v, (lane & 32) != 0);
    wave_halve<4, 16>(v, (lane & 16) != 0);
    wave_halve<2, 8>(v, (lane & 8) != 0);
    float t = v[0];
#pragma unroll
    for (int o = 4; o > 0; o >>= 1) t += __shfl_xor(t, o, 64);
    return t;
}

template <class R> using MaskT = typename MaskOf<R>::type;
template <class R> __device__ __forceinline__ MaskT<R> in_unit(R x) {
    return and_(ge_(x, splat<R>(0.0f)), le_(x, splat<R>(1.0f)));
}
template <class R> __device__ __forceinline__ R masked(MaskT<R> m, R x) { return select_(m, x, splat<R>(0.0f)); }
// 0 <= x <= 1 given clamp01(x), which the forward terms already hold: one compare per value instead of two.
template <class R> __device__ __forceinline__ MaskT<R> in_unit(R x, R clamped) { return eq_(clamped, x); }

// utils.srgb_to_linear and its derivative from ONE log / exp pair: with u = clamp(x) + 0.055 and
// e = (u / 1.055)^1.4 = exp2(1.4 log2 u - 1.4 log2 1.055), the value is e u / 1.055 and the slope 2.4 e / 1.055.
template <class R> __device__ __forceinline__ void srgb_to_linear_and_grad(R x, R &value, R &slope) {
    const R t = clamp01(x), u = t + 0.055f;
    const R e = exp2_hw(fma_(splat<R>(1.4f), log2_hw(u), splat<R>(-0.10814020f) /* 1.4*log2(1.055) */));
    const MaskT<R> low = le_(t, splat<R>(0.04045f));
    value = select_(low, t * (1.0f / 12.92f), (e * u) * (1.0f / 1.055f));
    slope = masked(in_unit(x, t), select_(low, splat<R>(1.0f / 12.92f), e * 2.2748815f /* 2.4/1.055 */));
}

// d/dc of utils.linear_to_srgb (functions.py:50-66) for c already in [0,1].
template <class R> __device__ __forceinline__ R linear_to_srgb_grad_unit(R c) {
    const R hi = exp2_hw(log2_hw(c) * (1.0f / 2.4f - 1.0f)) * 0.43958333f /* 1.055/2.4 */;
    return select_(le_(c, splat<R>(0.0031308f)), splat<R>(12.92f), hi);
}

// utils.linear_to_srgb (functions.py:50-66) and its derivative for c already in [0,1], from ONE log2 (the loss steps need both of the
// same value): the two functions above / in brdf_math.hpp evaluate log2_hw(c) each -- the very same instruction on the very same operand,
// which the compiler does not merge across their inline assembly.  Same statements otherwise: bit-identical to calling them separately.
template <class R> __device__ __forceinline__ void linear_to_srgb_unit_and_grad(R c, R &value, R &slope) {
    const R l = log2_hw(c);
    const MaskT<R> low = le_(c, splat<R>(0.0031308f));
    const R hi = fma_sat_after_trans(splat<R>(1.055f), exp2_hw(l * (1.0f / 2.4f)), splat<R>(-0.055f));
    value = select_(low, c * 12.92f, hi);
    slope = select_(low, splat<R>(12.92f), exp2_hw(l * (1.0f / 2.4f - 1.0f)) * 0.43958333f /* 1.055/2.4 */);
}

// Forward terms of one (pixel, light) pair that the chain rule needs again.
template <class R> struct LightEvalT {
    R ndl_raw, ndl, c, s2, den, dl, dD, ds, q, dg, rad;
    MaskT<R> nh_pos;
    R F[3], u[3], uc[3];      // uc = clamp01(u): the light's clamped contribution, also the test of the clamp's sub-gradient
};

template <class R>
__device__ __forceinline__ void eval_light(const PixelTermsT<R> &t, const LightGeomT<R> &g, const float inten[3], LightEvalT<R> &e) {
    e.ndl_raw = dot(t.n, g.d) * g.rinv;                             // N.L = (N.d) rinv: the forward kernels' form (shade_light), L never formed
    e.ndl = clamp01(e.ndl_raw);
    const R nh = e.ndl_raw + t.ndv_raw;                              // N.h = N.L + N.V
    e.den = ggx_den(t, g, nh, e.s2, e.nh_pos);
    e.c = masked(e.nh_pos, nh * g.rh);                               // clamp(N.H), :215
    e.dl = fma_(e.ndl, t.omk, t.kk);
    e.dD = fma_(e.den * e.den, splat<R>(kPi), splat<R>(1e-7f));
    e.ds = fma_(t.ndv * 4.0f, e.ndl, splat<R>(1e-7f));
    e.q = rcp((e.dD * t.dv) * (e.dl * e.ds));
    e.dg = t.a2ndv * e.ndl * e.q;
    e.rad = e.ndl * g.att;
#pragma unroll
    for (int ch = 0; ch < 3; ++ch) {
        e.F[ch] = fma_(t.f0[ch], g.om5, g.p5);
        e.u[ch] = fma_(e.F[ch], e.dg - t.kb[ch], t.kb[ch]) * (e.rad * inten[ch]);
        e.uc[ch] = clamp01(e.u[ch]);
    }
}

// Accumulators that do not depend on the light.
template <class R> struct PixelAdjointT {
    R g_kb[3];            // adjoint of kb = kd_scale * base / pi
    R g_f0[3];
    R g_a2, g_k, g_ndv;
    Vec3T<R> g_n;         // adjoint of the unit normal
    __device__ __forceinline__ void clear() {
#pragma unroll
        for (int c = 0; c < 3; ++c) { g_kb[c] = splat<R>(0.0f); g_f0[c] = splat<R>(0.0f); }
        g_a2 = g_k = g_ndv = splat<R>(0.0f);
        g_n = {splat<R>(0.0f), splat<R>(0.0f), splat<R>(0.0f)};
    }
};

// Chain rule through one light's contribution, given the adjoint of its clamped colour.
template <int LIGHT, bool PG, class R, class VT>
__device__ __forceinline__ void backprop_light(const PixelTermsT<R> &t, const LightGeomT<R> &g, const float inten[3],
                                               const LightEvalT<R> &e, const R g_col[3], PixelAdjointT<R> &adj,
                                               const VT &V, LightParamAdjT<R> &pa) {
    R g_dg = splat<R>(0.0f), g_rad = splat<R>(0.0f), g_p5 = splat<R>(0.0f);
#pragma unroll
    for (int ch = 0; ch < 3; ++ch) {
        const R gu = masked(in_unit(e.u[ch], e.uc[ch]), g_col[ch]);          // clamp :177
        const R S = fma_(e.F[ch], e.dg - t.kb[ch], t.kb[ch]);                // F dg + (1 - F) kb
        const R gS = gu * (e.rad * inten[ch]);
        g_rad = fma_(gu * S, splat<R>(inten[ch]), g_rad);
        adj.g_kb[ch] = fma_(gS, splat<R>(1.0f) - e.F[ch], adj.g_kb[ch]);
        g_dg = fma_(gS, e.F[ch], g_dg);
        const R gF = gS * (e.dg - t.kb[ch]);
        adj.g_f0[ch] = fma_(gF, g.om5, adj.g_f0[ch]);                        // F = f0 + (1-f0) p5, :196
        if constexpr (PG) {
            g_p5 = fma_(gF, splat<R>(1.0f) - t.f0[ch], g_p5);
            pa.g_I[ch] = (gu * S) * e.rad;                                   // u = S rad I   (:175-176)
        }
    }
    R g_ndl = g_rad * g.att;                                                 // :175
    // dg = (a2 ndv ndl) q,  q = 1 / (dD dv dl ds)
    const R g_num = g_dg * e.q;
    const R g_Q = -(g_dg * e.dg) * e.q;                                      // adjoint of the product dD dv dl ds
    adj.g_a2 = fma_(g_num, t.ndv * e.ndl, adj.g_a2);
    R g_ndv = g_num * t.a2 * e.ndl;
    g_ndl = fma_(g_num, t.a2ndv, g_ndl);
    const R dvdl = t.dv * e.dl, dDds = e.dD * e.ds;
    const R g_dD = g_Q * (dvdl * e.ds);
    const R g_dv = g_Q * (dDds * e.dl);
    const R g_dl = g_Q * (dDds * t.dv);
    const R g_ds = g_Q * (dvdl * e.dD);
    // dD = pi den^2 + 1e-7 ; den = c^2 (a2 - 1) + 1  (:216-217)
    const R g_den = masked(e.nh_pos, g_dD * (2.0f * kPi) * e.den);
    adj.g_a2 = fma_(g_den, splat<R>(1.0f) - e.s2, adj.g_a2);                 // d den / d a2 = c^2
    const R g_c = masked(in_unit(e.c), g_den * 2.0f * e.c * (t.a2 - 1.0f));
    // dv = ndv (1-k) + k + 1e-7 ; dl likewise ; ds = 4 ndv ndl + 1e-7
    g_ndv = fma_(g_dv, t.omk, g_ndv);
    adj.g_k = fma_(g_dv, splat<R>(1.0f) - t.ndv, adj.g_k);
    g_ndl = fma_(g_dl, t.omk, g_ndl);
    adj.g_k = fma_(g_dl, splat<R>(1.0f) - e.ndl, adj.g_k);
    g_ndv = fma_(g_ds, e.ndl * 4.0f, g_ndv);
    g_ndl = fma_(g_ds, t.ndv * 4.0f, g_ndl);
    adj.g_ndv = adj.g_ndv + g_ndv;                                           // N.V does not depend on the light
    // dots -> unit normal (clamps pass on the closed interval); c = N . h / |h|
    const R gl = masked(in_unit(e.ndl_raw, e.ndl), g_ndl);
    const R gch = g_c * g.rh, glr = gl * g.rinv;                             // d N.L / d n = L = d rinv
    adj.g_n.x = fma_(glr, g.d.x, fma_(gch, g.h.x, adj.g_n.x));
    adj.g_n.y = fma_(glr, g.d.y, fma_(gch, g.h.y, adj.g_n.y));
    adj.g_n.z = fma_(glr, g.d.z, fma_(gch, g.h.z, adj.g_n.z));
    if constexpr (PG) {
        // ---- light / view parameters.  h = V + L (un-normalised); c = (n.h)/|h| (:215), cos = clamp((h.V)/|h|) (:156-158),
        // p5 = (1 - cos)^5 (:196).  d(x.h / |h|)/dh = (x - (x.h / |h|^2) h) / |h|.
        const R rh = g.rh;
        const R hv = dotv(g.h, V);
        const R cos_raw = hv * rh;
        const R om = splat<R>(1.0f) - clamp01(cos_raw), om2 = om * om;
        const R gcs = masked(in_unit(cos_raw), g_p5 * (om2 * om2) * -5.0f) * rh;
        const R nhr = (e.ndl_raw + t.ndv_raw) * g.rhh, hvr = hv * g.rhh;
        const R wh = fma_(gch, nhr, gcs * hvr);                              // g_h = gch n + gcs V - wh h
        const Vec3T<R> g_h = {fma_(gch, t.n.x, fma_(gcs, as_real<R>(V.x), -wh * g.h.x)),
                              fma_(gch, t.n.y, fma_(gcs, as_real<R>(V.y), -wh * g.h.y)),
                              fma_(gch, t.n.z, fma_(gcs, as_real<R>(V.z), -wh * g.h.z))};
        pa.g_V = {fma_(gcs, g.h.x, g_h.x), fma_(gcs, g.h.y, g_h.y), fma_(gcs, g.h.z, g_h.z)};   // + the direct V of Hv.V
        const Vec3T<R> g_Ld = {fma_(gl, t.n.x, g_h.x), fma_(gl, t.n.y, g_h.y), fma_(gl, t.n.z, g_h.z)};   // N.L and h
        if (LIGHT == PBR_LIGHT_POINT) {
            // L = d rinv, rinv = 1/(|d| + 1e-7) (:139); att = 1/(|d|^2 + 1e-7) (:140); rad = ndl att (:175)
            const R g_rinv = dot(g_Ld, g.d);
            const R g_att = g_rad * e.ndl;
            const R coef = fma_(g_rinv * g.rdist, -(g.rinv * g.rinv), (g_att * -2.0f) * (g.att * g.att));
            pa.g_L = {fma_(g_Ld.x, g.rinv, coef * g.d.x), fma_(g_Ld.y, g.rinv, coef * g.d.y), fma_(g_Ld.z, g.rinv, coef * g.d.z)};
        } else {
            pa.g_L = g_Ld;
        }
    }
}

// Forward decode of one pixel group, as the chain rule needs it again (cooktorrance.py:99-118 and the conversions it calls):
// decoded colours and their derivatives, F0, the stored normal and roughness, the light-independent PixelTerms.
template <class R> struct BwdTexelT {
    R base[3], dbase[3], f0[3], df0[3], alin[3];
    R m, om, kd_scale, rough;
    Vec3T<R> nraw;
    PixelTermsT<R> pt;
};

template <int WF, int VEC, class R, class VT>
__device__ __forceinline__ void bwd_decode(const KArgs &a, const Texels<VEC> &t, int g, const VT &V, BwdTexelT<R> &x) {
    x.kd_scale = splat<R>(1.0f);
    x.m = WF != PBR_WORKFLOW_SPECULAR ? gather<R>(t.me, g) : splat<R>(0.0f);
    x.om = splat<R>(1.0f) - x.m;
#pragma unroll
    for (int c = 0; c < 3; ++c) {
        const R al = gather<R>(t.al[c], g);
        x.alin[c] = x.base[c] = al; x.dbase[c] = splat<R>(1.0f);
        if (a.albedo_srgb) srgb_to_linear_and_grad(al, x.base[c], x.dbase[c]);
        x.alin[c] = x.base[c];
        if (WF == PBR_WORKFLOW_METALLIC) {
            x.f0[c] = fma_(x.m, x.base[c], x.om * kDielectricF0);                  // lerp(0.04, base, m) :107
            x.df0[c] = splat<R>(0.0f);
        } else if (WF == PBR_WORKFLOW_SPECULAR) {
            const R sp = gather<R>(t.sp[c], g);
            x.f0[c] = sp; x.df0[c] = splat<R>(1.0f);
            if (a.spec_srgb) srgb_to_linear_and_grad(sp, x.f0[c], x.df0[c]);
        } else {   // CONVERTED: to_diffuse_specular_material (metallic.py:98-108), then the specular workflow
            const R sp = fma_(x.alin[c], x.m, x.om * kDielectricF0);
            x.base[c] = x.alin[c] * x.om;
            x.f0[c] = sp; x.df0[c] = splat<R>(1.0f);
            if (a.spec_srgb) srgb_to_linear_and_grad(sp, x.f0[c], x.df0[c]);
        }
    }
    if (WF == PBR_WORKFLOW_METALLIC) x.kd_scale = x.om;
    x.nraw = {gather<R>(t.nm[0], g), gather<R>(t.nm[1], g), gather<R>(t.nm[2], g)};
    x.rough = gather<R>(t.ro, g);
    pixel_terms(x.nraw, V, x.rough, x.base, x.f0, x.kd_scale, x.pt);
}

// The colour adjoint: the adjoint of a clamped linear colour `lin` (:177) behind the output encode (:179-180).  With a loss two steps, which
// the tiled kernel takes apart around its sum: the encode's value and slope from one log2, then the upstream value through that slope.
template <class R> __device__ __forceinline__ void encode_and_slope(bool srgb, R lin, R &out, R &slope) {
    out = lin; slope = splat<R>(1.0f);
    if (srgb) linear_to_srgb_unit_and_grad(lin, out, slope);
}
template <class R> __device__ __forceinline__ R behind_encode(bool srgb, R up, R slope) { return srgb ? up * slope : up; }
// Per channel.  `ref`: the upstream value of the encoded colour, or with LOSS the target -- then the upstream value is (out - ref) scale,
// formed here, and `sqd` receives the squared difference over the group's pixels (whose sum it joins is the caller's).
template <bool LOSS, class R>
__device__ __forceinline__ R colour_adjoint(bool srgb, R lin, R ref, float scale, float &sqd) {
    if constexpr (LOSS) {
        R out, slope;
        encode_and_slope(srgb, lin, out, slope);
        const R d = out - ref;
        sqd = hsum(d * d);
        return behind_encode(srgb, d * scale, slope);
    } else {
        return srgb ? ref * linear_to_srgb_grad_unit(lin) : ref;       // (the slope alone: no value, and no log2 where there is no encode)
    }
}
// ONE light: `uc` is the light's clamped colour (backprop_light applies that clamp's mask).
template <bool LOSS, class R>
__device__ __forceinline__ void colour_adjoint(bool srgb, const R (&uc)[3], const R (&ref)[3], float scale, R (&g_col)[3], float (&sqd)[3]) {
#pragma unroll
    for (int c = 0; c < 3; ++c) g_col[c] = colour_adjoint<LOSS>(srgb, uc[c], ref[c], scale, sqd[c]);
}
// ... with a weight `w` per pixel, the same for the three channels (the weighted light-stack steps): the loss is mean(w (out - ref)^2), so the
// upstream value is d (scale w) and `sqd` receives w d d.  A weight of exactly 0 beside finite values gives exactly +-0 in both; nothing is
// tested, so 0 * NaN stays NaN.
template <class R>
__device__ __forceinline__ void colour_adjoint(bool srgb, const R (&uc)[3], const R (&ref)[3], float scale, R w, R (&g_col)[3], float (&sqd)[3]) {
    const R ws = w * scale;
#pragma unroll
    for (int c = 0; c < 3; ++c) {
        R out, slope;
        encode_and_slope(srgb, uc[c], out, slope);
        const R d = out - ref[c];
        sqd[c] = hsum(w * d * d);
        g_col[c] = behind_encode(srgb, d * ws, slope);
    }
}
// SEVERAL lights (H12: per-light clamp, sum, clamp, encode), the same adjoint for all of them: pass 1 over the lights -- the summed colour
// decides the outer clamp, and the encode is taken at clamp01(sum).  Pass 2, every light's backprop_light with this g_col, is the caller's.
template <int LIGHT, bool LOSS, class R, class VT>
__device__ __forceinline__ void colour_adjoint_lights(const KArgs &a, bool srgb, const PixelTermsT<R> &pt, const VT &V, R xs, float ys,
                                                      const R (&ref)[3], float scale, R (&g_col)[3], float (&sqd)[3]) {
    R sum[3] = {splat<R>(0.0f), splat<R>(0.0f), splat<R>(0.0f)};
    for (int l = 0; l < a.n_lights; ++l) {
        const LightU lu = light_of(a, l);
        LightEvalT<R> e;
        eval_light(pt, light_geom<LIGHT, R>(lu, V, xs, ys), lu.inten, e);
#pragma unroll
        for (int c = 0; c < 3; ++c) sum[c] = sum[c] + e.uc[c];
    }
#pragma unroll
    for (int c = 0; c < 3; ++c) g_col[c] = masked(in_unit(sum[c]), colour_adjoint<LOSS>(srgb, clamp01(sum[c]), ref[c], scale, sqd[c]));
}
// The same two without a loss: `up` is the upstream value, nothing else goes in or comes back.
template <class R> __device__ __forceinline__ void colour_adjoint(bool srgb, const R (&uc)[3], const R (&up)[3], R (&g_col)[3]) {
    float none[3];
    colour_adjoint<false>(srgb, uc, up, 0.0f, g_col, none);
}
template <int LIGHT, class R, class VT>
__device__ __forceinline__ void colour_adjoint_lights(const KArgs &a, bool srgb, const PixelTermsT<R> &pt, const VT &V, R xs, float ys, const R (&up)[3], R (&g_col)[3]) {
    float none[3];
    colour_adjoint_lights<LIGHT, false>(a, srgb, pt, V, xs, ys, up, 0.0f, g_col, none);
}

// The light-independent tail of the chain rule: adjoints of kb / f0 / a2 / k / N.V / the unit normal -> gradients w.r.t. the stored texels
// of group g, scattered into the lane's gradient arrays (gs: the specular workflow only).  Hands back gv, the adjoint of the clamped N.V:
// with the light / view adjoints it carries the direct share of V (gv n).
template <int WF, int VEC, class R, class VT>
__device__ __forceinline__ R bwd_tail(const BwdTexelT<R> &x, const PixelAdjointT<R> &adj, const VT &V, int g, float (&ga)[3][VEC],
                                      float (&gn)[3][VEC], float (&gr)[VEC], float (&gm)[VEC], float (&gs)[3][VEC]) {
    // kb = kd_scale * base / pi ; kd_scale = 1 - m  (:169-174)
    R g_m = splat<R>(0.0f);
#pragma unroll
    for (int c = 0; c < 3; ++c) {
        R g_base = adj.g_kb[c] * (x.kd_scale * kInvPi);
        if (WF == PBR_WORKFLOW_METALLIC) {                               // kd_scale = 1 - m; lerp(0.04, base, m)  (:107)
            g_m = fma_(adj.g_kb[c], x.base[c] * (-kInvPi), g_m);
            g_base = fma_(adj.g_f0[c], x.m, g_base);
            g_m = fma_(adj.g_f0[c], x.base[c] - kDielectricF0, g_m);
        } else if (WF == PBR_WORKFLOW_SPECULAR) {
            scatter(gs[c], g, adj.g_f0[c] * x.df0[c]);
        } else {   // diffuse = a (1-m) ; specular = 0.04 (1-m) + a m
            const R g_sp = adj.g_f0[c] * x.df0[c], g_diff = adj.g_kb[c] * kInvPi;
            g_base = fma_(g_diff, x.om, g_sp * x.m);
            g_m = fma_(g_sp, x.alin[c] - kDielectricF0, fma_(-g_diff, x.alin[c], g_m));
        }
        scatter(ga[c], g, g_base * x.dbase[c]);
    }
    scatter(gm, g, g_m);
    scatter(gr, g, fma_(adj.g_k, (x.rough + 1.0f) * 0.25f, adj.g_a2 * (x.rough * 2.0f)));   // k = (r+1)^2/8, a2 = r^2
    // N.V clamp, then F.normalize: g_n = (g - n (n.g)) / |n|
    const R gv = masked(in_unit(x.pt.ndv_raw, x.pt.ndv), adj.g_ndv);
    const Vec3T<R> gnh = {fma_(gv, as_real<R>(V.x), adj.g_n.x), fma_(gv, as_real<R>(V.y), adj.g_n.y), fma_(gv, as_real<R>(V.z), adj.g_n.z)};
    const R rn = rsq(dot_plus(x.nraw, x.nraw, 1e-24f));
    const R radial = dot(x.pt.n, gnh);
    scatter(gn[0], g, (gnh.x - x.pt.n.x * radial) * rn);
    scatter(gn[1], g, (gnh.y - x.pt.n.y * radial) * rn);
    scatter(gn[2], g, (gnh.z - x.pt.n.z * radial) * rn);
    return gv;
}

}  // namespace pbr
