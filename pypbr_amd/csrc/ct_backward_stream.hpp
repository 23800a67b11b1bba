// ct_backward_stream.hpp -- the streamed form of the backward kernel (fp16 maps, one light), hand-scheduled; its body is shared with the
// streamed rendering-loss step (ct_loss.hip).  The chain rule it runs per tile is backward_body_to's (ct_backward.hpp).
#pragma once
#include "ct_backward.hpp"

namespace pbr {

// With fp16 maps the backward pass moves 44 B per pixel and is bound by instruction issue, not by HBM: a one-tile wave
// spends about as long being dispatched, forming its 19 plane addresses and waiting for its first loads as it spends
// computing, and its 4 waves per SIMD (125 VGPRs) cannot cover that: the VALUs idle a third of the time.  Here the grid is as many
// waves as the chip holds at once (or a small multiple), and wave w of a material walks its 128-pixel tiles w, w + G,
// w + 2 G ... (G = waves per material): at any moment the chip works on one compact window of every plane, as with
// one-tile waves, every wave does the same amount of work (no tail round), and the texels and the upstream gradient of the NEXT tile travel global ->
// LDS (global_load_lds_dword: no VGPR destination, so the prefetch costs no registers) while the current tile is
// differentiated from registers; 3 waves per SIMD (the loop needs 124-150 VGPRs; a fourth wave measured level).  Per tile: 8 (10) map planes x 256 B + 3 gradient
// planes x 512 B = 3.5 (4) KiB of LDS per wave, ONE buffer -- a tile's values are copied to registers (11 ds_reads)
// before the next tile's loads are issued into the same buffer.  Plane addresses, the material index and the light block
// are formed once per wave; a tile costs a scalar row / column split and the lane-constant offset.  Same backward_body as
// cook_torrance_backward_kernel<.., 2, false, __half, false>: bit-identical gradients.
//   Requires (checked by the launcher): one light, untiled maps, W % 128 == 0, planes below 2^30 pixels, every plane
//   4-byte aligned with even strides, no light / view adjoints.
#ifndef PBR_BWD_STREAM_WAVES
#define PBR_BWD_STREAM_WAVES 3
#endif
constexpr int kStreamWavesPerSimd = PBR_BWD_STREAM_WAVES;
constexpr int kStreamMapPlanes = 10;                                 // albedo 3, normal 3, roughness, metallic | specular 3
constexpr int kStreamLdsWords = kStreamMapPlanes * 64 + 3 * 128;
typedef __attribute__((address_space(3))) void *lds_ptr;

// One LDS-DMA load: lane l's dword goes to LDS byte OFF + 4 l of the tile buffer.  M0 (the LDS base of the instruction) is
// the buffer for EVERY load of the kernel -- the plane's place inside it travels in the instruction's offset field, which
// the hardware adds to the global address too, so the plane's (scalar) base is biased by -OFF: no s_mov m0 + wait state
// per load (14 loads per tile).
template <typename T, int OFF>
__device__ __forceinline__ void dma_dword(const void *plane, int64_t uniform_elems, uint32_t lane_elems, uint32_t *buf) {
    const uint64_t base = reinterpret_cast<uint64_t>(plane) + (uint64_t)uniform_elems * sizeof(T) - (uint64_t)OFF;
    const __attribute__((address_space(1))) void *g = (const __attribute__((address_space(1))) void *)(reinterpret_cast<global_ptr>(base) + lane_elems * (uint32_t)sizeof(T));
    __builtin_amdgcn_global_load_lds(g, (lds_ptr)buf, 4, OFF, 2);
}

// The body, shared with the streamed rendering-loss step (ct_loss.hip): with a Loss policy `b.gout` is the TARGET image -- same three fp32
// planes, same DMA slots -- and the upstream gradient is formed from it inside backward_body_to.
template <int LIGHT, int WF, bool FULL, class Loss>
__device__ __forceinline__ void backward_stream_body(const KArgs &a, const BArgs &b, const int tiles_per_material, const int n_stores, uint32_t *buf, Loss &loss) {
    const int lane = threadIdx.x, mat = blockIdx.y;
    const int t0 = blockIdx.x, t1 = tiles_per_material, step = gridDim.x;      // tiles t0, t0 + step, ... of material `mat`
    if (FULL) {      // the usual rendering-loss launch: sRGB in and out, a normal map, every gradient wanted -- no flag branches
        // exactly the facts the launcher has checked for this workflow (a false assumption would be undefined behaviour): the
        // specular decode flag only where the workflow reads it, the metallic | specular gradient only where it is written
        __builtin_assume(a.albedo_srgb != 0); __builtin_assume(a.out_srgb != 0); __builtin_assume(a.has_normal != 0);
        __builtin_assume(b.g_albedo != nullptr); __builtin_assume(b.g_normal != nullptr); __builtin_assume(b.g_rough != nullptr);
        if (WF != PBR_WORKFLOW_METALLIC) __builtin_assume(a.spec_srgb != 0);
        if (WF == PBR_WORKFLOW_SPECULAR) __builtin_assume(b.g_spec != nullptr); else __builtin_assume(b.g_metal != nullptr);
    }
    const bool has_normal = FULL || a.has_normal != 0;
    auto issue = [&](int t) {
        const uint32_t l2 = (uint32_t)t * 128u + 2u * lane, l1 = (uint32_t)t * 128u + lane;   // lane offsets in pixels: pairs | singles
        dma_dword<__half, 0 * 256>(a.albedo, mat * a.a_bs, l2, buf);
        dma_dword<__half, 1 * 256>(a.albedo, mat * a.a_bs + a.a_cs, l2, buf);
        dma_dword<__half, 2 * 256>(a.albedo, mat * a.a_bs + 2 * a.a_cs, l2, buf);
        if (has_normal) {
            dma_dword<__half, 3 * 256>(a.normal, mat * a.n_bs, l2, buf);
            dma_dword<__half, 4 * 256>(a.normal, mat * a.n_bs + a.n_cs, l2, buf);
            dma_dword<__half, 5 * 256>(a.normal, mat * a.n_bs + 2 * a.n_cs, l2, buf);
        }
        dma_dword<__half, 6 * 256>(a.rough, mat * a.r_bs, l2, buf);
        if (WF != PBR_WORKFLOW_SPECULAR) {
            dma_dword<__half, 7 * 256>(a.metal, mat * a.m_bs, l2, buf);
        } else {
            dma_dword<__half, 7 * 256>(a.spec, mat * a.s_bs, l2, buf);
            dma_dword<__half, 8 * 256>(a.spec, mat * a.s_bs + a.s_cs, l2, buf);
            dma_dword<__half, 9 * 256>(a.spec, mat * a.s_bs + 2 * a.s_cs, l2, buf);
        }
        constexpr int G = kStreamMapPlanes * 256;                // the upstream gradient: 128 floats per plane, two loads each
        dma_dword<float, G + 0>(b.gout, mat * a.o_bs, l1, buf);
        dma_dword<float, G + 256>(b.gout, mat * a.o_bs + 64, l1, buf);
        dma_dword<float, G + 512>(b.gout, mat * a.o_bs + a.o_cs, l1, buf);
        dma_dword<float, G + 768>(b.gout, mat * a.o_bs + a.o_cs + 64, l1, buf);
        dma_dword<float, G + 1024>(b.gout, mat * a.o_bs + 2 * a.o_cs, l1, buf);
        dma_dword<float, G + 1280>(b.gout, mat * a.o_bs + 2 * a.o_cs + 64, l1, buf);
    };
    // The tile's values leave LDS through hand-written ds_reads: for an LDS read the compiler can see it waits until EVERY
    // vector-memory operation in flight has finished (it knows the buffer is the target of LDS-DMA loads, not which of
    // them) -- that includes the previous tile's stores, a full write round trip per tile.
    const uint32_t lds0 = (uint32_t)(size_t)(lds_ptr)buf;
    const uint32_t at4 = lds0 + 4u * lane, at8 = lds0 + kStreamMapPlanes * 256u + 8u * lane;
    issue(t0);
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    for (int t = t0; t < t1; t += step) {
        // the tile's loads were issued BEFORE the previous tile's stores (vmcnt counts both, in order): when at most the
        // stores are still in flight, the loads have landed
        if (FULL && WF != PBR_WORKFLOW_SPECULAR) asm volatile("s_waitcnt vmcnt(8)" ::: "memory");
        else if (FULL) asm volatile("s_waitcnt vmcnt(10)" ::: "memory");
        else if (n_stores == 8) asm volatile("s_waitcnt vmcnt(8)" ::: "memory");
        else if (n_stores == 5) asm volatile("s_waitcnt vmcnt(5)" ::: "memory");
        else asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        uint32_t w[kStreamMapPlanes];
        float2 g2[3];
#pragma unroll
        for (int q = 0; q < kStreamMapPlanes; ++q) {
            w[q] = 0u;
            const bool used = q < 3 || (q < 6 && has_normal) || q == 6 || q == 7 || (q > 7 && WF == PBR_WORKFLOW_SPECULAR);
            if (used) asm volatile("ds_read_b32 %0, %1 offset:%2" : "=v"(w[q]) : "v"(at4), "i"(q * 256) : "memory");
        }
#pragma unroll
        for (int c = 0; c < 3; ++c) asm volatile("ds_read_b64 %0, %1 offset:%2" : "=v"(g2[c]) : "v"(at8), "i"(c * 512) : "memory");
        // the values are in registers: the buffer may be overwritten (every later use of them depends on this wait)
        asm volatile("s_waitcnt lgkmcnt(0)"
                     : "+v"(w[0]), "+v"(w[1]), "+v"(w[2]), "+v"(w[3]), "+v"(w[4]), "+v"(w[5]), "+v"(w[6]), "+v"(w[7]), "+v"(w[8]), "+v"(w[9]),
                       "+v"(g2[0]), "+v"(g2[1]), "+v"(g2[2]) :: "memory");
        Texels<2> tx;
        float go[3][2];
        auto halves = [&](int plane, float v[2]) {
            const f16x2 h = __builtin_bit_cast(f16x2, w[plane]);
            v[0] = (float)h.x; v[1] = (float)h.y;
        };
#pragma unroll
        for (int c = 0; c < 3; ++c) halves(c, tx.al[c]);
        if (has_normal) {
#pragma unroll
            for (int c = 0; c < 3; ++c) halves(3 + c, tx.nm[c]);
        }
        halves(6, tx.ro);
        if (WF != PBR_WORKFLOW_SPECULAR) {
            halves(7, tx.me);
        } else {
#pragma unroll
            for (int c = 0; c < 3; ++c) halves(7 + c, tx.sp[c]);
        }
#pragma unroll
        for (int c = 0; c < 3; ++c) { go[c][0] = g2[c].x; go[c][1] = g2[c].y; }
        if (t + step < t1) issue(t + step);
        const int ty = (int)a.div_tx.div((uint32_t)t);          // row of the material; tiles_x = W / 128 tiles per row
        LanePos p;
        p.b = p.b0 = mat; p.y = ty; p.x = (t - ty * a.tiles_x) * 128 + 2 * lane;
        p.pix = p.src = (int64_t)t * 128 + 2 * lane;
        p.valid = true; p.sb = true; p.dup = 0;
        if constexpr (Loss::on) {
#pragma unroll
            for (int c = 0; c < 3; ++c) { loss.tgt[c][0] = go[c][0]; loss.tgt[c][1] = go[c][1]; }
            backward_body_to<LIGHT, WF, 2, false, __half, false>(a, b, p, tx, go, nullptr, 0,
                [&](float (&ga)[3][2], float (&gn)[3][2], float (&gr)[2], float (&gm)[2], float (&gs)[3][2]) {
                    store_gradients<WF, 2, __half>(a, b, p, ga, gn, gr, gm, gs);
                }, loss);
        } else {
            backward_body<LIGHT, WF, 2, false, __half, false>(a, b, p, tx, go, nullptr, 0);
        }
    }
}

template <int LIGHT, int WF, bool FULL>
__global__ __launch_bounds__(64) __attribute__((amdgpu_waves_per_eu(PBR_BWD_STREAM_WAVES)))
void cook_torrance_backward_stream_kernel(const KArgs a, const BArgs b, const int tiles_per_material, const int n_stores) {
    __shared__ uint32_t buf[kStreamLdsWords];
    NoLoss none;
    backward_stream_body<LIGHT, WF, FULL>(a, b, tiles_per_material, n_stores, buf, none);
}

// (A form of this kernel with 16-byte memory instructions -- 4 + 2 vector-memory instructions per tile instead of 14 + 8 -- was built in round 3
// and measured level, 143.5 against 142.9 us: the kernel is not limited by how its requests are shaped.  Removed in round 5; profiles/EXPERIMENTS.md.)

}  // namespace pbr
