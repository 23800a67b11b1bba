"""The capture and fit kernels at their 32-bit addressing limits: what tests/test_gpu_addressing_limits.py does for the render, blend, fold,
map-op, resize and unpack kernels, for the families merged since.  Every one of those files says its offsets are 64-bit and mixes int32
pixel coordinates, uint32 quad indices, int loop counters and int64 strides in one expression; their own tests run 24 x 36, 23 x 35, 5 x 9.

Route A -- large strides, small planes.  One arena of 3 x 2^30 float32 elements (12 GiB), seen as fp16 or uint8 where a kernel needs that,
every byte 0xA5 before a test places anything (fp32 -2.9e-16, fp16 -0.022, uint8 165).  A test places the 24 x 36 planes of the quad
paths -- strides that are multiples of 4, pointers on 16 bytes -- or the 23 x 35 planes with an ODD large stride for the element paths, so
that batch strides ("batch") or plane strides ("plane") pass 2^31 elements or 2^32 bytes, and calls the C ABI through ctypes with exactly
those strides.  Asserted per case: (1) every result bit-equal to the same call on dense clones (which the family's own test file holds to
its oracle); (2) inputs unchanged and, after the placed regions are refilled, EVERY byte of the arena 0xA5 again -- nothing outside
what the call must write was written; (3) non-vacuity: for every element whose offset passes a boundary, the place a narrowed offset
would reach -- base + (offset mod 2^32) in elements and base + (offset x size mod 2^32) in bytes -- lies inside the arena and holds
other data than the true place (_distinct), so a wrapped read gives another result and a wrapped store fails (1) and (2) instead of
faulting.  A SIGN-extended 32-bit element offset (2^31 <= offset < 2^32) is negative and cannot be kept inside any arena in front of
which nothing is allocated: fp32 tensors (whose offsets stay below 3 x 2^30 elements) have that hole, fp16 and uint8 tensors are placed at
offsets of 2^32 elements and more, where the signed and the unsigned narrowing agree.
  big strides     fp32 batch 2^31 + 2^22 el (2^33 + 2^24 B) | plane 2^30 + 2^22 el: plane 1 passes 2^32 B, plane 2 passes 2^31 el
                  fp16 batch 2^32 + 2^26 el (2^33 + 2^27 B) | plane 2^31 + 2^26 el: plane 1 passes 2^31 el and 2^32 B, plane 2 passes 2^32 el
                  uint8 image 2^32 + 2^27 B, row 2^28 + 64 B (rows 16 ... 23 pass 2^32 B)

Audit: kernel -> its index arithmetic (read in the source, host launcher included; no overflow found) -> the test that crosses it.
  geometry.hip   remap_planes_kernel            sp = src + (i64)b s_bs + (i64)ry ws; lo + p s_ps; dp + p d_ps (p int, strides i64)   test_remap_planes_*
                 remap_planes_backward_kernel   gp + p g_ps + iy wo (iy i64); ip + p i_ps                                          test_remap_planes_*
  rotation.hip   rotate_planes_kernel           sp[p s_ps + off[k]] (off int, < 2^31: rotate_arguments); dp + p d_ps                 test_rotate_planes_large_strides
                 rotate_planes_backward_kernel  gp + p g_ps; n[(p + 1) s_ps] (src read for the normal triple); base[n] int in-plane   test_rotate_planes_large_strides
  packing.hip    plane_ops_kernel / _backward   src + b stride (b = blockIdx.z as i64); dst + plane stride                          test_plane_ops_large_strides
                 (its overlap test takes first-to-last ranges, so a written tensor with a large stride may not span a read one:
                 the side that does not cross sits above the crossing side's last plane, from 11 GiB on)
  pack_image.hip pack_images_kernel             dense: src + (i64)c stride_c + 4 q; general: y stride_h + x stride_w + c stride_c    test_pack_images_large_strides
  normal_ops.hip normal_from_height(_backward)  h + b h_bs (b i64); 2 n_ps + o; (i64)y W + (i64)u V                                  test_normal_ops_large_strides
                 normal_transform(_backward)    so = b s_bs + p (i64); so + 2 s_ps                                                   test_normal_ops_large_strides, test_normal_transform_through_the_python_wrapper
                 (the other raw wrappers that forward strides: test_rows_dense_callers_forward_the_strides_of_arena_views)
  height_ops.hip normal_divergence(_backward)   i = (i64)y W + x; b n_bs; 2 n_ps                                                     test_height_ops_large_strides
                 height_stats / normalize / grad_sums / normalize_backward   h + b h_bs, i64 loops over n <= 2^31 - 1              test_height_ops_large_strides
                 poisson_scale_kernel           not in the issue's families (a dense complex spectrum, batch stride H (W/2 + 1))     left out
  rectify.hip    rectify_kernel                 img = src + l image_stride (l i64); (i64)yc stride_h + (i64)xc stride_w;
                                                targets + l 3 plane + at                                                           test_rectify_source_strides, test_capture_of_sixteen_shots
  photometric.hip photometric_kernel            targets + (i64)l 3 plane + at; t + c plane; weights + (i64)l stride + at             test_capture_of_sixteen_shots
  smoothness.hip smoothness_step_kernel         p + (i64)b bs; c ps + at; at = (i64)row W + x0; g: c gs + (i64)r W + x0              test_smoothness_large_strides, test_smoothness_through_priors_step, test_smoothness_in_plane
                 (priors._entry passes H W as the weights' batch stride -- its weights are contiguous by contract -- so the weights'
                 stride is crossed through the C ABI only)
  ct_stack.hip, ct_stack_weighted.hip   cook_torrance_stack and the orthographic loss step, plain and weighted:
                                                targets + (int64_t)l * 3 * plane + at, weights + l light_stride + at                test_light_stack_past_2_to_31_elements[orthographic]
  adam.hip       adam_step_kernel               p0 = (i64)b bs + (i64)c ps; s0 = q pixels (q i64); (i64)b 3 pixels (unit)           test_adam_large_strides, test_adam_through_material_adam, test_adam_dense_state
  ct_camera_stack.hip, ct_view_stack.hip and their weighted siblings: the same offsets, and cameras[l] per shot                       test_light_stack_past_2_to_31_elements[camera | per-shot-camera]
  ct_camera.hip  the camera forward and its MSE step  b * the maps', the result's and the target's batch strides                  test_camera_batch_past_2_to_31_elements
  rotation.hip, height_ops.hip at the largest accepted plane: in-plane offsets up to 2^31 - 1                                          test_rotation_at_its_largest_plane, test_height_ops_at_their_largest_plane
NOT COVERED here -- these offsets have not run past 2^31:
  the fit steps (pbr_cook_torrance_*_mse_stack_fit_step, six entry points): they add the gradients of lights, intensities and cameras to
                 the steps' passes over the same addresses.  To cover them: the calls of test_light_stack_past_2_to_31_elements with
                 `light` requiring grad, and float64 autograd of the parameters over the WHOLE stack (the parameter gradients are sums
                 over every pixel, so no window of rows gives their reference).
  pbr_adam_step fp16 with its master past 2^31 elements: the fp32 entry of test_adam_dense_state covers the state offset q pixels; fp16 with
                 its master crosses on Route A only.  To cover it: that test with a 2^28-element fp16 parameter and a float32 master.
  poisson_scale_kernel: a dense complex spectrum, not among the families of this file.

Route B -- one contiguous tensor past 2^31 elements, for the offsets a kernel forms itself.  Data made on the device by a seeded
generator; the first and the far window against the family's float64 oracle at the family's own band, and _distinct against the window a
wrapped offset would reach.

Small shapes: photometric stereo under 3, 4 and 16 lights and under 1 ... 4 passes on the shadowed set, against the oracle at the bands
tests/test_addressing_limits_host.py derives (its EXPECTED / ITERATIONS tables).

Every test prints its figures before it asserts: worst error / band where there is one, peak GiB (the fixture), wall time.

MEASURED on the MI355X (peak device memory includes the 12 GiB arena, which lives as long as the module; the whole file runs in 35 s):
  test                                      the offset that crosses                                     peak GiB   time     figures
  every Route A case (89 cases)             the table above; 3456 ... 10368 elements past a boundary     12.3       <= 0.5 s  bit-equal to the dense call
    (the time is the two launches, two passes over the arena -- fill and compare, 12 GiB each, about 5 ms -- and the host-side check)
  test_photometric_stereo_* (22 cases)      none: L = 3, 4, 16 and K = 1 ... 4 at 24 x 36 | 24 x 35       12.0       0.2 s    worst 1.6e-6 / band 1e-5 (shadowed K = 4), 8.9e-7 / 1e-5 (L = 16)
  test_smoothness_in_plane fp16 5 x 2^29    row W + x = 2^31 at row 4                                    22.0       0.3 s    0.50 fp16 ulp / 1
  test_smoothness_in_plane fp32 3 x 2^30    row W + x = 2^31 at row 2 (2^32 bytes at row 1)              36.0       1.0 s    gradient / k 4.2e-7 / band 2e-6
  test_adam_dense_state                     q pixels = 8 x 2^28 = 2^31; b bs + c ps the same             40.0       1.0 s    every bit of p, m, v the float32 oracle's
  test_capture_of_sixteen_shots             l 3 plane = 45 x 6912^2 = 2.15e9 (targets: 2.29e9 floats)    34.8       1.3 s    rectify 5.6e-8 / band 2e-6; stereo 6.8e-7 / band 1e-5
  test_light_stack_past_2_to_31_elements    the same offset in the stack, the targets and the weights    36.6       3.2 s    forward 2.6e-7 / 2e-6; loss 8e-9 of 0.23; gradients <= 1.3e-9 / 7.7e-9
    (three families; 3.2 s each: two loss steps, and 6 float64 autograd passes over 4 x 6912 pixels under 16 lights on the host)
  test_camera_batch_past_2_to_31_elements   b x batch stride: material 11 starts 2.2e9 elements in       51.0       0.3 s    forward 1.4e-7 / 2e-6; loss 7e-9 of 0.20; gradients <= 2.0e-10 / 5.6e-9
  test_rotation_at_its_largest_plane        source offset 2 114 125 715, its own 2 145 915 720           20.0       0.4 s    bit-equal to the gather through the index function
  test_height_ops_at_their_largest_plane    i = y W + x up to 2^31 - 88 048; argmin 2 147 395 597        76.0       2.3 s    divergence bit-equal; backward 0.006 of its bound;
                                                                                                                              normalisation 6.5e-8 / 2e-6, its backward 0.001 of its bound
    (2.3 s: five float64 reductions over the 2.1e9-pixel plane on the device)
"""
import ctypes
import os
import sys
import time

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
import adam_oracle as AO  # noqa: E402
import photometric_cases as PC  # noqa: E402
import photometric_oracle as PO  # noqa: E402
import smoothness_oracle as SO  # noqa: E402

from pypbr_amd import _native as N  # noqa: E402
from pypbr_amd import capture, priors  # noqa: E402
from test_gpu_addressing_limits import GiB, _distinct, _need, _release_device_memory  # noqa: E402,F401  (the fixture is autouse here too)
from test_gpu_write_guards import Guards  # noqa: E402

pytestmark = pytest.mark.gpu

SENT = 0xA5
ARENA_FLOATS = 3 << 30
ARENA_BYTES = 4 * ARENA_FLOATS
TWO31, TWO32 = 1 << 31, 1 << 32
INT_OF = {torch.float32: torch.int32, torch.float16: torch.int16, torch.uint8: torch.uint8, torch.int16: torch.int16}
SENT_INT = {torch.int32: 0xA5A5A5A5 - (1 << 32), torch.int16: 0xA5A5 - (1 << 16), torch.uint8: SENT}
CODE = {torch.float32: N.F32, torch.float16: N.F16}
SLOT = 1 << 20                      # bytes between the bases of two placed tensors
HIGH = 11 * GiB                     # where tensors sit that must lie ABOVE every crossing tensor's last plane
QUAD, ELEMENT = (24, 36), (23, 35)


def bits(t):
    return t.contiguous().view(INT_OF[t.dtype])


def big_stride(dtype, which, odd):
    """The stride (elements) that crosses: see the docstring's table."""
    if dtype == torch.float32:
        s = TWO31 + (1 << 22) if which == "batch" else (1 << 30) + (1 << 22)
    elif dtype == torch.float16:
        s = TWO32 + (1 << 26) if which == "batch" else TWO31 + (1 << 26)
    else:
        s = TWO32 + (1 << 27)
    return s + (1 if odd else 0)


class Arena:
    """The 12 GiB of Route A: places strided views, then checks that a call wrote its regions and nothing else."""

    def __init__(self):
        self.f32 = torch.empty(ARENA_FLOATS, dtype=torch.float32, device="cuda")
        assert self.f32.data_ptr() % 256 == 0
        self.regions, self.slots, self.high_slots = [], 0, 0

    def reset(self):
        self.f32.view(torch.uint8).fill_(SENT)
        self.regions, self.slots, self.high_slots = [], 0, 0
        return self

    def typed(self, dtype):
        return self.f32.view(dtype)

    def next_base(self, high=False):
        """Byte offset of the next tensor's first element: 1 MiB apart, from 1 MiB (or from HIGH) on."""
        if high:
            self.high_slots += 1
            return HIGH + self.high_slots * SLOT
        self.slots += 1
        return self.slots * SLOT

    def place(self, shape, dtype, strides, base, data=None, written=False, misalign=0):
        esz = torch.empty(0, dtype=dtype).element_size()
        start = base // esz + misalign
        view = self.typed(dtype).as_strided(tuple(shape), tuple(strides), start)
        offsets = sum(np.arange(n, dtype=np.int64).reshape((-1,) + (1,) * (len(shape) - 1 - d)) * s for d, (n, s) in enumerate(zip(shape, strides)))
        offsets = np.broadcast_to(offsets, shape).reshape(-1)                              # element offsets from the pointer the kernel gets
        assert offsets.min() == 0 and (start + int(offsets.max()) + 1) * esz <= ARENA_BYTES, "the placement leaves the arena"
        if data is not None:
            view.copy_(data)
        self.regions.append(dict(view=view, data=None if data is None else data.clone(), written=written, start=start, esz=esz, offsets=offsets, dtype=dtype))
        return view

    def disjoint(self):
        """No two placed elements share a byte."""
        at = np.concatenate([(r["start"] + r["offsets"]) * r["esz"] for r in self.regions])
        size = np.concatenate([np.full(r["offsets"].size, r["esz"], dtype=np.int64) for r in self.regions])
        order = np.argsort(at, kind="stable")
        at, size = at[order], size[order]
        assert (at[1:] >= at[:-1] + size[:-1]).all(), "two placed tensors overlap"

    def crossings(self, what):
        """Non-vacuity, before the call: per region the elements whose offset passes 2^31 elements or 2^32 bytes; where a narrowed offset
        would reach lies inside the arena and holds other data.  Returns (elements past a boundary, of them: a signed 32-bit element offset
        would leave the arena)."""
        self.disjoint()
        total = outside_signed = 0
        for r in self.regions:
            o, esz, start = r["offsets"], r["esz"], r["start"]
            cross = (o >= TWO31) | (o * esz >= TWO32)
            if not cross.any():
                continue
            total += int(cross.sum())
            oc = o[cross]
            by_elements = (start + oc % TWO32) * esz                                       # the element offset narrowed to 32 bits, unsigned
            by_bytes = start * esz + (oc * esz) % TWO32                                    # the byte offset narrowed to 32 bits
            signed = np.where(oc % TWO32 >= TWO31, oc % TWO32 - TWO32, oc % TWO32)
            outside_signed += int(((start + signed) < 0).sum())
            for wrapped in (by_elements, by_bytes):
                assert (wrapped >= 0).all() and (wrapped + esz <= ARENA_BYTES).all(), (what, "a narrowed offset would leave the arena")
            typed = self.typed(r["dtype"])
            true = typed[torch.from_numpy(start + oc).cuda()].double().cpu().numpy()
            moved = by_bytes != (start + oc) * esz
            assert moved.any(), what
            if r["data"] is not None:                                                      # (a result's true place and wrapped place both hold the sentinel now)
                there = typed[torch.from_numpy(by_bytes[moved] // esz).cuda()].double().cpu().numpy()
                _distinct(true[moved], there, 0.0, (what, "bytes"))
                narrowed = by_elements != (start + oc) * esz
                if narrowed.any():
                    there = typed[torch.from_numpy(by_elements[narrowed] // esz).cuda()].double().cpu().numpy()
                    _distinct(true[narrowed], there, 0.0, (what, "elements"))
        assert total > 0, (what, "no offset of this case passes a boundary")
        return total, outside_signed

    def finish(self, what):
        """After the call: inputs unchanged; the results (dense clones, in placement order); then every region refilled and the whole arena
        compared with the sentinel."""
        torch.cuda.synchronize()
        results = []
        for r in self.regions:
            got = r["view"].clone()
            if r["data"] is not None and not r["written"]:
                assert torch.equal(bits(got), bits(r["data"])), (what, "an input was written")
            results.append(got)
            r["view"].view(INT_OF[r["dtype"]]).fill_(SENT_INT[INT_OF[r["dtype"]]])
        words = self.f32.view(torch.int32)
        for i in range(0, ARENA_FLOATS, 1 << 28):
            assert bool((words[i:i + (1 << 28)] == SENT_INT[torch.int32]).all()), (what, "written outside the call's regions, float32 elements from", i)
        return results


@pytest.fixture(scope="module")
def arena():
    _need(14)
    a = Arena()
    yield a
    del a.f32


class Placer:
    """What a family's run() places its tensors through: `inp` for what the call reads (or updates in place: written=True), `out` for what
    it writes.  mode: None = dense clones outside the arena; "batch" / "plane" = in the arena with that stride past the boundary."""

    def __init__(self, arena=None, mode=None, odd=False, what=""):
        self.arena, self.mode, self.odd, self.what, self.outs, self.cross, self.kept = arena, mode, odd, what, [], None, []

    def strides(self, shape, dtype, big):
        """[B,C,H,W]: (batch, plane, W, 1); [B,H,W]: (batch, W, 1).  Compact strides 16384 and 1024; `big` puts the crossing stride on the
        batch or on the planes -- on the batch where the tensor has one plane."""
        h, w = shape[-2:]
        if big == "dense":
            return tuple(int(np.prod(shape[d + 1:])) for d in range(len(shape)))
        if len(shape) == 3:
            return (16384 if big is None else big_stride(dtype, "batch", self.odd), w, 1)
        if big is None:
            return (16384, 1024, w, 1)
        if big == "batch" or shape[1] == 1:
            return (big_stride(dtype, "batch", self.odd), 1024, w, 1)
        return (16384, big_stride(dtype, "plane", self.odd), w, 1)

    def ready(self):
        """Between placing and launching: the non-vacuity check of the placements."""
        if self.arena is not None:
            self.cross = self.arena.crossings(self.what)

    def _put(self, shape, dtype, data, big, written, high):
        if self.arena is None and isinstance(big, tuple):                                  # explicit strides: the dense call sees a contiguous clone
            big = None
        if self.arena is None:
            t = torch.empty(tuple(shape), dtype=dtype, device="cuda")
            t.view(INT_OF[dtype]).fill_(SENT_INT[INT_OF[dtype]])
            if data is not None:
                t.copy_(data)
            return t
        big = self.mode if big == "mode" else big
        strides = big if isinstance(big, tuple) else self.strides(shape, dtype, big)
        return self.arena.place(shape, dtype, strides, self.arena.next_base(high), data, written)

    def inp(self, data, big="mode", written=False, high=False):
        t = self._put(data.shape, data.dtype, data, big, written, high)
        self.kept.append(t)                                                                # (a dense clone dropped before the launch would hand its memory to the next one)
        if written:
            self.outs.append(t)
        return t

    def out(self, shape, dtype=torch.float32, big="mode", high=False):
        t = self._put(shape, dtype, None, big, True, high)
        self.outs.append(t)
        return t


def sp(t):
    """(pointer, batch stride, plane stride) of a [B,C,H,W] tensor; (pointer, batch stride) of a [B,H,W] one."""
    return (t.data_ptr(),) + tuple(t.stride()[:-2])


def stream():
    return torch.cuda.current_stream().cuda_stream


def route_a(arena, run, what, mode, odd):
    """run(placer) places its tensors, calls placer.ready(), launches, and returns dense results it keeps outside the arena (or None).
    Once on dense clones, once in the arena: every result bit for bit, the arena otherwise untouched."""
    _need(1)                                                                               # (beside the arena, which the fixture asked for)
    t0 = time.perf_counter()
    dense = Placer()
    extra_d = run(dense) or []
    torch.cuda.synchronize()
    want = [t.clone() for t in dense.outs]
    arena.reset()
    placed = Placer(arena, mode, odd, what)
    extra_a = run(placed) or []
    assert placed.cross is not None, "run() calls p.ready() between placing and launching"
    got_all = arena.finish(what)
    got = [g for g, r in zip(got_all, arena.regions) if r["written"]]
    assert len(got) == len(want) and len(extra_a) == len(extra_d)
    same = all(torch.equal(bits(a), bits(b)) for a, b in zip(got, want)) and all(torch.equal(bits(a), bits(b)) for a, b in zip(extra_a, extra_d))
    untouched = [bool((bits(b) == SENT_INT[INT_OF[b.dtype]]).all()) for b in want]
    n, outside = placed.cross
    print("\n%s: %d elements past 2^31 elements / 2^32 bytes (%d of them where a sign-extended 32-bit offset leaves the arena); %d results bit-equal to the dense call: %s; %.2f s"
          % (what, n, outside, len(want) + len(extra_d), same, time.perf_counter() - t0))
    assert not any(untouched), (what, "a result of the dense call was never written: the comparison would be vacuous")
    assert same, what


def rand(shape, dtype, seed, lo=0.0, hi=1.0):
    g = torch.Generator(device="cuda").manual_seed(seed)
    return (torch.rand(shape, device="cuda", generator=g) * (hi - lo) + lo).to(dtype)


def unit_normals(shape, dtype, seed):
    n = rand(shape, torch.float32, seed, -0.5, 0.5)
    n[..., 2, :, :] += 1.0
    return (n / n.norm(dim=-3, keepdim=True)).to(dtype)


CASES = [("batch", QUAD, False), ("plane", QUAD, False), ("batch", ELEMENT, True), ("plane", ELEMENT, True)]
CASE_IDS = ["batch-quad", "plane-quad", "batch-odd", "plane-odd"]
DTYPES = [torch.float32, torch.float16]
DTYPE_IDS = ["fp32", "fp16"]


# ---------------------------------------------------------------- Route A: geometry.hip
@pytest.mark.parametrize("dtype", DTYPES, ids=DTYPE_IDS)
@pytest.mark.parametrize("mode,size,odd", CASES, ids=CASE_IDS)
def test_remap_planes_large_strides(arena, mode, size, odd, dtype):
    """Crop + both flips + roll of [2,3,h,w] to (h - 4, w - 4): columns from x_offset downwards wrap, so quads take the span path and, at the
    wrap and the ragged end, the pixel-by-pixel path.  The backward (fp32) gathers into a source-sized gradient."""
    h, w = size
    ho, wo = h - 4, w - 4
    geo = (2, 3, h, w, ho, wo, 5, -1, 7, -1, 0b010)
    lib = N.lib()

    def forward(p):
        src = p.inp(rand((2, 3, h, w), dtype, 11))
        dst = p.out((2, 3, ho, wo), dtype)
        p.ready()
        N.check(lib.pbr_remap_planes(*sp(src), *sp(dst), *geo, CODE[dtype], stream()))
    route_a(arena, forward, "remap_planes %s %s" % (mode, dtype), mode, odd)
    if dtype == torch.float32:
        def backward(p):
            go = p.inp(rand((2, 3, ho, wo), torch.float32, 12, -0.4, 0.6))
            gi = p.out((2, 3, h, w))
            p.ready()
            N.check(lib.pbr_remap_planes_backward(*sp(go), *sp(gi), *geo, stream()))
        route_a(arena, backward, "remap_planes_backward %s" % mode, mode, odd)


# ---------------------------------------------------------------- Route A: rotation.hip
@pytest.mark.parametrize("dtype", DTYPES, ids=DTYPE_IDS)
@pytest.mark.parametrize("mode,size,odd", CASES, ids=CASE_IDS)
def test_rotate_planes_large_strides(arena, mode, size, odd, dtype):
    """rotate by 30 degrees (constant padding), three planes of which planes 0 ... 2 are the normal triple (normal_first_plane = 0): the
    forward rotates their (x, y); the backward reads `src` through its own strides for F.normalize's adjoint."""
    from pypbr_amd._rotate_ops import _rotate_geom, rotate_plan
    h, w = size
    plan = rotate_plan(h, w, 30.0)
    geom = _rotate_geom(plan)
    lib = N.lib()
    tail = (2, 3, h, w, plan.H, plan.W, ctypes.byref(geom), 0) + tuple(plan.normal_matrix)

    def forward(p):
        src = p.inp(unit_normals((2, 3, h, w), dtype, 21))
        dst = p.out((2, 3, plan.H, plan.W), dtype)
        p.ready()
        N.check(lib.pbr_rotate_planes(*sp(src), *sp(dst), *tail, CODE[dtype], stream()))
    route_a(arena, forward, "rotate_planes %s %s" % (mode, dtype), mode, odd)
    if dtype == torch.float32:
        def backward(p):
            go = p.inp(rand((2, 3, plan.H, plan.W), torch.float32, 22, -0.4, 0.6))
            src = p.inp(unit_normals((2, 3, h, w), torch.float32, 21))
            gi = p.out((2, 3, h, w))
            p.ready()
            N.check(lib.pbr_rotate_planes_backward(*sp(go), *sp(gi), *sp(src), *tail, stream()))
        route_a(arena, backward, "rotate_planes_backward %s" % mode, mode, odd)


# ---------------------------------------------------------------- Route A: normal_ops.hip
@pytest.mark.parametrize("dtype", DTYPES, ids=DTYPE_IDS)
@pytest.mark.parametrize("mode,size,odd", CASES, ids=CASE_IDS)
def test_normal_ops_large_strides(arena, mode, size, odd, dtype):
    h, w = size
    lib = N.lib()
    m = (0.8, -0.6, 0.6, 0.8)

    def from_height(p):
        hm = p.inp(rand((2, 1, h, w), dtype, 31))
        out = p.out((2, 3, h, w), dtype)
        p.ready()
        N.check(lib.pbr_normal_from_height(hm.data_ptr(), hm.stride(0), *sp(out), 2, h, w, 1.5, 0, CODE[dtype], stream()))
    route_a(arena, from_height, "normal_from_height %s %s" % (mode, dtype), mode, odd)

    def transform(p):
        n = p.inp(unit_normals((2, 3, h, w), dtype, 32))
        out = p.out((2, 3, h, w), dtype)
        p.ready()
        N.check(lib.pbr_normal_transform(*sp(n), *sp(out), 2, h * w, *m, 1, CODE[dtype], stream()))
    route_a(arena, transform, "normal_transform %s %s" % (mode, dtype), mode, odd)
    if dtype != torch.float32:
        return

    def from_height_backward(p):
        hm = p.inp(rand((2, 1, h, w), torch.float32, 31))
        g = p.inp(rand((2, 3, h, w), torch.float32, 33, -0.4, 0.6))
        gh = p.out((2, 1, h, w))
        p.ready()
        N.check(lib.pbr_normal_from_height_backward(hm.data_ptr(), hm.stride(0), *sp(g), gh.data_ptr(), gh.stride(0), 2, h, w, 1.5, 0, stream()))
    route_a(arena, from_height_backward, "normal_from_height_backward %s" % mode, mode, odd)

    def transform_backward(p):
        n = p.inp(unit_normals((2, 3, h, w), torch.float32, 32))
        g = p.inp(rand((2, 3, h, w), torch.float32, 34, -0.4, 0.6))
        gi = p.out((2, 3, h, w))
        p.ready()
        N.check(lib.pbr_normal_transform_backward(*sp(n), *sp(g), *sp(gi), 2, h * w, *m, 1, stream()))
    route_a(arena, transform_backward, "normal_transform_backward %s" % mode, mode, odd)


def test_normal_transform_through_the_python_wrapper(arena):
    """_transform_raw forwards the strides of the views it is given (a _rows_dense caller): the same bits as on dense clones."""
    from pypbr_amd._normal_ops import _transform_raw
    h, w = QUAD

    def run(p):
        n = p.inp(unit_normals((2, 3, h, w), torch.float16, 35))
        out = p.out((2, 3, h, w), torch.float16)
        p.ready()
        _transform_raw(n, (0.8, -0.6, 0.6, 0.8), True, out=out)
    route_a(arena, run, "_transform_raw", "batch", False)


def test_rows_dense_callers_forward_the_strides_of_arena_views(arena):
    """The raw wrappers behind the public calls (the _rows_dense callers) take the batch and plane strides from the views they are given:
    _geometry._remap_raw, _rotate_ops._rotate_raw, _packing._unpack_raw and _pack_raw, _normal_ops._nfh_raw, _height_ops._divergence_raw,
    each on arena views whose strides cross, against the same call on dense clones.  They allocate their results themselves."""
    from pypbr_amd import _geometry, _height_ops, _normal_ops, _packing, _rotate_ops
    h, w = QUAD

    def remap(p):
        t = p.inp(rand((2, 3, h, w), torch.float16, 36))
        p.ready()
        return [_geometry._remap_raw(t, (5, -1), (7, -1), 0b010, h - 4, w - 4)]
    route_a(arena, remap, "_remap_raw", "plane", False)
    plan = _rotate_ops.rotate_plan(h, w, 30.0)

    def rotate(p):
        t = p.inp(unit_normals((2, 3, h, w), torch.float32, 37))
        p.ready()
        return [_rotate_ops._rotate_raw(t, plan, 0)]
    route_a(arena, rotate, "_rotate_raw", "batch", False)
    layout = _packing._unpack_layout([("albedo", 1), ("normal", 2)], 3)

    def unpack(p):
        x = p.inp(rand((2, 3, h, w), torch.float16, 38, 0.3, 0.7))
        p.ready()
        return [t.clone() for t in _packing._unpack_raw(x, layout, 1.0, 0.0, False)]
    route_a(arena, unpack, "_unpack_raw", "plane", False)

    def pack(p):
        xs = [p.inp(rand((2, 3, h, w), torch.float32, 39)), p.inp(rand((2, 1, h, w), torch.float32, 40))]
        p.ready()
        return [_packing._pack_raw(xs, [(3, 2, 2.0, -1.0), (1, 1, 1.0, 0.0)], False)]
    route_a(arena, pack, "_pack_raw", "batch", False)

    def from_height(p):
        hm = p.inp(rand((2, 1, h, w), torch.float16, 41))
        p.ready()
        return [_normal_ops._nfh_raw(hm, 1.5, False)]
    route_a(arena, from_height, "_nfh_raw", "batch", False)

    def divergence(p):
        n = p.inp(unit_normals((2, 3, h, w), torch.float32, 42))
        p.ready()
        return [_height_ops._divergence_raw(n, 1.5, False)]
    route_a(arena, divergence, "_divergence_raw", "plane", False)


# ---------------------------------------------------------------- Route A: height_ops.hip
@pytest.mark.parametrize("dtype", DTYPES, ids=DTYPE_IDS)
@pytest.mark.parametrize("mode,size,odd", CASES, ids=CASE_IDS)
def test_height_ops_large_strides(arena, mode, size, odd, dtype):
    """pbr_normal_divergence and its backward; pbr_height_stats + pbr_height_normalize and their backward (the heights and gradients fp32 by
    definition, the normalised result in `dtype`).  The workspaces and the statistics are dense and lie outside the arena."""
    h, w = size
    lib = N.lib()

    def divergence(p):
        n = p.inp(unit_normals((2, 3, h, w), dtype, 41))
        div = p.out((2, h, w))
        p.ready()
        N.check(lib.pbr_normal_divergence(*sp(n), div.data_ptr(), div.stride(0), 2, h, w, 1.5, 0, CODE[dtype], stream()))
    route_a(arena, divergence, "normal_divergence %s %s" % (mode, dtype), mode, odd)
    nbytes = lib.pbr_height_workspace_bytes(2, h, w)
    assert nbytes > 0

    def normalize(p):
        hm = p.inp(rand((2, h, w), torch.float32, 42, -3.0, 5.0))
        out = p.out((2, 1, h, w), dtype)
        ws = torch.zeros(nbytes // 8, dtype=torch.float64, device="cuda")
        stats = torch.zeros(2, 5, device="cuda")
        p.ready()
        N.check(lib.pbr_height_stats(hm.data_ptr(), hm.stride(0), ws.data_ptr(), 2, h, w, stream()))
        N.check(lib.pbr_height_normalize(hm.data_ptr(), hm.stride(0), ws.data_ptr(), out.data_ptr(), out.stride(0), stats.data_ptr(), 2, h, w, CODE[dtype], stream()))
        return [stats]
    route_a(arena, normalize, "height_stats + height_normalize %s %s" % (mode, dtype), mode, odd)
    if dtype != torch.float32:
        return

    def divergence_backward(p):
        n = p.inp(unit_normals((2, 3, h, w), torch.float32, 41))
        dd = p.inp(rand((2, h, w), torch.float32, 43, -0.4, 0.6))
        gn = p.out((2, 3, h, w))
        p.ready()
        N.check(lib.pbr_normal_divergence_backward(*sp(n), dd.data_ptr(), dd.stride(0), *sp(gn), 2, h, w, 1.5, 0, stream()))
    route_a(arena, divergence_backward, "normal_divergence_backward %s" % mode, mode, odd)
    from pypbr_amd._height_ops import _normalize_raw
    dense_out, stats = _normalize_raw(rand((2, h, w), torch.float32, 42, -3.0, 5.0), torch.float32)

    def normalize_backward(p):
        g = p.inp(rand((2, 1, h, w), torch.float32, 44, -0.4, 0.6))
        out = p.inp(dense_out)
        dh = p.out((2, h, w))
        ws = torch.zeros(nbytes // 8, dtype=torch.float64, device="cuda")
        p.ready()
        N.check(lib.pbr_height_normalize_backward(g.data_ptr(), g.stride(0), out.data_ptr(), out.stride(0), stats.data_ptr(), ws.data_ptr(), dh.data_ptr(),
                                                  dh.stride(0), 2, h, w, stream()))
    route_a(arena, normalize_backward, "height_normalize_backward %s" % mode, mode, odd)


# ---------------------------------------------------------------- Route A: smoothness.hip
def smooth_entry(t, g, w, k, kind, wrap):
    """pbr_smooth_tensor from the strides of the views (priors._entry takes contiguous weights: it passes H W as their batch stride)."""
    return N.SmoothTensor(t.data_ptr(), None if g is None else g.data_ptr(), None if w is None else w.data_ptr(), t.stride(0), t.stride(1),
                          0 if g is None else g.stride(0), 0 if g is None else g.stride(1), 0 if w is None else w.stride(0), k, 1e-3, CODE[t.dtype],
                          t.shape[0], t.shape[1], t.shape[2], t.shape[3], priors.KINDS[kind], int(wrap))


@pytest.mark.parametrize("dtype", DTYPES, ids=DTYPE_IDS)
@pytest.mark.parametrize("kind", ["l2", "charbonnier"])
@pytest.mark.parametrize("mode,size,odd", CASES, ids=CASE_IDS)
def test_smoothness_large_strides(arena, mode, size, odd, kind, dtype):
    """Two entries in one launch, wrap on: entry 0 crosses on the parameter's side (and its per-image weights on their batch stride), entry 1
    on the gradient's side.  Loss, terms and both gradients bit-equal to the dense launch."""
    from test_gpu_smoothness import make_map, make_weights
    h, w = size
    rng = np.random.default_rng(50 + h)
    half = dtype == torch.float16
    maps = [torch.from_numpy(make_map(rng, (2, 3, h, w), half)).to(dtype).cuda() for _ in range(2)]
    weights = torch.from_numpy(make_weights(rng, (2, 3, h, w), "image")).float().cuda()
    lib = N.lib()

    def run(p):
        p0 = p.inp(maps[0])
        g0 = p.out((2, 3, h, w), dtype, big=None)
        w0 = p.inp(weights, big="batch")
        p1 = p.inp(maps[1], big=None)
        g1 = p.out((2, 3, h, w), dtype)
        p.ready()
        table = (N.SmoothTensor * 2)(smooth_entry(p0, g0, w0, 0.7 / (2 * h * w), kind, True), smooth_entry(p1, g1, None, 0.3 / (2 * h * w), kind, True))
        assert table[0].weights_batch_stride == w0.stride(0) and table[0].param_batch_stride == p0.stride(0) and table[1].grad_plane_stride == g1.stride(1)
        nbytes = lib.pbr_smoothness_workspace_bytes(table, 2)
        assert nbytes > 0, lib.pbr_smoothness_check(table, 2)
        ws = torch.zeros(nbytes // 4, device="cuda")
        loss, terms = torch.zeros((), device="cuda"), torch.zeros(2, device="cuda")
        N.check(lib.pbr_smoothness_step(table, 2, loss.data_ptr(), terms.data_ptr(), ws.data_ptr(), nbytes, stream()))
        return [loss, terms]
    route_a(arena, run, "smoothness_step %s %s %s" % (mode, kind, dtype), mode, odd)


def test_smoothness_through_priors_step(arena):
    """priors._step builds its table with priors._entry from the strides of the views it is given."""
    from test_gpu_smoothness import make_map
    h, w = QUAD
    x = torch.from_numpy(make_map(np.random.default_rng(59), (2, 3, h, w), False)).float().cuda()

    def run(p):
        t = p.inp(x)
        g = p.out((2, 3, h, w))
        p.ready()
        loss, terms = priors._step([t], [g], [None], [0.7 / (2 * h * w)], priors.KINDS["charbonnier"], 1e-3, False)
        return [loss, terms]
    route_a(arena, run, "priors._step", "plane", False)


# ---------------------------------------------------------------- Route A: adam.hip
ADAM_ENTRIES = [("box", 3), ("unit", 3), ("none", 1)]


def adam_states(size, half, seed, batch=2):
    from test_gpu_adam import one_step_state
    return [one_step_state(kind, (batch, c) + size, half, seed + i) for i, (kind, c) in enumerate(ADAM_ENTRIES)]


@pytest.mark.parametrize("dtype", DTYPES, ids=DTYPE_IDS)
@pytest.mark.parametrize("mode,size,odd", CASES, ids=CASE_IDS)
def test_adam_large_strides(arena, mode, size, odd, dtype):
    """A box, a unit and an unprojected entry in one launch; parameters (updated in place) and gradients on crossing strides, the dense
    state -- exp_avg, exp_avg_sq, the fp16 entries' master -- in the arena as well.  Everything written bit-equal to the dense launch.
    pbr_adam_check wants a parameter's batch stride to clear the whole image before it, (C - 1) plane_stride + pixels, and a second image behind
    planes 2^30 elements apart would leave the arena: the plane-stride cases hold one image."""
    from pypbr_amd.optim import _coefficients
    half = dtype == torch.float16
    batch = 1 if mode == "plane" else 2
    states = adam_states(size, half, 60, batch)
    lib = N.lib()
    project = {"box": N.ADAM_BOX, "unit": N.ADAM_UNIT, "none": N.ADAM_NONE}

    def run(p):
        rows = []
        for (kind, c), (p0, g0, m0, v0, _) in zip(ADAM_ENTRIES, states):
            to = lambda a, dt: torch.from_numpy(a).to(dt).cuda()                          # noqa: E731
            param = p.inp(to(p0, dtype), written=True)
            grad = p.inp(to(g0, dtype))
            m, v = p.inp(to(m0, torch.float32), big="dense", written=True), p.inp(to(v0, torch.float32), big="dense", written=True)
            master = p.inp(to(p0, torch.float32), big="dense", written=True) if half else None
            rows.append(N.AdamTensor(param.data_ptr(), grad.data_ptr(), m.data_ptr(), v.data_ptr(), None if master is None else master.data_ptr(),
                                     size[0] * size[1], param.stride(0), param.stride(1), grad.stride(0), grad.stride(1), batch, c, CODE[dtype], project[kind],
                                     0.05, 1.0, 0.1, 0))
        p.ready()
        table = (N.AdamTensor * len(rows))(*rows)
        coeffs = (N.AdamCoeffs * 1)(_coefficients(1e-2, (0.9, 0.999), 1e-8, 2.0))
        N.check(lib.pbr_adam_step(table, len(rows), coeffs, None, 1, stream()))
    route_a(arena, run, "adam_step %s %s" % (mode, dtype), mode, odd)


def test_adam_through_material_adam(arena):
    """MaterialAdam.step reads the strides of the parameter and of its gradient through optim._planes."""
    from pypbr_amd.optim import MaterialAdam
    p0, g0, m0, v0, _ = adam_states(QUAD, False, 70)[0]

    def run(p):
        to = lambda a: torch.from_numpy(a).float().cuda()                                  # noqa: E731
        param, grad = p.inp(to(p0), written=True), p.inp(to(g0))
        m, v = p.inp(to(m0), big="dense", written=True), p.inp(to(v0), big="dense", written=True)
        p.ready()
        param.requires_grad_(True)
        param.grad = grad
        opt = MaterialAdam([dict(params=[param], bounds=(0.05, 1.0))], lr=1e-2)
        opt.state[param] = {"step": torch.tensor(1.0), "exp_avg": m, "exp_avg_sq": v}
        opt.step()
        param.grad = None
        param.requires_grad_(False)
    route_a(arena, run, "MaterialAdam.step", "batch", False)


# ---------------------------------------------------------------- Route A: packing.hip
@pytest.mark.parametrize("dtype", DTYPES, ids=DTYPE_IDS)
@pytest.mark.parametrize("side", ["source", "destination"])
@pytest.mark.parametrize("mode,size,odd", CASES, ids=CASE_IDS)
def test_plane_ops_large_strides(arena, mode, size, odd, side, dtype):
    """One PLANE_NORMAL_XY op (two planes in, three out) and three PLANE_AFFINE ops in one table, forward (and backward, fp32).  The
    library refuses a written tensor whose first-to-last range holds a read one, so only one side crosses per case and the other sits
    above it."""
    h, w = size
    lib = N.lib()
    src_big, dst_big = ("mode", None) if side == "source" else (None, "mode")

    def forward(p):
        xy = p.inp(rand((2, 2, h, w), dtype, 81, 0.3, 0.7), big=src_big, high=src_big is None)
        planes = [p.inp(rand((2, 1, h, w), dtype, 82 + k), big=src_big, high=src_big is None) for k in range(3)]
        normal = p.out((2, 3, h, w), dtype, big=dst_big, high=dst_big is None)
        outs = [p.out((2, 1, h, w), dtype, big=dst_big, high=dst_big is None) for _ in range(3)]
        p.ready()
        ops = [N.PlaneOp(N.PLANE_NORMAL_XY, 0, *sp(xy), *sp(normal), None, 0, 0, 1.0, 0.0)]
        ops += [N.PlaneOp(N.PLANE_AFFINE, 0, a.data_ptr(), a.stride(0), 0, o.data_ptr(), o.stride(0), 0, None, 0, 0, 2.0, -1.0) for a, o in zip(planes, outs)]
        N.check(lib.pbr_plane_ops((N.PlaneOp * 4)(*ops), 4, 2, h * w, CODE[dtype], stream()))
    route_a(arena, forward, "plane_ops %s %s %s" % (side, mode, dtype), mode, odd)
    if dtype != torch.float32:
        return

    def backward(p):
        xy = p.inp(rand((2, 2, h, w), dtype, 81, 0.3, 0.7), big=src_big, high=src_big is None)
        up_n = p.inp(rand((2, 3, h, w), dtype, 86, -0.4, 0.6), big=src_big, high=src_big is None)
        ups = [p.inp(rand((2, 1, h, w), dtype, 87 + k, -0.4, 0.6), big=src_big, high=src_big is None) for k in range(3)]
        g_xy = p.out((2, 2, h, w), big=dst_big, high=dst_big is None)
        gs = [p.out((2, 1, h, w), big=dst_big, high=dst_big is None) for _ in range(3)]
        p.ready()
        ops = [N.PlaneOp(N.PLANE_NORMAL_XY, 0, *sp(up_n), *sp(g_xy), *sp(xy), 1.0, 0.0)]
        ops += [N.PlaneOp(N.PLANE_AFFINE, 0, a.data_ptr(), a.stride(0), 0, o.data_ptr(), o.stride(0), 0, None, 0, 0, 2.0, -1.0) for a, o in zip(ups, gs)]
        N.check(lib.pbr_plane_ops_backward((N.PlaneOp * 4)(*ops), 4, 2, h * w, N.F32, stream()))
    route_a(arena, backward, "plane_ops_backward %s %s" % (side, mode), mode, odd)


# ---------------------------------------------------------------- Route A: pack_image.hip
PACK_STRIDES = {    # name -> ((stride_c, stride_h, stride_w) of a [3,h,w] float32 source, the size)
    "channel-dense-form": ((big_stride(torch.float32, "plane", False), QUAD[1], 1), QUAD),
    "channel-odd": ((big_stride(torch.float32, "plane", True), ELEMENT[1], 1), ELEMENT),
    "row": ((64, (1 << 27) + 4, 1), QUAD),                  # rows 8 ... pass 2^32 bytes, rows 16 ... pass 2^31 elements
    "pixel": ((4096, 64, (1 << 26) + 1), QUAD),             # columns 16 ... pass 2^32 bytes, columns 32 ... pass 2^31 elements
}


@pytest.mark.parametrize("bits", [8, 16])
@pytest.mark.parametrize("which", list(PACK_STRIDES))
def test_pack_images_large_strides(arena, which, bits):
    """pbr_pack_images reads a [3,h,w] float32 source view through stride_c, stride_h, stride_w: the channel stride in the dense form (whole
    quads) and the general one, the row and the pixel stride in the general form; plain samples and an encoded normal in one table."""
    strides, (h, w) = PACK_STRIDES[which]
    lib = N.lib()
    sample = torch.uint8 if bits == 8 else torch.int16

    def run(p):
        a = p.inp(rand((3, h, w), torch.float32, 91, -0.1, 1.1), big=strides)
        n = p.inp(unit_normals((3, h, w), torch.float32, 92), big=strides)
        da, dn = p.out((h, w, 3), sample, big="dense"), p.out((h, w, 3), sample, big="dense")
        p.ready()
        table = (N.ImagePack * 2)(N.ImagePack(a.data_ptr(), *a.stride(), da.data_ptr(), 3, bits, 0, 0), N.ImagePack(n.data_ptr(), *n.stride(), dn.data_ptr(), 3, bits, 1, 0))
        N.check(lib.pbr_pack_images(table, 2, h, w, stream()))
    route_a(arena, run, "pack_images %s %d bits" % (which, bits), None, False)


# ---------------------------------------------------------------- Route A: rectify.hip
RECTIFY_STRIDES = (TWO32 + (1 << 27), (1 << 28) + 64, 4, 1)             # image, row, pixel (an RGBA-like pitch), channel; bytes


def rectify_homographies(size):
    h, w = size
    return np.stack([np.array([[1.02, 0.03, 0.4], [-0.02, 0.98, 0.7], [1e-4, 2e-4, 1.0]]), np.array([[0.9, -0.05, 2.5], [0.04, 1.05, -1.5], [-2e-4, 1e-4, 1.0]])])


@pytest.mark.parametrize("size", [QUAD, ELEMENT], ids=["quad", "pixel-form"])
def test_rectify_source_strides(arena, size):
    """Two photographs in the uint8 view of the arena: the second 2^32 + 2^27 bytes behind the first, rows 2^28 + 64 bytes apart (rows 16 ...
    pass 2^32 bytes inside an image, the last tap of image 1 lies 10.6e9 bytes in).  Targets and weights are dense by definition and sit
    above the source.  supersample 2, clip_level 250, to_linear."""
    h, w = size
    lib = N.lib()
    photos = torch.randint(0, 256, (2, h, w, 3), device="cuda", generator=torch.Generator(device="cuda").manual_seed(95), dtype=torch.uint8)
    table = (ctypes.c_double * 18)(*rectify_homographies(size).reshape(-1).tolist())

    def run(p):
        src = p.inp(photos, big=RECTIFY_STRIDES)
        targets, weights = p.out((2, 3, h, w), big="dense", high=True), p.out((2, 1, h, w), big="dense", high=True)
        p.ready()
        N.check(lib.pbr_rectify_images(src.data_ptr(), 2, h, w, *src.stride(), table, targets.data_ptr(), weights.data_ptr(), h, w, 2, 250, 1, stream()))
    route_a(arena, run, "rectify_images %dx%d" % size, None, False)

    def wrapper(p):
        src = p.inp(photos, big=RECTIFY_STRIDES)
        p.ready()
        return list(capture.rectify(src, rectify_homographies(size), size, supersample=2, clip_level=250, to_linear=True))
    route_a(arena, wrapper, "capture.rectify %dx%d" % size, None, False)


# ---------------------------------------------------------------- small shapes: photometric stereo under 3, 4 and 16 lights, 1 ... 4 passes
def photometric(c, weights=None, **kw):
    from test_gpu_photometric import dev
    _need(1)
    w = None if weights is None else dev(weights[:, None])
    return capture.photometric_stereo(dev(c.targets), w, light=c.light, light_intensity=c.intensity, light_size=PC.LIGHT_SIZE, **kw)


@pytest.mark.parametrize("size", [PC.SIZE, PC.SIBLING], ids=["24x36", "24x35"])
@pytest.mark.parametrize("name", ["gentle", "shadowed"])
@pytest.mark.parametrize("n_lights", [3, 4, 16])
def test_photometric_stereo_light_counts(n_lights, name, size):
    """L = 16 fills the shadow mask's 16 bits and the `live` mask at its widest; L = 3 is the smallest count with a solution."""
    import test_addressing_limits_host as H
    from test_gpu_photometric import held
    c, r = H.case(name, size, n_lights), H.solved(name, size, n_lights)
    if n_lights == 16 and name == "shadowed":                                            # on the CPU: bits 8 ... 15 are in use
        dropped = r.valid[None] & ~r.used
        assert dropped[8:].any() and dropped[15].any()
    held("L=%d %s %dx%d" % ((n_lights, name) + size), H.band(name, size, n_lights), photometric(c), r)


@pytest.mark.parametrize("n_lights", [3, 4])
def test_photometric_stereo_one_shot_masked_by_weight(n_lights):
    """Shot 1 has weight 0 on the left half: two shots of three leave no solution there (exactly invalid), three of four do."""
    import test_addressing_limits_host as H
    from test_gpu_photometric import held
    from test_photometric_host import band_for, float32_error
    c, weights = H.case("gentle", PC.SIZE, n_lights), H.masked_weights(n_lights)
    r = PO.photometric_stereo(c.targets, weights, c.light, c.intensity, light_size=PC.LIGHT_SIZE)
    r32 = PO.photometric_stereo(c.targets, weights, c.light, c.intensity, light_size=PC.LIGHT_SIZE, dtype=np.float32)
    band = band_for(float32_error(r32, r))
    n, a, conf = held("L=%d, shot 1 masked" % n_lights, band, photometric(c, weights), r)
    left = slice(0, PC.SIZE[1] // 2)
    if n_lights == 3:
        assert (conf[:, left] == 0).all() and (n[2, :, left] == 1).all() and (n[:2, :, left] == 0).all()
    else:
        assert (conf[:, left] > 0).mean() > 0.9


@pytest.mark.parametrize("size", [PC.SIZE, PC.SIBLING], ids=["24x36", "24x35"])
@pytest.mark.parametrize("iterations", [1, 2, 3, 4])
def test_photometric_stereo_iterations_on_the_shadowed_set(iterations, size):
    import test_addressing_limits_host as H
    from test_gpu_photometric import held
    c, r = H.case("shadowed", size), H.solved("shadowed", size, iterations=iterations)
    held("shadowed %dx%d K=%d" % (size + (iterations,)), H.band("shadowed", size, iterations=iterations), photometric(c, iterations=iterations), r)


# ---------------------------------------------------------------- Route B: one contiguous tensor past 2^31 elements
def seeded(seed):
    return torch.Generator(device="cuda").manual_seed(seed)


@pytest.mark.parametrize("kind", ["charbonnier", "l2"])
@pytest.mark.parametrize("dtype,H,W,need", [(torch.float16, 5, 1 << 29, 26), (torch.float32, 3, 1 << 30, 40)], ids=["fp16-5x2^29", "fp32-3x2^30"])
def test_smoothness_in_plane(dtype, H, W, need, kind):
    """One map of one channel whose rows are 2^29 fp16 (row 4 starts at element 2^31) or 2^30 fp32 elements long (the width limit; row 2 starts
    at 2^31): the offsets row W + x the kernel forms itself.  All rows of the first 64 and of the last 64 columns -- so the last columns of the
    last row, and both sides of the row starts where row W + x passes 2^31 -- against the float64 oracle evaluated on the columns and one
    halo column beside them, under tests/test_gpu_smoothness.py's rule (fp16: one fp16 ulp of the oracle's value; fp32: gradient / k within
    the band that covers 4 x the float32 oracle's own error).  A byte offset wrapped at 2^32 would reach the same columns 4 rows (fp16) or
    1 row (fp32) higher."""
    from test_gpu_smoothness import band_of
    _need(need)
    t0 = time.perf_counter()
    half = dtype == torch.float16
    p = torch.rand(1, H, W, device="cuda", generator=seeded(101), dtype=dtype)
    grad = torch.empty_like(p)
    assert p.numel() > TWO31 and (H - 1) * W >= TWO31
    loss, terms = priors._step([p], [grad], [None], [1.0], priors.KINDS[kind], 1e-3, False)
    torch.cuda.synchronize()
    up = TWO32 // p.element_size() // W                                                   # rows a byte offset wrapped at 2^32 lies higher
    worst, bands = 0.0, []
    for cols, keep in ((slice(0, 66), slice(0, 64)), (slice(W - 66, W), slice(2, 66))):
        crop = p[:, :, cols].double().cpu().numpy()
        got = grad[:, :, cols].double().cpu().numpy()[..., keep]
        _, g64 = SO.evaluate(crop, 1.0, kind, 1e-3, False, None, "sum")
        _, g32 = SO.evaluate(crop, 1.0, kind, 1e-3, False, None, "sum", dtype=np.float32)
        g64, g32 = g64[..., keep], g32[..., keep]
        if half:
            ulp = np.spacing(np.abs(g64).astype(np.float16)).astype(np.float64)
            worst, band, tol = max(worst, float((np.abs(got - g64) / ulp).max())), 1.0, float(ulp.max())
        else:
            band = band_of(float(np.abs(g32 - g64).max()), "in-plane gradient")
            worst, tol = max(worst, float(np.abs(got - g64).max())), band
        bands.append(band)
        _distinct(g64[0, H - 1], g64[0, H - 1 - up], tol, ("smoothness in-plane", kind, str(dtype)))
    print("\nsmoothness in-plane %s %s %d x %d: worst %s %.3e / band %s; loss %.6e; %.1f s"
          % (kind, dtype, H, W, "fp16 ulps" if half else "gradient / k", worst, bands, float(loss), time.perf_counter() - t0))
    assert worst <= min(bands) and np.isfinite(float(loss)) and float(loss) > 0 and float(terms[0]) == float(loss)


def test_adam_dense_state():
    """One box entry of 3 x 3 planes of 2^28 fp32 elements: parameter, exp_avg and exp_avg_sq are real (9 GiB each), the gradient is a stride-0
    expansion of one plane.  The state's offset q pixels and the parameter's b batch_stride + c plane_stride reach 2^31 at plane 8.  The first
    4096 elements of plane 0 and the last 4096 of plane 8 against tools/adam_oracle.py in float32, bit for bit; a byte offset wrapped at 2^32
    would reach plane 4, an element offset wrapped at 2^31 plane 0: their results differ."""
    from pypbr_amd.optim import _coefficients
    _need(34)
    t0 = time.perf_counter()
    B, C, px, n = 3, 3, 1 << 28, 4096
    param = torch.rand(B, C, px, device="cuda", generator=seeded(111)).mul_(0.97).add_(0.04)
    m = torch.rand(B, C, px, device="cuda", generator=seeded(112)).sub_(0.5).mul_(0.02)
    v = torch.rand(B, C, px, device="cuda", generator=seeded(113)).mul_(1e-4).add_(1e-9)
    g = torch.rand(px, device="cuda", generator=seeded(114)).sub_(0.5).mul_(0.1)
    assert (B * C - 1) * px >= TWO31
    windows = [(0, 0, slice(0, n)), (2, 2, slice(px - n, px)), (1, 1, slice(px - n, px)), (0, 0, slice(px - n, px))]     # first, far, wrapped at 2^32 B, at 2^31 el
    before = [[t[b, c, cols].cpu().numpy() for t in (param, m, v)] + [g[cols].cpu().numpy()] for b, c, cols in windows]
    entry = N.AdamTensor(param.data_ptr(), g.data_ptr(), m.data_ptr(), v.data_ptr(), None, px, C * px, px, 0, 0, B, C, N.F32, N.ADAM_BOX, 0.05, 1.0, 0.0, 0)
    table, coeffs = (N.AdamTensor * 1)(entry), (N.AdamCoeffs * 1)(_coefficients(1e-2, (0.9, 0.999), 1e-8, 2.0))
    assert N.lib().pbr_adam_check(table, 1, 1) == N.OK
    N.check(N.lib().pbr_adam_step(table, 1, coeffs, None, 1, stream()))
    torch.cuda.synchronize()
    want = [AO.step(p0, g0, m0, v0, 2, lr=1e-2, betas=(0.9, 0.999), eps=1e-8, bounds=(0.05, 1.0), dtype=np.float32) for p0, m0, v0, g0 in before]
    shares = []
    for (b, c, cols), ref in zip(windows[:2], want[:2]):
        got = [t[b, c, cols].cpu().numpy() for t in (param, m, v)]
        shares.append([float((a.view(np.int32) == r.astype(np.float32).view(np.int32)).mean()) for a, r in zip(got, ref)])
    print("\nadam dense state: share of bits equal to the float32 oracle's, (p, m, v) of the first and the far window: %s; clamped in the far window: %d; %.1f s"
          % (shares, int(((want[1][0] == np.float32(0.05)) | (want[1][0] == 1.0)).sum()), time.perf_counter() - t0))
    assert shares == [[1.0, 1.0, 1.0], [1.0, 1.0, 1.0]]
    for other in want[2:]:
        _distinct(want[1][0], other[0], 0.0, "adam dense state")


def window_stereo(targets, weights, c, full, y0, x0, dtype=np.float64):
    """tools/photometric_oracle.py on the window [y0, y0 + h) x [x0, x0 + w) of a grid of `full` pixels."""
    return PO.photometric_stereo(targets, weights, c.light, c.intensity, light_size=PC.LIGHT_SIZE, dtype=dtype, window=(y0, x0) + tuple(full))


def test_capture_of_sixteen_shots():
    """capture.rectify of 16 photographs (432 x 432, the gentle Lambertian set under 16 lights) into 16 x 3 x 6912 x 6912 targets -- 2.29e9
    floats, shot 15's planes start at 2.15e9 > 2^31 -- and capture.photometric_stereo on that stack: L = 16 at full size.  The first 32 x 32
    window of shot 0 and the last of shot 15 against tools/rectify_oracle.py (tests/test_gpu_rectify.py's held()); the first and the last
    32 x 32 window of the maps against tools/photometric_oracle.py (tests/test_gpu_photometric.py's held(), the band from the float32
    oracle's own error on the window).  Both kernels' pixel forms (outputs 4 bytes off a 16-byte boundary, through the C ABI): the last 4
    rows bit for bit.  The targets 2^32 bytes in front of shot 15's far window differ from it."""
    from test_gpu_photometric import held as held_stereo
    from test_gpu_rectify import held as held_rectify
    from test_photometric_host import band_for, float32_error
    import rectify_oracle as RO
    _need(44)
    t0 = time.perf_counter()
    L, S, hs, K = 16, 6912, 432, 32
    plane = S * S
    assert 45 * plane > TWO31
    c = PC.lambertian("gentle", (hs, hs), n_lights=L)
    photos = np.ascontiguousarray(np.moveaxis(np.floor(c.targets.astype(np.float64) * 255.0 + 0.5).astype(np.uint8), 1, -1))       # [L,hs,hs,3]
    hom = np.diag([hs / S, hs / S, 1.0])
    src = torch.from_numpy(photos).cuda()
    targets, weights = capture.rectify(src, np.broadcast_to(hom, (L, 3, 3)).copy(), (S, S))
    assert targets.shape == (L, 3, S, S) and targets[L - 1].storage_offset() > TWO31 and targets.is_contiguous()
    wins = {"first": (0, 0, 0), "far": (L - 1, S - K, S - K)}
    worst = {}
    for name, (l, y0, x0) in wins.items():
        shift = np.array([[1.0, 0, x0], [0, 1.0, y0], [0, 0, 1.0]])
        r = RO.rectify(photos[l], hom @ shift, (K, K))
        held_rectify("16 shots, %s window" % name, 1, targets[l, :, y0:y0 + K, x0:x0 + K], weights[l, :, y0:y0 + K, x0:x0 + K], r)
        worst[name] = r
    far = targets[L - 1, :, S - K:, S - K:]
    at = (targets[L - 1, :, S - K:, S - K:].storage_offset()
          + (torch.arange(3)[:, None, None] * plane + torch.arange(K)[None, :, None] * S + torch.arange(K)[None, None, :])) - (TWO32 // 4)
    _distinct(far.double().cpu().numpy(), targets.view(-1)[at.cuda()].double().cpu().numpy(), 4e-6, "rectified targets, 2^32 bytes earlier")
    t_rect = time.perf_counter() - t0
    # the pixel form of rectify: both outputs one float off their alignment
    lib = N.lib()
    tb, wb = torch.empty(L * 3 * plane + 4, device="cuda"), torch.empty(L * plane + 4, device="cuda")
    t2, w2 = tb[1:1 + L * 3 * plane].view(L, 3, S, S), wb[1:1 + L * plane].view(L, 1, S, S)
    assert t2.data_ptr() % 16 == 4
    table = (ctypes.c_double * (9 * L))(*np.broadcast_to(hom, (L, 3, 3)).reshape(-1).tolist())
    N.check(lib.pbr_rectify_images(src.data_ptr(), L, hs, hs, *src.stride(), table, t2.data_ptr(), w2.data_ptr(), S, S, 1, 0, 0, stream()))
    strips = [int((t2[L - 1, :, S - 4:] != targets[L - 1, :, S - 4:]).sum()), int((w2[L - 1, :, S - 4:] != weights[L - 1, :, S - 4:]).sum()),
              int((t2[0, :, :4] != targets[0, :, :4]).sum())]
    print("rectify, pixel form against quad form: differing elements in shot 15's last 4 rows (targets, weights) and shot 0's first 4 rows: %s" % strips)
    assert strips == [0, 0, 0]
    del tb, wb, t2, w2
    # photometric stereo on the stack
    got = capture.photometric_stereo(targets, weights, light=c.light, light_intensity=c.intensity, light_size=PC.LIGHT_SIZE)
    for name, (y0, x0) in (("first", (0, 0)), ("far", (S - K, S - K))):
        t_win = targets[:, :, y0:y0 + K, x0:x0 + K].cpu().numpy()
        w_win = weights[:, 0, y0:y0 + K, x0:x0 + K].cpu().numpy()
        r = window_stereo(t_win, w_win, c, (S, S), y0, x0)
        r32 = window_stereo(t_win, w_win, c, (S, S), y0, x0, np.float32)
        _, _, banded = PC.classes(r)
        assert banded.sum() >= K * K // 2, (name, int(banded.sum()))
        band = band_for(float32_error(r32, r))
        held_stereo("16 shots at %d^2, %s window" % (S, name), band, [t[:, y0:y0 + K, x0:x0 + K] for t in got], r)
    # the far window's own non-vacuity: shot 15 read 2^32 bytes early (the targets the rectify check gathered there) gives other maps
    t_wrapped = t_win.copy()
    t_wrapped[L - 1] = targets.view(-1)[at.cuda()].cpu().numpy()
    moved = window_stereo(t_wrapped, w_win, c, (S, S), y0, x0)
    _distinct(r.normal, moved.normal, band, "stereo far window, shot 15 read 2^32 bytes early")
    _distinct(r.albedo, moved.albedo, band, "stereo far window, shot 15 read 2^32 bytes early")
    # the pixel form of photometric stereo
    gd = Guards(257)                                                                      # an odd margin: every output 4 bytes off its 16-byte boundary
    outs = [gd.output((n, S, S)) for n in (3, 3, 1)]
    assert all(o.data_ptr() % 16 == 4 for o in outs)
    lt = (ctypes.c_float * (3 * L))(*np.asarray(c.light, dtype=np.float64).reshape(-1).tolist())
    it = (ctypes.c_float * (3 * L))(*np.broadcast_to(c.intensity, (L, 3)).reshape(-1).tolist())
    N.check(lib.pbr_photometric_stereo(targets.data_ptr(), weights.data_ptr(), 0, L, S, S, lt, it, N.LIGHT_POINT, PC.LIGHT_SIZE, 1, 3, 0.1, 1e-4, 0,
                                       outs[0].data_ptr(), outs[1].data_ptr(), outs[2].data_ptr(), stream()))
    strips = [int((o[:, S - 4:] != t_[:, S - 4:]).sum()) + int((o[:, :4] != t_[:, :4]).sum()) for o, t_ in zip(outs, got)]
    print("photometric stereo, pixel form against quad form: differing elements in the first and last 4 rows of (normal, albedo, confidence): %s" % strips)
    gd.check("photometric stereo, pixel form, 16 shots at %d^2" % S)                       # margins intact, every element written and finite
    assert strips == [0, 0, 0]
    print("\ncapture of 16 shots at %d^2: rectify and its windows %.1f s, everything %.1f s" % (S, t_rect, time.perf_counter() - t0))


STACK_FAMILIES = {      # name -> (view_type, whether every shot has its own camera)
    "orthographic": ("directional", False), "camera": ("point", False), "per-shot-camera": ("point", True),
}


@pytest.mark.parametrize("family", list(STACK_FAMILIES))
def test_light_stack_past_2_to_31_elements(family):
    """F.cook_torrance_stack and the loss step, plain and weighted, of one family -- orthographic (ct_stack.hip), one camera
    (ct_camera_stack.hip), one camera per shot (ct_view_stack.hip) and their weighted siblings -- on one fp32 material of 6912 x 6912 under
    16 point lights: the stack and the targets are 2.29e9 floats, shot 15's planes start at (int64_t)l * 3 * plane = 2.15e9 > 2^31.  The
    first rows of shot 0 and the last rows of shot 15 against float64 (torch_oracle.cook_torrance | tools/camera_oracle.py with y_offset /
    H_total, as the families' own files: the forward within 2e-6; the loss within 1e-6 (1 + loss) of the float64 mean over the library's
    own stack; gradients within test_gpu_light_stack._tol of float64 autograd on the rows).  _tol is 2e-5 max|g| + 1e-9, made for stacks of
    16 x 64 pixels: the gradient of a mean over 2.3e9 values is 1e-9 itself and the absolute term would pass anything, so the loss goes
    backward under the upstream factor n / (3 L 16 64) (as that file's own upstream-gradient test does with 3.0), which gives each pixel's
    gradient the size it has in that file's first case; the reference carries the same factor.  The targets 2^32 bytes in front of shot 15's
    last rows give other gradients."""
    import camera_oracle as CO
    import torch_oracle as O
    from pypbr_amd import functional as F
    from test_gpu_addressing_limits import _maps
    from test_gpu_light_stack import _tol
    from test_gpu_parity import TRACK
    _need(40)
    t0 = time.perf_counter()
    view_type, per_shot = STACK_FAMILIES[family]
    L, S, R = 16, 6912, 4
    plane, n = S * S, 16 * 3 * S * S
    k = n / (3 * L * 16 * 64)
    maps = _maps(S, S, 141)
    ang = torch.arange(L, dtype=torch.float32) * (2 * np.pi / L) + 0.3
    lights = torch.stack([0.55 * torch.cos(ang), 0.55 * torch.sin(ang), 0.7 + 0.02 * torch.arange(L)], 1)
    intens = torch.rand(L, 3, generator=torch.Generator().manual_seed(142)) * 0.7 + 0.3
    if view_type == "directional":
        view = torch.tensor([0.05, 0.1, 0.9])
    elif per_shot:
        view = torch.stack([0.2 * torch.sin(ang), 0.2 * torch.cos(ang), 1.1 + 0.03 * torch.arange(L)], 1)       # a hand-held camera: [L,3]
    else:
        view = torch.tensor([0.1, -0.15, 1.2])
    kw = dict(view_dir=view, light=lights, light_intensity=intens, light_type="point", light_size=1.5, view_type=view_type)
    targets = torch.rand(L, 3, S, S, device="cuda", generator=seeded(143))
    weights = torch.rand(L, 1, S, S, device="cuda", generator=seeded(144))
    assert targets[L - 1].storage_offset() > TWO31

    def ref_rows(leaves, y0, l):
        if view_type == "directional":
            return O.cook_torrance(*leaves, None, view=view.double(), light=lights[l].double(), intensity=intens[l].double(), light_type="point",
                                   light_size=1.5, y_offset=y0, H_total=S)
        return CO.cook_torrance_camera(*leaves, None, camera=(view[l] if per_shot else view).double(), lights=lights[l:l + 1].double(),
                                       intensities=intens[l:l + 1].double(), light_type="point", light_size=1.5, y_offset=y0, H_total=S)
    out = F.cook_torrance_stack(*maps, **kw)
    assert out.shape == (L, 3, S, S)
    worst = 0.0
    for l, y0 in ((0, 0), (L - 1, S - R)):
        crop = [t[:, y0:y0 + R].double().cpu() for t in maps]
        ref = ref_rows(crop, y0, l)
        worst = max(worst, float((out[l, :, y0:y0 + R].double().cpu() - ref).abs().max()))
    at = out[L - 1, :, S - R:].storage_offset() + (torch.arange(3)[:, None, None] * plane + torch.arange(R)[None, :, None] * S + torch.arange(S)[None, None, :]) - (TWO32 // 4)
    _distinct(ref.numpy(), out.view(-1)[at.cuda()].double().cpu().numpy(), TRACK, "light stack, 2^32 bytes earlier")
    loss64 = {None: 0.0, "weighted": 0.0}
    for l in range(L):
        d = (out[l].double() - targets[l].double()) ** 2
        loss64[None] += float(d.sum()) / n
        loss64["weighted"] += float((d * weights[l].double()).sum()) / n
        del d
    del out
    print("\n%s stack forward at %d^2, L = %d: worst |hip - float64| %.2e / band %.0e" % (family, S, L, worst, TRACK))
    assert worst <= TRACK
    wrapped_targets = targets.view(-1)[at.cuda()].double().cpu()
    prefix = {"orthographic": "", "camera": "camera_", "per-shot-camera": "view_"}[family]
    for mode in (None, "weighted"):
        leaves = [t.clone().requires_grad_(True) for t in maps]
        before = dict(F.STACK_LAUNCHES)
        loss = F.rendering_loss_mse_stack(*leaves, targets=targets, weights=weights if mode else None, **kw)
        stepped = [name for name in F.STACK_LAUNCHES if F.STACK_LAUNCHES[name] != before.get(name, 0)]
        (loss * k).backward()
        errs = []
        for y0, swap in ((0, False), (S - R, False), (S - R, True)):
            crop = [t[:, y0:y0 + R].double().cpu().requires_grad_(True) for t in maps]
            total = 0.0
            for l in range(L):
                tgt = wrapped_targets if (swap and l == L - 1) else targets[l, :, y0:y0 + R].double().cpu()
                d = (ref_rows(crop, y0, l) - tgt) ** 2
                total = total + ((d * weights[l, :, y0:y0 + R].double().cpu()) if mode else d).sum()
            (total * (k / n)).backward()
            if swap:
                _distinct(want[0].numpy(), crop[0].grad.numpy(), _tol(torch.float32, float(want[0].abs().max())), (family, "step", mode))
                continue
            want = [t.grad for t in crop]
            for name, x, y in zip(("albedo", "normal", "roughness", "metallic"), leaves, want):
                errs.append((name, y0, float((x.grad[:, y0:y0 + R].double().cpu() - y).abs().max()), _tol(torch.float32, float(y.abs().max()))))
        print("%s step%s (%s): loss %.9g (float64 over the library's stack %.9g); gradient rows (map, row, error, band): %s; %.1f s"
              % (family, " weighted" if mode else "", stepped, float(loss.detach()), loss64[mode], ["%s %d %.2e / %.2e" % e for e in errs], time.perf_counter() - t0))
        assert stepped == [prefix + ("weighted_" if mode else "") + "mse_stack_step"], (family, mode, stepped, "the one-pass step of this family did not serve the call")
        assert abs(float(loss.detach()) - loss64[mode]) <= 1e-6 * (1 + loss64[mode])
        assert all(e <= b for _, _, e, b in errs)


def test_camera_batch_past_2_to_31_elements():
    """The perspective camera's forward and its MSE step (ct_camera.hip; cook_torrance and rendering_loss_mse with view_type="point") over
    12 x 8192^2 fp32 materials without a normal map, the batch shape tests/test_gpu_addressing_limits.py uses for the base kernels:
    material 11's planes, result and target start 2.2e9 elements in.  Material 0's first rows and material 11's last rows against
    tools/camera_oracle.py in float64 (tests/test_gpu_camera.py: the forward within 2e-6; the loss within 1e-6 (1 + loss) of the float64
    mean over the library's own forward; map gradients within test_gpu_light_stack._tol, under the upstream factor n / (3 x 16 x 64) for
    the reason test_light_stack_past_2_to_31_elements gives).  Material 11's far rows differ from material 0's, where a wrapped material
    offset would read."""
    import camera_oracle as CO
    from pypbr_amd import functional as F
    from test_gpu_addressing_limits import _maps
    from test_gpu_light_stack import _tol
    _need(64)
    t0 = time.perf_counter()
    B, H, W, R = 12, 8192, 8192, 4
    n = B * 3 * H * W
    k = n / (3 * 16 * 64)
    maps = _maps(H, W, 151, B=B, normal=False)
    camera, light, inten = torch.tensor([0.1, -0.15, 1.2]), torch.tensor([0.1, 0.1, 1.0]), torch.tensor([1.0, 0.9, 0.8])
    kw = dict(view_dir=camera, light=light, light_intensity=inten, light_type="point", light_size=1.5, view_type="point")
    target = torch.rand(B, 3, H, W, device="cuda", generator=seeded(152))
    assert target[B - 1].storage_offset() > TWO31 and maps[0][B - 1].storage_offset() > TWO31

    def ref_rows(leaves, y0):
        return CO.cook_torrance_camera(leaves[0], None, leaves[2], leaves[3], None, camera=camera.double(), lights=light[None].double(),
                                       intensities=inten[None].double(), light_type="point", light_size=1.5, y_offset=y0, H_total=H)
    out = F.cook_torrance(*maps, **kw)
    assert out.shape == (B, 3, H, W)
    refs = {}
    for b, y0 in ((0, 0), (B - 1, H - R), (0, H - R)):
        refs[b, y0] = ref_rows([None if t is None else t[b, :, y0:y0 + R].double().cpu() for t in maps], y0)
    worst = max(float((out[b, :, y0:y0 + R].double().cpu() - refs[b, y0]).abs().max()) for b, y0 in ((0, 0), (B - 1, H - R)))
    loss64 = sum(float(((out[b].double() - target[b].double()) ** 2).sum()) for b in range(B)) / n
    del out
    print("\ncamera forward over %d x %d^2: worst |hip - float64| %.2e / band 2e-06" % (B, H, worst))
    assert worst <= 2e-6
    _distinct(refs[B - 1, H - R].numpy(), refs[0, H - R].numpy(), 2e-6, "camera forward, material 0 in place of material 11")
    leaves = [None if t is None else t.requires_grad_(True) for t in maps]
    loss = F.rendering_loss_mse(*leaves, target=target, **kw)
    (loss * k).backward()

    def grads64(b, y0, tgt):
        crop = [None if t is None else t[b, :, y0:y0 + R].detach().double().cpu().requires_grad_(True) for t in maps]
        (((ref_rows(crop, y0) - tgt.double().cpu()) ** 2).sum() * (k / n)).backward()
        return [None if t is None else t.grad for t in crop]
    errs = []
    for b, y0 in ((0, 0), (B - 1, H - R)):
        want = grads64(b, y0, target[b, :, y0:y0 + R])
        for name, x, y in zip(("albedo", "normal", "roughness", "metallic"), leaves, want):
            if x is not None:
                errs.append((name, b, float((x.grad[b, :, y0:y0 + R].double().cpu() - y).abs().max()), _tol(torch.float32, float(y.abs().max()))))
    wrong = grads64(B - 1, H - R, target[0, :, H - R:])
    print("camera MSE step: loss %.9g (float64 over the library's forward %.9g); gradient rows (map, material, error, band): %s; %.1f s"
          % (float(loss.detach()), loss64, ["%s %d %.2e / %.2e" % e for e in errs], time.perf_counter() - t0))
    assert abs(float(loss.detach()) - loss64) <= 1e-6 * (1 + loss64)
    assert all(e <= band for _, _, e, band in errs)
    _distinct(want[0].numpy(), wrong[0].numpy(), _tol(torch.float32, float(want[0].abs().max())), "camera MSE step, material 0's target")


# ---------------------------------------------------------------- the largest accepted plane: 46340 x 46340 = 2^31 - 88 047 elements
BIG = 46340


def rotate_indices_window(plan, i0, j0, h, w):
    """_rotate_ops.rotate_indices for the output window [i0, i0 + h) x [j0, j0 + w) alone: the same float32 steps on the window's own
    coordinates (the whole map's index tensor is 17 GB at 46340^2)."""
    f32 = torch.float32
    x = torch.arange(j0, j0 + w, dtype=f32)[None, :] + torch.tensor(plan.x0, dtype=f32)
    y = torch.arange(i0, i0 + h, dtype=f32)[:, None] + torch.tensor(plan.y0, dtype=f32)
    t = [torch.tensor(v, dtype=f32) for v in (plan.t00, plan.t10, plan.t01, plan.t11)]
    gx, gy = x * t[0] + y * t[1], x * t[2] + y * t[3]
    ix = torch.round(((gx + 1) * plan.Wp - 1) / 2).long()
    iy = torch.round(((gy + 1) * plan.Hp - 1) / 2).long()
    inside = (ix >= 0) & (ix < plan.Wp) & (iy >= 0) & (iy < plan.Hp)
    sx, sy = ix - plan.pad, iy - plan.pad
    if plan.circular:
        sx, sy = sx % plan.w, sy % plan.h
    else:
        inside &= (sx >= 0) & (sx < plan.w) & (sy >= 0) & (sy < plan.h)
    return torch.where(inside, sy * plan.w + sx, torch.full_like(sx, -1))


def test_rotation_at_its_largest_plane():
    """rotate_maps' kernel on one fp16 plane of 46340 x 46340, the largest rotate_arguments accepts (in-plane offsets are 32-bit): rotated by
    2 degrees, constant padding (the padded image is 84732 wide, its coordinates exact in fp32).  The first 32 x 32 window and a window of
    the last 32 rows -- 3000 columns from the corner that rotates into the source: the corners themselves are fill -- bit-equal to a gather
    through the index function evaluated on the window (rotate_indices_window, held to rotate_indices on a small plan first).  The window's
    source offsets and its own reach 2.1e9 elements, 4.2e9 bytes (2^31 bytes passed, 2^32 not: a plane cannot); the elements 2^31 bytes
    earlier differ."""
    from pypbr_amd._rotate_ops import _rotate_raw, rotate_indices, rotate_plan
    _need(12)
    t0 = time.perf_counter()
    small = rotate_plan(24, 36, 2.0)
    assert torch.equal(rotate_indices_window(small, 5, 7, 11, 13), rotate_indices(small)[5:16, 7:20])
    plan = rotate_plan(BIG, BIG, 2.0)
    assert (plan.H, plan.W) == (BIG, BIG) and plan.Wp < (1 << 24)
    src = torch.rand(1, 1, BIG, BIG, device="cuda", generator=seeded(161), dtype=torch.float16)
    out = _rotate_raw(src, plan, -1)
    K = 32
    candidates = [(0, 0)] + [(BIG - K, j0) for j0 in (3000, BIG - 3000 - K)]
    flat, figures = src.view(-1), []
    for i0, j0 in candidates:
        idx = rotate_indices_window(plan, i0, j0, K, K)
        valid = idx >= 0
        want = torch.where(valid.cuda(), flat[idx.clamp(min=0).cuda()], torch.zeros((), dtype=torch.float16, device="cuda"))
        got = out[0, 0, i0:i0 + K, j0:j0 + K]
        figures.append((i0, j0, float(valid.float().mean()), int(idx.max()), int((got != want).sum())))
    print("\nrotation at %d^2 fp16: (row, column, share with a source, largest source offset, differing elements) %s; %.1f s" % (BIG, figures, time.perf_counter() - t0))
    assert all(f[4] == 0 for f in figures)
    far = max(figures[1:], key=lambda f: f[2])
    assert far[2] > 0.99 and far[3] > 0.95 * TWO31 and far[0] * BIG + far[1] > 0.99 * TWO31
    idx = rotate_indices_window(plan, far[0], far[1], K, K)
    _distinct(flat[idx.clamp(min=0).cuda()].double().cpu().numpy(), flat[(idx.clamp(min=0) - (1 << 30)).cuda()].double().cpu().numpy(), 0.0, "rotation, 2^31 bytes earlier")


def test_height_ops_at_their_largest_plane():
    """pbr_normal_divergence and its backward, pbr_height_stats + pbr_height_normalize and their backward on one 46340 x 46340 plane
    (2^31 - 88 047 pixels, the largest map_shape_ok takes), fp32.  The first and the far-corner 32 x 32 windows: the divergence bit-equal
    to tests/test_gpu_height_ops.py's ref_div; its backward and the normalisation's within that file's _close of float64 (autograd of
    ref_div on the window and two halo pixels; the normalisation's formula with the plane's float64 mean, minimum and range, which are
    reduced on the device in float64).  The height map's minimum and maximum are planted in its last 8 elements, so the argmin / argmax the
    kernel keeps as float bits are 2^31 - 88 050 and 2^31 - 88 053, and their gradient entries collect sums over the whole plane.  Each far
    window differs from the window 2^32 bytes (2^30 elements) in front of it."""
    from pypbr_amd import _height_ops as HO
    from test_gpu_height_ops import _close, ref_div
    _need(100)
    t0 = time.perf_counter()
    H = W = BIG
    K, n_px = 32, BIG * BIG
    wins = {"first": (0, 0), "far": (H - K, W - K)}

    def early(t2d, y0, x0, h=K, w=K):
        """The window of a [H,W] plane 2^30 elements in front of (y0, x0)."""
        at = (torch.arange(y0, y0 + h)[:, None] * W + torch.arange(x0, x0 + w)[None, :]) - (1 << 30)
        return t2d.reshape(-1)[at.cuda()].double().cpu().numpy()
    # the divergence and its backward
    n = torch.rand(1, 3, H, W, device="cuda", generator=seeded(171))
    n[:, :2] -= 0.5
    n[:, 2] += 0.5
    div = HO._divergence_raw(n, 1.5, False)
    dd = torch.rand(1, H, W, device="cuda", generator=seeded(172)).sub_(0.4)
    gn = HO._divergence_backward_raw(n, dd, 1.5, False)
    for name, (y0, x0) in wins.items():
        ya, xa = max(y0 - 2, 0), max(x0 - 2, 0)                                           # two halo pixels in front; behind: the map's edge or one pixel
        yb, xb = min(y0 + K + 1, H), min(x0 + K + 1, W)
        crop = n[0, :, ya:yb, xa:xb].cpu()
        inner = (slice(y0 - ya, y0 - ya + K), slice(x0 - xa, x0 - xa + K))
        want = ref_div(crop, 1.5, False)[inner]
        differing = int((div[0, y0:y0 + K, x0:x0 + K].cpu() != want).sum())
        print("\ndivergence at %d^2, %s window: %d elements differ from ref_div" % (BIG, name, differing))
        assert differing == 0
        x = crop.double().requires_grad_()
        (ref_div(x, 1.5, False) * dd[0, ya:yb, xa:xb].double().cpu()).sum().backward()
        _close(gn[0, :, y0:y0 + K, x0:x0 + K], x.grad[(slice(None),) + inner], "divergence backward at %d^2, %s window" % (BIG, name))
    _distinct(want.double().numpy(), early(div[0], H - K, W - K), 0.0, "divergence, 2^32 bytes earlier")
    del n, div, dd, gn
    # the height statistics, the normalisation and its backward
    h = torch.rand(1, H, W, device="cuda", generator=seeded(173)).mul_(3.0).sub_(1.0)
    flat = h.view(-1)
    flat[n_px - 3], flat[n_px - 6] = -2.5, 4.0                                            # the minimum and the maximum, at the far end
    out, stats = HO._normalize_raw(h, torch.float32)
    mean = sum(float(flat[i:i + (1 << 28)].double().sum()) for i in range(0, n_px, 1 << 28)) / n_px
    mn, rng = -2.5 - mean, 6.5
    idx = stats[:, 3:].contiguous().view(torch.int32).cpu()
    print("height statistics at %d^2: mean %.9g (float64 %.9g), argmin %d, argmax %d" % (BIG, float(stats[0, 0]), mean, int(idx[0, 0]), int(idx[0, 1])))
    assert idx.tolist() == [[n_px - 3, n_px - 6]]
    G = torch.rand(1, 1, H, W, device="cuda", generator=seeded(174)).sub_(0.4)
    dh = HO._normalize_backward_raw(G, out, stats)
    y64 = lambda t: ((t.double() - mean) - mn) / (rng + 1e-8)                             # noqa: E731
    sum_g = sum(float(G.view(-1)[i:i + (1 << 28)].double().sum()) for i in range(0, n_px, 1 << 28))
    sum_gy = sum(float((G.view(-1)[i:i + (1 << 28)].double() * y64(flat[i:i + (1 << 28)])).sum()) for i in range(0, n_px, 1 << 28))
    for name, (y0, x0) in wins.items():
        ref = y64(h[0, y0:y0 + K, x0:x0 + K].cpu())
        err = float((out[0, 0, y0:y0 + K, x0:x0 + K].double().cpu() - ref).abs().max())
        print("height normalisation at %d^2, %s window: |out - float64| %.2e / band 2e-06" % (BIG, name, err))
        assert err <= 2e-6
        # d/dh of sum G y: G / (range + eps) everywhere; the minimum also takes -(sum G - sum G y) / (range + eps), the maximum -sum G y / (range + eps)
        g64 = G[0, 0, y0:y0 + K, x0:x0 + K].double().cpu() / (rng + 1e-8)
        if name == "far":
            g64[K - 1, K - 3] += -(sum_g - sum_gy) / (rng + 1e-8)
            g64[K - 1, K - 6] += -sum_gy / (rng + 1e-8)
        _close(dh[0, y0:y0 + K, x0:x0 + K], g64, "normalisation backward at %d^2, %s window" % (BIG, name))
    _distinct(ref.numpy(), early(out[0, 0], H - K, W - K), 2e-6, "height normalisation, 2^32 bytes earlier")
    print("height ops at %d^2: %.1f s" % (BIG, time.perf_counter() - t0))
