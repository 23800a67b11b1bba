"""Photograph rectification on the device (csrc/rectify.hip, pbr_rectify_images; pypbr_amd.capture.rectify) against the float64 oracle of
its definition (tools/rectify_oracle.py) on the populations tests/test_rectify_host.py pins (tools/rectify_cases.py): a 40 x 56 x 3
photograph onto a 24 x 36 grid -- four workgroups of the quad form, ragged on both axes -- fully inside, hanging over every edge, across a
horizon, and with clipped taps.

Tolerances.  The kernel forms its coordinates in float64, rounds fx and fy to float32 and weighs and sums in float32: at most 4 S^2 + 4
roundings of values <= 1, (4 S^2 + 4) 2^-24 <= 4.1e-6 at S = 4, for any source size.  The bands are the project's two standing ones above
that bound: 2e-6 at S = 1 (bound 4.8e-7), 1e-5 at S = 2 and 4 (bounds 1.2e-6, 4.1e-6).  They hold for `weights` and for `weights * targets`
(the premultiplied value) on EVERY pixel -- both are continuous in the coordinates -- and for `targets` itself, a quotient by the
coverage, within 4 x the band where the oracle's coverage is >= 0.25.  Where the oracle has zero coverage with margin (no sub-sample within
0.01 source pixels of a bound, no |d| < 1e-9) both outputs are exactly 0.  With to_linear the curve's own error comes on top: hardware log2
and exp2, about 1 ulp each, on an exponent of magnitude <= 2.4 x 4.2 -- 1.5e-6 on values <= 1 -- so that run is made at S = 2, whose band
of 1e-5 covers 1.2e-6 + 1.5e-6.  The bit-for-bit tests need no tolerance."""
import ctypes
import functools
import os
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
import rectify_cases as C  # noqa: E402
import rectify_oracle as O  # noqa: E402

from pypbr_amd import _native as N  # noqa: E402
from pypbr_amd import capture  # noqa: E402
from pypbr_amd import functional as F  # noqa: E402

pytestmark = pytest.mark.gpu

IMG = C.photograph()
HOM = C.homographies()
H, W = C.SIZE
Hs, Ws = C.SOURCE_SHAPE[:2]
SETS = ("inside", "overhang", "horizon")
BAND = {1: 2e-6, 2: 1e-5, 4: 1e-5}
EDGE, UNWRITTEN, G = -777.0, -1234.0, 256


@functools.lru_cache(maxsize=None)
def oracle(name, S, clip=None, to_linear=False, size=C.SIZE):
    return O.rectify(IMG, HOM[name], size, supersample=S, clip_level=clip, to_linear=to_linear)


def translation(tx, ty):
    return np.array([[1.0, 0, tx], [0, 1.0, ty], [0, 0, 1.0]])


def held(what, S, targets, weights, r):
    """One image of a launch against its oracle result at the bands of S; the figures are printed before anything is asserted."""
    t, w = targets.double().cpu().numpy(), weights.double().cpu().numpy().reshape(r.coverage.shape)
    band = BAND[S]
    direct = r.coverage >= 0.25
    zero = C.clear_zero(r)
    e_w, e_v = np.abs(w - r.coverage).max(), np.abs(w[None] * t - r.value).max()
    e_t = np.abs(t - r.targets)[:, direct].max() if direct.any() else 0.0
    print("%-28s S=%d  |weights| %.2e  |weights*targets| %.2e  (band %.0e)   |targets| %.2e on %d pixels (4 x band)   exact zeros on %d pixels"
          % (what, S, e_w, e_v, band, e_t, int(direct.sum()), int(zero.sum())))
    assert np.isfinite(t).all() and np.isfinite(w).all()
    assert w.min() >= 0 and w.max() <= 1 and t.min() >= 0 and t.max() <= 1
    assert e_w <= band and e_v <= band, what
    assert e_t <= 4 * band, what
    assert (w[zero] == 0).all() and (t[:, zero] == 0).all(), what
    assert (t[:, w == 0] == 0).all(), what                   # a masked-out target is exactly 0 wherever the kernel itself found no coverage


@pytest.fixture(scope="module")
def photo():
    return torch.from_numpy(IMG).cuda()


@pytest.mark.parametrize("S", [1, 2, 4])
def test_three_sets_in_one_launch_against_the_oracle(photo, S):
    images = photo[None].expand(3, Hs, Ws, 3)                        # image stride 0: one photograph under three homographies
    before = capture.CALLS["rectify_images"]
    targets, weights = capture.rectify(images, np.stack([HOM[n] for n in SETS]), C.SIZE, supersample=S)
    assert capture.CALLS["rectify_images"] == before + 1
    assert tuple(targets.shape) == (3, 3, H, W) and tuple(weights.shape) == (3, 1, H, W)
    assert targets.dtype == weights.dtype == torch.float32 and targets.is_cuda and targets.is_contiguous() and weights.is_contiguous()
    for l, name in enumerate(SETS):
        held(name, S, targets[l], weights[l], oracle(name, S))
    assert (weights[0].cpu().numpy() >= 1 - BAND[S]).all()           # `inside`: every pixel fully covered


@pytest.mark.parametrize("S", [1, 2, 4])
def test_clipped_taps_count_as_uncovered(photo, S):
    targets, weights = capture.rectify(photo, HOM["inside"], C.SIZE, supersample=S, clip_level=C.CLIP_LEVEL)
    r = oracle("inside", S, clip=C.CLIP_LEVEL)
    held("clip %d" % C.CLIP_LEVEL, S, targets[0], weights[0], r)
    full, partial, zero = C.classes(r.coverage)
    w = weights[0, 0].cpu().numpy()
    assert (w[zero] == 0).all() and (w[partial] > 0).all() and (w[partial] < 1).all()          # (clipping is an integer test: no margin needed)
    assert (targets[0].cpu().numpy()[:, full | partial].max() < C.CLIP_LEVEL / 255.0 + BAND[S])   # no clipped sample reaches a target
    _, w_off = capture.rectify(photo, HOM["inside"], C.SIZE, supersample=S)          # without a clip level nothing is dropped
    assert (w_off >= weights).all()


def test_to_linear_weighs_linear_values(photo):
    targets, weights = capture.rectify(photo, HOM["overhang"], C.SIZE, supersample=2, to_linear=True)
    held("overhang, to_linear", 2, targets[0], weights[0], oracle("overhang", 2, to_linear=True))
    plain, w_plain = capture.rectify(photo, HOM["overhang"], C.SIZE, supersample=2)
    assert torch.equal(weights, w_plain) and not torch.equal(targets, plain)


def _unpacked(samples_hwc: torch.Tensor) -> torch.Tensor:
    """pbr_unpack_image's floats of a dense (H,W,3) uint8 device tensor: [3,H,W]."""
    h, w, c = samples_hwc.shape
    out = torch.empty((c, h, w), dtype=torch.float32, device=samples_hwc.device)
    return F.unpack_image(samples_hwc.contiguous(), 8, (1, w * c, c), (c, h, w), out)


@pytest.mark.parametrize("tx,ty", [(5, -3), (-2, 4), (0, 0), (30, 20)])
def test_integer_translation_is_unpack_image_bit_for_bit(photo, tx, ty):
    """The exactness clause: S = 1 and an integer translation give pbr_unpack_image's floats and weights of exactly 0 or 1."""
    targets, weights = capture.rectify(photo, translation(tx, ty), C.SIZE)
    floats = _unpacked(photo)
    want_t, want_w = torch.zeros(3, H, W, device="cuda"), torch.zeros(1, H, W, device="cuda")
    ys = [y for y in range(H) if 0 <= y + ty < Hs]
    xs = [x for x in range(W) if 0 <= x + tx < Ws]
    assert ys and xs and (len(ys) < H or len(xs) < W or (tx, ty) == (0, 0))
    want_t[:, ys[0]:ys[-1] + 1, xs[0]:xs[-1] + 1] = floats[:, ys[0] + ty:ys[-1] + 1 + ty, xs[0] + tx:xs[-1] + 1 + tx]
    want_w[:, ys[0]:ys[-1] + 1, xs[0]:xs[-1] + 1] = 1.0
    assert torch.equal(weights[0], want_w) and torch.equal(targets[0], want_t)


def test_tail_path_equals_the_quad_path_bit_for_bit(photo):
    """Width 37 is written one pixel per lane, width 36 four: the same homography gives the same bits on the 36 shared columns."""
    for S in (1, 2, 4):
        t36, w36 = capture.rectify(photo, HOM["overhang"], (H, 36), supersample=S)
        t37, w37 = capture.rectify(photo, HOM["overhang"], (H, 37), supersample=S)
        assert torch.equal(t37[..., :36], t36) and torch.equal(w37[..., :36], w36)
        r = O.rectify(IMG, HOM["overhang"], (H, 37), supersample=S)
        held("overhang, width 37", S, t37[0], w37[0], r)


def test_rgba_view_equals_the_dense_rgb_call_bit_for_bit(photo):
    rgba = torch.cat([photo, torch.full((Hs, Ws, 1), 77, dtype=torch.uint8, device="cuda")], dim=2)
    dense = capture.rectify(photo, HOM["overhang"], C.SIZE, supersample=2, clip_level=C.CLIP_LEVEL)
    whole = capture.rectify(rgba, HOM["overhang"], C.SIZE, supersample=2, clip_level=C.CLIP_LEVEL)          # C = 4: alpha is never read
    view = rgba[..., :3]
    assert not view.is_contiguous() and view.stride() == (Ws * 4, 4, 1)
    viewed = capture.rectify(view, HOM["overhang"], C.SIZE, supersample=2, clip_level=C.CLIP_LEVEL)
    for got in (whole, viewed):
        assert torch.equal(got[0], dense[0]) and torch.equal(got[1], dense[1])
    # host data goes up as bytes and gives the same bits: a numpy array, a list of PIL images
    from PIL import Image
    for host in (IMG, [Image.fromarray(IMG)], torch.from_numpy(IMG)):
        got = capture.rectify(host, HOM["overhang"], C.SIZE, supersample=2, clip_level=C.CLIP_LEVEL)
        assert got[0].is_cuda and torch.equal(got[0], dense[0]) and torch.equal(got[1], dense[1])


def test_seventeen_images_are_two_chunks_and_equal_per_image_calls(photo):
    L = 17
    images = torch.stack([torch.roll(photo, shifts=(l, 2 * l), dims=(0, 1)) for l in range(L)])
    homs = np.stack([HOM[SETS[l % 3]] @ translation(0.37 * l, -0.21 * l) for l in range(L)])
    before = capture.CALLS["rectify_images"]
    targets, weights = capture.rectify(images, homs, C.SIZE, supersample=2)
    assert capture.CALLS["rectify_images"] == before + 2 and tuple(targets.shape) == (L, 3, H, W) and tuple(weights.shape) == (L, 1, H, W)
    for l in range(L):
        t, w = capture.rectify(images[l], homs[l], C.SIZE, supersample=2)
        assert torch.equal(t[0], targets[l]) and torch.equal(w[0], weights[l]), l
    # a list of host arrays goes the same way
    t2, w2 = capture.rectify([im.cpu().numpy() for im in images], homs, C.SIZE, supersample=2)
    assert torch.equal(t2, targets) and torch.equal(w2, weights)


def _guarded_call(width, S, misalign=0, clip=0, lin=0):
    """pbr_rectify_images through the C ABI on the three sets: the source inside 0xFF margins, both outputs inside EDGE margins with their
    interior pre-filled.  Returns (targets, weights) after checking the margins and that every element was written."""
    src = torch.full((Hs * Ws * 3 + 2 * G,), 255, dtype=torch.uint8, device="cuda")
    src[G:G + Hs * Ws * 3] = torch.from_numpy(IMG).reshape(-1).cuda()
    nt, nw = 3 * 3 * H * width, 3 * H * width
    tbuf = torch.full((nt + 2 * G + misalign,), EDGE, dtype=torch.float32, device="cuda")
    wbuf = torch.full((nw + 2 * G + misalign,), EDGE, dtype=torch.float32, device="cuda")
    t, w = tbuf[G + misalign:G + misalign + nt], wbuf[G + misalign:G + misalign + nw]
    t.fill_(UNWRITTEN)
    w.fill_(UNWRITTEN)
    assert (t.data_ptr() % 16 == 0) == (misalign % 4 == 0)
    table = (ctypes.c_double * 27)(*np.stack([HOM[n] for n in SETS]).reshape(-1).tolist())
    rc = N.lib().pbr_rectify_images(src.data_ptr() + G, 3, Hs, Ws, 0, Ws * 3, 3, 1, table, t.data_ptr(), w.data_ptr(), H, width, S, clip, lin,
                                    torch.cuda.current_stream().cuda_stream)
    assert rc == N.OK
    torch.cuda.synchronize()
    for buf, view in ((tbuf, t), (wbuf, w)):
        lo = G + misalign
        assert (buf[:lo] == EDGE).all() and (buf[lo + view.numel():] == EDGE).all()          # canaries in front and behind
        assert not (view == UNWRITTEN).any() and not (view == EDGE).any() and torch.isfinite(view).all()   # every element written
    assert (src[:G] == 255).all() and (src[G + Hs * Ws * 3:] == 255).all()
    return t.view(3, 3, H, width).clone(), w.view(3, 1, H, width).clone()


@pytest.mark.parametrize("S", [1, 4])
def test_guard_bands_around_both_outputs(photo, S):
    quad = _guarded_call(36, S)                                      # the quad form
    for l, name in enumerate(SETS):
        held("guarded " + name, S, quad[0][l], quad[1][l], oracle(name, S))
    pixel = _guarded_call(36, S, misalign=1)                         # the same width off 16-byte alignment: the pixel form
    assert torch.equal(pixel[0], quad[0]) and torch.equal(pixel[1], quad[1])
    odd = _guarded_call(37, S)                                       # a width 4 does not divide: the pixel form
    assert torch.equal(odd[0][..., :36], quad[0]) and torch.equal(odd[1][..., :36], quad[1])
    via_python = capture.rectify(photo[None].expand(3, Hs, Ws, 3), np.stack([HOM[n] for n in SETS]), C.SIZE, supersample=S)
    assert torch.equal(via_python[0], quad[0]) and torch.equal(via_python[1], quad[1])


def test_guard_bands_with_clip_and_to_linear():
    a = _guarded_call(36, 2, clip=C.CLIP_LEVEL, lin=1)
    b = _guarded_call(37, 2, clip=C.CLIP_LEVEL, lin=1)
    assert torch.equal(b[0][..., :36], a[0]) and torch.equal(b[1][..., :36], a[1])


def test_two_calls_give_the_same_bits(photo):
    homs = np.stack([HOM[n] for n in SETS])
    images = photo[None].expand(3, Hs, Ws, 3)
    for kw in (dict(supersample=1), dict(supersample=4, clip_level=C.CLIP_LEVEL), dict(supersample=2, to_linear=True)):
        a, b = capture.rectify(images, homs, C.SIZE, **kw), capture.rectify(images, homs, C.SIZE, **kw)
        assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1])


def test_end_to_end_rectified_photographs_fit_like_their_own_samples():
    """cook_torrance_stack of a known material, encoded to uint8 with pack_image and pasted into a larger black photograph at an integer
    offset: rectify gives back pbr_unpack_image's floats of those samples and weights of exactly 1, so the stack loss and its map
    gradients equal, bit for bit, the call on the unpacked samples with all-ones weights."""
    g = torch.Generator().manual_seed(11)
    albedo, rough, metal = torch.rand(3, H, W, generator=g), torch.rand(1, H, W, generator=g) * 0.8 + 0.2, torch.rand(1, H, W, generator=g)
    nxy = (torch.rand(2, H, W, generator=g) - 0.5) * 0.6
    normal = torch.cat([nxy, torch.ones(1, H, W)], 0)
    normal = normal / normal.norm(dim=0, keepdim=True)
    known = [t.cuda() for t in (albedo, normal, rough, metal)]
    lights = torch.tensor([[0.2, 0.1, 0.9], [-0.3, 0.25, 0.7], [0.0, -0.4, 1.1]])
    kw = dict(view_dir=[0.0, 0.0, 1.0], light=lights, light_intensity=[1.5, 1.5, 1.5], light_type="point")
    stack = F.cook_torrance_stack(*known, **kw)                      # [L,3,H,W]
    L, oy, ox = stack.shape[0], 9, 13
    samples = torch.stack([F.pack_image(stack[l]) for l in range(L)])               # [L,H,W,3] uint8
    assert samples.dtype == torch.uint8 and int(samples.max()) > 50
    photos = torch.zeros((L, Hs, Ws, 3), dtype=torch.uint8, device="cuda")
    photos[:, oy:oy + H, ox:ox + W] = samples
    targets, weights = capture.rectify(photos, translation(ox, oy), C.SIZE)
    floats = torch.stack([_unpacked(samples[l]) for l in range(L)])
    ones = torch.ones((L, 1, H, W), device="cuda")
    assert torch.equal(targets, floats) and torch.equal(weights, ones)

    def step(t, w):
        maps = [m.clone().add_(0.05).clamp_(0.05, 0.95).requires_grad_(True) for m in (known[0], known[2], known[3])]
        loss = F.rendering_loss_mse_stack(maps[0], known[1], maps[1], maps[2], targets=t, weights=w, **kw)
        loss.backward()
        return loss.detach(), [m.grad for m in maps]
    loss_a, grads_a = step(targets, weights)
    loss_b, grads_b = step(floats, ones)
    assert torch.isfinite(loss_a) and float(loss_a) > 0
    assert torch.equal(loss_a, loss_b)
    for ga, gb in zip(grads_a, grads_b):
        assert ga is not None and torch.equal(ga, gb) and float(ga.abs().max()) > 0
