"""Material rotation on the GPU (csrc/rotation.hip, pypbr_amd/rotation.py): upstream's pad / torchvision rotate / centre crop /
rotate_normals chain as one index function per output pixel.

Forward values are COPIES, so the non-normal planes are compared bit for bit: against the real reference's outputs
(tests/golden/rotate.npz, tools/gen_rotate_golden.py) and, on more shapes, against the ATen restatement of the chain
(tools/rotate_oracle.py) run on the device.  The normal planes pass through rotate_normals' arithmetic and hold the normal operations'
1e-6.  Two correct fp32 implementations may round a coordinate that lies on a tie to either side: pixels in the tie band
(gen_rotate_golden.band: within 16 * 2^-24 * max(Hp, Wp) pixel of a half-integer) must hold one of the texels on either side of the tie
(gen_rotate_golden.candidates), every other pixel the very texel.  STRICT angles keep at most 1 % of their pixels in the band, TIE
angles at most 10 % (asserted by the generator and by tests/test_rotation_host.py).

Gradients of the non-normal planes are sums of grad_out values: with integer-valued grad_out every sum is exact, so they are compared
BIT-EQUAL with autograd through the device oracle.  torch.autograd.gradcheck does not apply: nearest sampling is piecewise constant in
the angle and a permutation-with-sums in the values, and gradcheck's finite differences of a bit copy are exact only by accident of the
step; the exact comparison above says more."""
import ctypes
import os
import random
import sys

import numpy as np
import pytest
import torch

from test_gpu_write_guards import Guards

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
import gen_rotate_golden as G  # noqa: E402
import rotate_oracle as O  # noqa: E402

pytestmark = pytest.mark.gpu

GOLD = np.load(os.path.join(ROOT, "tests", "golden", "rotate.npz"))
NORMAL_TOL = 1e-6                       # what tests/test_gpu_normal_ops.py holds the normal operations to
HALF_ULP = 2.0 ** -11                   # one fp16 ulp of a component in [0.5, 1]: fp16 storage of an fp32 result that is 1e-6 off


def _in(size):
    return {k: torch.from_numpy(GOLD["in__%s__%s" % (size, k)]) for k in G.MAPS}


def oracle_block(x, angle, expand, mode, nfp=None):
    """The restated chain over a (P,h,w) | (B,P,h,w) fp32 block on whatever device it has; planes nfp .. nfp + 2 are a normal map."""
    out = O.rotate_map(x, angle, expand, mode)
    if nfp is None:
        return out
    images = out if out.dim() == 4 else out[None]
    done = torch.stack([torch.cat([im[:nfp], O.rotate_normals(im[nfp:nfp + 3], angle), im[nfp + 3:]]) for im in images])
    return done if out.dim() == 4 else done[0]


def _gather(x, idx):
    """x (..., P, h, w) through an (H, W) map of source offsets (-1: fill)."""
    flat = torch.cat([x.reshape(x.shape[:-2] + (-1,)), torch.zeros(x.shape[:-2] + (1,), dtype=x.dtype)], dim=-1)
    return flat[..., torch.where(idx < 0, torch.full_like(idx, flat.shape[-1] - 1), idx)]


def check_forward(got, x, want, h, w, angle, expand, mode, nfp=None, normal_tol=NORMAL_TOL, tag=None):
    """got against want (the oracle's or the reference's result for x): outside the tie band bit-equal (normal planes within normal_tol),
    inside it the pixel holds one of the candidate texels on either side of the tie, all its planes the same one."""
    from pypbr_amd import functional as F
    plan = F.rotate_plan(h, w, angle, expand, mode)
    got, x, want = got.cpu(), x.cpu(), want.cpu()
    assert got.shape == want.shape and tuple(got.shape[-2:]) == (plan.H, plan.W), (tag, got.shape, want.shape)
    bx, by = G.band(plan)
    inband = bx | by
    P = got.shape[-3]
    plain = torch.tensor([nfp is None or not nfp <= p < nfp + 3 for p in range(P)])

    def matches(a, b):                                   # per pixel: every plane agrees
        ok = (a[..., plain, :, :] == b[..., plain, :, :]).all(dim=-3)
        if nfp is not None:
            ok &= ((a[..., ~plain, :, :].float() - b[..., ~plain, :, :].float()).abs() <= normal_tol).all(dim=-3)
        return ok
    ok = matches(got, want)
    assert bool(ok[..., ~inband].all()), (tag, "outside the tie band", int((~ok[..., ~inband]).sum()))
    if bool(inband.any()):
        for idx in G.candidates(plan):
            cand = _gather(x.float(), idx)
            if nfp is not None:
                cand = oracle_normals(cand, angle, nfp)
            ok |= matches(got, cand.to(got.dtype))
        assert bool(ok.all()), (tag, "inside the tie band", int((~ok).sum()))
    return float(inband.float().mean())


def oracle_normals(block, angle, nfp):
    images = block if block.dim() == 4 else block[None]
    done = torch.stack([torch.cat([im[:nfp], O.rotate_normals(im[nfp:nfp + 3], angle), im[nfp + 3:]]) for im in images])
    return done if block.dim() == 4 else done[0]


# ---- forward: the reference's outputs -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", [torch.float32, torch.float16])
def test_every_golden_case(dtype):
    from pypbr_amd import functional as F
    shares = []
    for name, (h, w, angle, expand, mode) in sorted(G.CASES.items()):
        ins = _in("%dx%d" % (h, w))
        x = torch.cat([ins[k] for k in G.MAPS]).to(dtype)                         # albedo 3, normal 3, roughness 1
        want = torch.cat([torch.from_numpy(GOLD["out__%s__%s" % (name, k)]) for k in G.MAPS])
        if dtype == torch.float16:                                                # fp16 storage: the chain on the rounded values (copies commute with it)
            want = oracle_block(x.float(), angle, expand, mode, nfp=3)
        got = F.rotate_maps(x.cuda(), angle, expand, mode, normal_first_plane=3)
        assert got.dtype == dtype and got.is_cuda
        tol = NORMAL_TOL if dtype == torch.float32 else NORMAL_TOL + HALF_ULP
        shares.append(check_forward(got, x, want.to(dtype) if dtype == torch.float16 else want, h, w, angle, expand, mode, nfp=3, normal_tol=tol,
                                    tag=(name, dtype)))
        band = torch.from_numpy(GOLD["band__" + name]).bool()
        assert tuple(band.shape) == tuple(got.shape[-2:])
    print("\n[golden] %d cases, tie-band share up to %.4f" % (len(shares), max(shares)))


def test_random_rotate_equals_the_reference_after_the_same_seed():
    from pypbr_amd import rotation as R
    from pypbr_amd.materials import BasecolorMetallicMaterial
    ins = _in("%dx%d" % G.RANDOM_SIZE)
    for seed in G.SEEDS:
        mat = BasecolorMetallicMaterial(**{k: v.cuda() for k, v in ins.items()})
        random.seed(seed)
        out = R.RandomRotate(*G.RANDOM_RANGE)(mat)
        assert out is not mat and all(torch.equal(mat._maps[k].cpu(), ins[k]) for k in ins)
        angle = float(GOLD["random__%d" % seed][0])
        got = torch.cat([out._maps[k] for k in G.MAPS])
        want = torch.cat([torch.from_numpy(GOLD["out__random%d__%s" % (seed, k)]) for k in G.MAPS])
        check_forward(got, torch.cat([ins[k] for k in G.MAPS]), want, *G.RANDOM_SIZE, angle, False, "constant", nfp=3, tag=("random", seed))


# ---- forward: the device oracle on the whole matrix -----------------------------------------------------------------------------------
@pytest.mark.parametrize("size", G.SIZES)
def test_forward_equals_the_device_oracle(size):
    """Every angle, both padding modes, expand on and off, fp32 and fp16; 13 x 9 as a batch of two."""
    from pypbr_amd import functional as F
    h, w = size
    g = torch.Generator().manual_seed(h * 100 + w)
    B = 2 if size == (13, 9) else 1
    n = torch.cat([torch.rand(B, 2, h, w, generator=g) * 2 - 1, torch.rand(B, 1, h, w, generator=g) + 0.2], dim=1)
    x = torch.cat([torch.rand(B, 2, h, w, generator=g), n / n.norm(dim=1, keepdim=True), torch.rand(B, 5, h, w, generator=g)], dim=1)   # 10 planes
    if B == 1:
        x = x[0]
    cases, worst = 0, {True: 0.0, False: 0.0}
    for hh, ww, angle, expand, mode, strict in G.matrix():
        if (hh, ww) != size:
            continue
        for dtype in (torch.float32, torch.float16):
            xd = x.to(dtype).cuda()
            want = oracle_block(xd.float(), angle, expand, mode, nfp=2)
            got = F.rotate_maps(xd, angle, expand, mode, normal_first_plane=2)
            tol = NORMAL_TOL if dtype == torch.float32 else NORMAL_TOL + HALF_ULP
            share = check_forward(got, xd, want.to(dtype), h, w, angle, expand, mode, nfp=2, normal_tol=tol, tag=(size, angle, expand, mode, dtype))
            worst[strict] = max(worst[strict], share)
            cases += 1
    assert cases >= 2 * 2 * len(G.STRICT)
    print("\n[%dx%d] %d cases; tie-band share: strict up to %.4f, tie up to %.4f" % (h, w, cases, worst[True], worst[False]))
    assert worst[True] <= G.STRICT_CAP and worst[False] <= G.TIE_CAP


@pytest.mark.parametrize("mode", G.MODES)
def test_blocks_of_10_and_32_planes_strided_and_unaligned(mode):
    """Source and destination blocks with plane strides larger than a plane, a batch stride likewise, and a destination one element off
    the 16-byte grid (the pixel-by-pixel store path at a width that is a multiple of four)."""
    from pypbr_amd import functional as F
    h, w, angle = 16, 24, 33.3
    plan = F.rotate_plan(h, w, angle, False, mode)
    g = torch.Generator().manual_seed(7)
    for P, nfp in ((10, 4), (32, 29), (32, None)):
        for B in (1, 2):
            for offset in (0, 1):
                big = torch.rand(B, P + 1, h * w + 5, generator=g).cuda()
                if nfp is not None:
                    big[:, nfp + 2] += 0.2
                src = big[:, :P, :h * w].view(B, P, h, w)                         # plane stride h w + 5, batch stride (P + 1) (h w + 5)
                pitch = plan.H * plan.W + 8
                room = torch.full((B * (P + 2) * pitch + 4,), float("nan"), device="cuda")
                dst = room[offset:offset + B * (P + 2) * pitch].view(B, P + 2, pitch)[:, :P, :plan.H * plan.W].view(B, P, plan.H, plan.W)
                assert (dst.data_ptr() % 16 == 0) == (offset == 0)
                out = F._rotate_raw(src, plan, -1 if nfp is None else nfp, out=dst)
                assert out.data_ptr() == dst.data_ptr()
                want = oracle_block(src.contiguous(), angle, False, mode, nfp=nfp)
                check_forward(dst, src, want, h, w, angle, False, mode, nfp=nfp, tag=(P, nfp, B, offset, mode))
                used = torch.zeros_like(room, dtype=torch.bool)
                used[offset:offset + B * (P + 2) * pitch].view(B, P + 2, pitch)[:, :P, :plan.H * plan.W] = True
                assert bool(torch.isnan(room[~used]).all()), ("written outside the destination planes", P, B, offset)


def test_four_quarter_turns_return_the_original_bits():
    from pypbr_amd import functional as F
    x = torch.rand(5, 32, 32, generator=torch.Generator().manual_seed(3)).cuda()
    for mode in G.MODES:
        y = x
        for _ in range(4):
            y = F.rotate_maps(y, 90.0, False, mode)
        assert torch.equal(y, x), mode
        assert torch.equal(F.rotate_maps(x, 90.0, False, mode), torch.rot90(x, 1, dims=(-2, -1))), mode      # counter-clockwise, as torchvision's


# ---- backward -------------------------------------------------------------------------------------------------------------------------
BACKWARD_SIZES = ((13, 9), (16, 24), (33, 47))


def _close(g, g64, what, rtol=2e-5):
    err = (g.detach().cpu().double() - g64.detach().cpu()).abs()
    ok = err <= rtol * (1 + g64.detach().cpu().abs())
    assert bool(ok.all()), (what, float(err.max()))


@pytest.mark.parametrize("size", BACKWARD_SIZES)
def test_gradients_are_bit_equal_to_the_device_oracle(size):
    """Integer-valued grad_out: every gradient is an exact sum, whatever its order.  Strict angles, both modes, expand on and off, a batch
    of two; a case with a pixel in the tie band is compared outside the preimages of those pixels only."""
    from pypbr_amd import functional as F
    h, w = size
    g = torch.Generator().manual_seed(h + w)
    cases, launches = 0, F.LAUNCHES["rotate_planes_backward"]
    for hh, ww, angle, expand, mode, strict in G.matrix():
        if (hh, ww) != size or not strict:
            continue
        plan = F.rotate_plan(h, w, angle, expand, mode)
        x = torch.rand(2, 4, h, w, generator=g).cuda().requires_grad_()
        xo = x.detach().clone().requires_grad_()
        go = torch.randint(-8, 9, (2, 4, plan.H, plan.W), generator=g).float().cuda()
        bx, by = G.band(plan)
        keep = (~(bx | by)).float().cuda()                                         # pixels on a tie may pick either texel: they send no gradient
        out = F.rotate_maps(x, angle, expand, mode)
        (out * go * keep).sum().backward()
        (O.rotate_map(xo, angle, expand, mode) * go * keep).sum().backward()
        assert x.grad.dtype == torch.float32 and x.grad.shape == x.shape
        assert torch.equal(x.grad, xo.grad), (size, angle, expand, mode, int((x.grad != xo.grad).sum()))
        assert float(x.grad.abs().max()) > 0
        cases += 1
    assert cases >= 2 * len(G.STRICT) and F.LAUNCHES["rotate_planes_backward"] - launches == cases


def test_backward_is_deterministic():
    from pypbr_amd import functional as F
    g = torch.Generator().manual_seed(11)
    x = torch.rand(2, 6, 16, 24, generator=g).cuda()
    go = torch.randn(2, 6, 16, 24, generator=g).cuda()
    grads = []
    for _ in range(2):
        xi = x.clone().requires_grad_()
        (F.rotate_maps(xi, 17.0, False, "circular", normal_first_plane=1) * go).sum().backward()       # circular: several preimages per texel
        grads.append(xi.grad)
    assert torch.equal(grads[0], grads[1])


@pytest.mark.parametrize("case", [((13, 9), 17.0, False, "constant"), ((16, 24), -71.5, False, "circular"), ((33, 47), 123.4, True, "constant"),
                                  ((16, 24), 90.0, True, "constant")], ids=str)
def test_normal_triple_gradient(case):
    """The normal map's planes inside a block: against float64 autograd through the oracle, within the band tests/test_gpu_normal_ops.py
    holds rotate_normals' gradient to (2e-5 (1 + |g|))."""
    from pypbr_amd import functional as F
    (h, w), angle, expand, mode = case
    plan = F.rotate_plan(h, w, angle, expand, mode)
    bx, by = G.band(plan)
    assert not bool((bx | by).any())                                               # no tie: fp32 and float64 pick the same texels
    g = torch.Generator().manual_seed(h)
    n = torch.cat([torch.rand(2, 2, h, w, generator=g) * 2 - 1, torch.rand(2, 1, h, w, generator=g) + 0.2], dim=1)
    x = torch.cat([torch.rand(2, 1, h, w, generator=g), n / n.norm(dim=1, keepdim=True), torch.rand(2, 2, h, w, generator=g)], dim=1)
    go = torch.randn(2, 6, plan.H, plan.W, generator=g)
    xd = x.cuda().requires_grad_()
    (F.rotate_maps(xd, angle, expand, mode, normal_first_plane=1) * go.cuda()).sum().backward()
    x64 = x.double().requires_grad_()
    idx = F.rotate_indices(plan)
    moved = _gather(x64, idx)                                                      # the index map as plain indexing: float64 values, the fp32 map
    (oracle_normals(moved, angle, 1) * go.double()).sum().backward()
    _close(xd.grad, x64.grad, case)
    assert float(xd.grad[:, 1:4].abs().max()) > 0


@pytest.mark.parametrize("size", [(13, 9), (5, 3), (16, 24)], ids=str)
@pytest.mark.parametrize("mode", G.MODES)
def test_guard_bands(size, mode):
    """Canaries around dst and grad_src, inputs untouched, every output element written: ragged widths (9, 3), and the last image of a
    batch (its planes end where the guard begins)."""
    from pypbr_amd import _native as N
    from pypbr_amd import functional as F
    lib = N.lib()
    s = torch.cuda.current_stream().cuda_stream
    h, w = size
    B, P, nfp = 2, 5, 1
    g = torch.Generator().manual_seed(h * w)
    for angle, expand in ((33.3, False), (123.4, True), (90.0, False)):
        try:
            plan = F.rotate_plan(h, w, angle, expand, mode)
        except ValueError:
            continue
        geom = F._rotate_geom(plan)
        x = torch.rand(B, P, h, w, generator=g)
        x[:, nfp + 2] += 0.2
        for dtype in (torch.float32, torch.float16):
            G_ = Guards()
            xi, out = G_.input(x.to(dtype)), G_.output((B, P, plan.H, plan.W), dtype)
            assert lib.pbr_rotate_planes(xi.data_ptr(), P * h * w, h * w, out.data_ptr(), P * plan.H * plan.W, plan.H * plan.W, B, P, h, w, plan.H,
                                         plan.W, ctypes.byref(geom), nfp, *plan.normal_matrix, N.F32 if dtype == torch.float32 else N.F16, s) == 0
            G_.check(("forward", size, mode, angle, expand, dtype))
            want = oracle_block(x.to(dtype).float().cuda(), angle, expand, mode, nfp=nfp).to(dtype)
            check_forward(out, x.to(dtype), want, h, w, angle, expand, mode, nfp=nfp, normal_tol=NORMAL_TOL if dtype == torch.float32 else NORMAL_TOL + HALF_ULP,
                          tag=("guard", size, mode, angle, expand, dtype))
        G_ = Guards()
        go = torch.randn(B, P, plan.H, plan.W, generator=g)
        gi_, xi, gs = G_.input(go), G_.input(x), G_.output((B, P, h, w))
        assert lib.pbr_rotate_planes_backward(gi_.data_ptr(), P * plan.H * plan.W, plan.H * plan.W, gs.data_ptr(), P * h * w, h * w, xi.data_ptr(),
                                              P * h * w, h * w, B, P, h, w, plan.H, plan.W, ctypes.byref(geom), nfp, *plan.normal_matrix, s) == 0
        G_.check(("backward", size, mode, angle, expand))
        bx, by = G.band(plan)
        if not bool((bx | by).any()):
            x64 = x.double().requires_grad_()
            (oracle_normals(_gather(x64, F.rotate_indices(plan)), angle, nfp) * go.double()).sum().backward()
            _close(gs, x64.grad, ("backward", size, mode, angle, expand))


# ---- material level -------------------------------------------------------------------------------------------------------------------
def _packed(seed, h, w, channels):
    g = torch.Generator().manual_seed(seed)
    t = torch.rand(channels, h, w, generator=g)
    n = torch.cat([torch.rand(2, h, w, generator=g) * 2 - 1, torch.rand(1, h, w, generator=g) + 0.2])
    t[3:6] = n / n.norm(dim=0, keepdim=True)
    return t


@pytest.mark.parametrize("workflow", ["metallic", "specular"])
def test_material_rotates_in_one_launch_and_equals_the_per_map_oracle(workflow):
    from pypbr_amd import functional as F, rotation as R
    from pypbr_amd.materials import BasecolorMetallicMaterial, DiffuseSpecularMaterial, NormalConvention
    if workflow == "metallic":
        cls, names = BasecolorMetallicMaterial, [("albedo", 3), ("normal", 3), ("roughness", 1), ("metallic", 1)]
    else:
        cls, names = DiffuseSpecularMaterial, [("albedo", 3), ("normal", 3), ("roughness", 1), ("specular", 3)]
    packed = _packed(21, 33, 47, sum(c for _, c in names))
    for angle, expand, mode in ((33.3, False, "constant"), (-71.5, True, "constant"), (17.0, False, "circular")):
        mat = cls.from_tensor(packed.cuda(), names, normal_convention=NormalConvention.DIRECTX)
        mat.albedo_is_srgb = False
        before = {k: v.clone() for k, v in mat._raw.items()}
        count = dict(F.LAUNCHES)
        assert R.rotate(mat, angle, expand=expand, padding_mode=mode) is mat
        assert F.LAUNCHES["rotate_planes"] - count["rotate_planes"] == 1, (workflow, angle)          # all planes of the one allocation
        assert F.LAUNCHES["rotate_planes_backward"] == count["rotate_planes_backward"]
        assert mat.albedo_is_srgb is False and mat.normal_convention == NormalConvention.DIRECTX
        plan = F.rotate_plan(33, 47, angle, expand, mode)
        assert mat.size == (plan.H, plan.W)
        for k, c in names:
            want = O.rotate_material_map(k, before[k], angle, expand, mode)
            check_forward(mat._maps[k], before[k], want, 33, 47, angle, expand, mode, nfp=0 if k == "normal" else None, tag=(workflow, k, angle))


def test_maps_of_two_sizes_and_loose_maps_get_one_launch_each():
    from pypbr_amd import functional as F, rotation as R
    from pypbr_amd.materials import BasecolorMetallicMaterial
    g = torch.Generator().manual_seed(5)
    maps = {"albedo": torch.rand(3, 16, 24, generator=g).cuda(), "roughness": torch.rand(1, 16, 24, generator=g).cuda(),
            "metallic": torch.rand(1, 13, 9, generator=g).cuda(), "height": torch.rand(1, 13, 9, generator=g).half().cuda()}
    mat = BasecolorMetallicMaterial(**maps)
    count = F.LAUNCHES["rotate_planes"]
    R.rotate(mat, 17.0)
    assert F.LAUNCHES["rotate_planes"] - count == 3                              # the 16 x 24 block, the 13 x 9 float32 map, the fp16 map
    for k, v in maps.items():
        want = O.rotate_map(v.float(), 17.0, False, "constant").to(v.dtype)
        check_forward(mat._maps[k], v, want, *v.shape[-2:], 17.0, False, "constant", tag=k)


def test_host_resident_material_and_pending_lazy_tile():
    from pypbr_amd import rotation as R
    from pypbr_amd.materials import BasecolorMetallicMaterial
    ins = _in("13x9")
    mat = BasecolorMetallicMaterial(**{k: v.clone() for k, v in ins.items()})            # on the host, handed out on the host
    R.rotate(mat, 33.3)
    for k in G.MAPS:
        got = mat._maps[k]
        assert got.device.type == "cpu"
        check_forward(got, ins[k], O.rotate_material_map(k, ins[k], 33.3), 13, 9, 33.3, False, "constant", nfp=0 if k == "normal" else None, tag=k)
    mat = BasecolorMetallicMaterial(**{k: v.cuda() for k, v in ins.items()})
    mat.tile(2)                                                                   # recorded, not carried out
    assert mat.lazy_tile == (2, 2)
    R.rotate(mat, 17.0)
    assert mat.lazy_tile == (1, 1) and mat.size == (26, 18)
    for k in ("albedo", "roughness"):
        tiled = ins[k].repeat(1, 2, 2)
        check_forward(mat._maps[k], tiled, O.rotate_map(tiled, 17.0), 26, 18, 17.0, False, "constant", tag=("tiled", k))


def test_compose_with_random_rotate_in_front_of_a_rendering_loss():
    """Compose([RandomCrop, RandomRotate, Tile]) in front of RenderingLoss: the loss's backward reaches a leaf albedo with the gradient
    the oracle's chain (slice, restated rotate, repeat) gives in front of the same loss."""
    from pypbr_amd import functional as F, rotation as R, transforms as T
    from pypbr_amd.losses import RenderingLoss
    from pypbr_amd.materials import BasecolorMetallicMaterial
    seed, span = 2, (10.0, 350.0)
    g = torch.Generator().manual_seed(9)
    n = torch.cat([torch.rand(2, 40, 40, generator=g) - 0.5, torch.ones(1, 40, 40)])
    maps = {"albedo": torch.rand(3, 40, 40, generator=g), "normal": n / n.norm(dim=0, keepdim=True),
            "roughness": torch.rand(1, 40, 40, generator=g) * 0.8 + 0.2, "metallic": torch.rand(1, 40, 40, generator=g)}
    target = torch.rand(3, 48, 48, generator=g).cuda()
    random.seed(seed)
    top, left = int(16 * random.random()), int(16 * random.random())              # RandomCrop's draws, then RandomRotate's
    angle = span[0] + (span[1] - span[0]) * random.random()
    bx, by = G.band(F.rotate_plan(24, 24, angle, False, "constant"))
    assert not bool((bx | by).any())                                               # seed 2 draws 29.2 degrees: no pixel on a tie

    mat = BasecolorMetallicMaterial(**{k: v.cuda() for k, v in maps.items()})
    albedo = mat._raw["albedo"].requires_grad_()
    random.seed(seed)
    count = dict(F.LAUNCHES)
    pred = T.Compose([T.RandomCrop(24, 24), R.RandomRotate(*span), T.Tile(2)])(mat)
    assert pred is not mat and pred.size == (48, 48) and mat.size == (40, 40)
    assert F.LAUNCHES["rotate_planes"] - count["rotate_planes"] == 2              # the leaf albedo on the differentiable path, the rest as one block
    RenderingLoss()(pred, target).backward()
    assert F.LAUNCHES["rotate_planes_backward"] - count["rotate_planes_backward"] == 1
    assert albedo.grad is not None and albedo.grad.shape == (3, 40, 40) and float(albedo.grad.abs().max()) > 0

    leaf = maps["albedo"].cuda().requires_grad_()
    chain = {k: O.rotate_material_map(k, (leaf if k == "albedo" else v.cuda())[:, top:top + 24, left:left + 24], angle).repeat(1, 2, 2)
             for k, v in maps.items()}
    RenderingLoss()(BasecolorMetallicMaterial(**chain), target).backward()
    _close(albedo.grad, leaf.grad.double(), "albedo gradient through crop, rotate, tile and the rendering loss")
    scale = float(leaf.grad.abs().max())
    assert float((albedo.grad - leaf.grad).abs().max()) <= 1e-4 * scale, scale     # the recorded tile sums its four repeats in another order: a few ulps
    for k in maps:                                                                # (after the loss: reading _maps carries the recorded tile out)
        got, want = pred._maps[k], chain[k].detach()
        assert got.shape == want.shape == (want.shape[0], 48, 48)
        assert float((got - want).abs().max()) <= NORMAL_TOL if k == "normal" else torch.equal(got, want), k
    outside = torch.ones(40, 40, dtype=torch.bool)
    outside[top:top + 24, left:left + 24] = False
    assert bool((albedo.grad[:, outside.cuda()] == 0).all())                      # texels outside the crop window receive exactly nothing
