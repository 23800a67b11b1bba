"""Normal -> height on the device (csrc/height_ops.hip around torch.fft.rfft2 / irfft2): every stage against its definition, the whole
against the real reference's float32 output and against float64 (tests/golden/height_ops.npz, height_ops_grad.npz, written by
tools/gen_height_golden.py), gradients against float64 autograd, batches, the material API, determinism and guard bands.

Bounds: 2e-6 against float64 forward (DESIGN 4's bound; upstream's own float32 output is up to 1.4e-5 from float64 on
these inputs, so it is the envelope, not the target); 2e-5 (1 + |g|) for gradients; 1e-5 relative for the Laplacian's eigenvalues
(the sin^2 form is a few ulp off, upstream's cos form 5 % at kx = 1, W = 4096)."""
import math
import os

import numpy as np
import pytest
import torch

from test_gpu_write_guards import Guards

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = np.load(os.path.join(ROOT, "tests", "golden", "height_ops.npz"))
GRAD = np.load(os.path.join(ROOT, "tests", "golden", "height_ops_grad.npz"))
CASES = sorted(k[len("ref64__"):] for k in GOLD.files if k.startswith("ref64__"))
GRAD_CASES = sorted(k[len("g64__"):] for k in GRAD.files if k.startswith("g64__"))
SMALL = 64 * 64                     # "the shapes up to 64 x 64"


def _case(key):
    name, scale, conv = key.split("__")
    return torch.from_numpy(GOLD["in__" + name].copy()), float(scale), conv


def _t(z, key):
    return torch.from_numpy(z[key].copy())


def ref_div(n, scale, directx):
    """functions.py:205-228, 250-283 restated in float32 ATen calls ((.., 3, H, W) -> (.., H, W)): elementwise IEEE operations in
    upstream's order, so bit-equal to upstream's div_g -- test_divergence_is_bit_equal_on_every_case pins that on the golden file."""
    nz = n[..., 2, :, :] + 1e-8
    gx = -n[..., 0, :, :] / nz
    gy = n[..., 1, :, :] / nz if directx else -n[..., 1, :, :] / nz
    gx, gy = gx * scale, gy * scale
    dgx = torch.cat([gx[..., :, 1:], gx[..., :, -1:]], -1) - gx
    dgy = torch.cat([gy[..., 1:, :], gy[..., -1:, :]], -2) - gy
    return dgx + dgy


def den64(H, W, cols=None):
    """-4 (sin^2(pi kx / W) + sin^2(pi ky / H)) on the full grid (or its first `cols` columns), float64 numpy."""
    ky, kx = np.arange(H, dtype=np.float64)[:, None], np.arange(W if cols is None else cols, dtype=np.float64)[None, :]
    return -4.0 * (np.sin(np.pi * kx / W) ** 2 + np.sin(np.pi * ky / H) ** 2)


def height64(n, scale, directx):
    """The whole definition in float64 numpy, from the formulas of the stages: (3, H, W) -> (1, H, W)."""
    n = n.numpy().astype(np.float64)
    ze = n[2] + 1e-8
    gx, gy = -n[0] / ze * scale, (n[1] if directx else -n[1]) / ze * scale
    div = (np.concatenate([gx[:, 1:], gx[:, -1:]], 1) - gx) + (np.concatenate([gy[1:], gy[-1:]], 0) - gy)
    den = den64(*div.shape)
    den[0, 0] = 1.0
    spec = np.fft.fft2(div) / den
    spec[0, 0] = 0.0
    h = np.fft.ifft2(spec).real
    h = h - h.mean()
    return ((h - h.min()) / (h.max() - h.min() + 1e-8))[None]


def unit_normals(shape, seed, zmin=0.3):
    g = torch.Generator().manual_seed(seed)
    z = zmin + (1.0 - zmin) * torch.rand(*shape[:-3], 1, *shape[-2:], generator=g)
    phi = 2.0 * math.pi * torch.rand(*shape[:-3], 1, *shape[-2:], generator=g)
    r = torch.sqrt(1.0 - z * z)
    return torch.cat([r * torch.cos(phi), r * torch.sin(phi), z], -3)


def _close(g, g64, what, extra=None, rtol=2e-5):
    g, g64 = g.detach().cpu().double(), g64.detach().cpu().double()
    err, bound = (g - g64).abs(), rtol * (1 + g64.abs())
    if extra is not None:
        bound = bound + extra.detach().cpu().double()
    print("%s: max |g - g64| %.3e, worst error / bound %.3f" % (what, float(err.max()), float((err / bound).max())))
    assert bool((err <= bound).all()), (what, float(err.max()), float((err / bound).max()))


def _stream():
    return torch.cuda.current_stream().cuda_stream


# ---- stage 1: the divergence ----------------------------------------------------------------------------------------------------------
def test_divergence_is_bit_equal_on_every_case():
    from pypbr_amd import _height_ops as HO
    for key in CASES:
        n, scale, conv = _case(key)
        want = _t(GOLD, "div__" + key)
        assert torch.equal(ref_div(n, scale, conv == "directx"), want), ("the restatement", key)
        got = HO._divergence_raw(n[None].cuda(), scale, conv == "directx")[0].cpu()
        assert torch.equal(got, want), (key, float((got - want).abs().max()))


def test_divergence_fp16_storage_strided_planes_and_a_batch():
    from pypbr_amd import _height_ops as HO, _native as N
    a, b = _case("n37x53__1__opengl")[0], _case("n37x53__2.5__directx")[0].flip(-1)
    pair = torch.stack([a, b])                                                   # two different images
    assert not torch.equal(a, b)
    for directx in (False, True):
        got = HO._divergence_raw(pair.cuda(), 2.5, directx).cpu()
        assert torch.equal(got, ref_div(pair, 2.5, directx)), directx
        half = pair.half()
        got = HO._divergence_raw(half.cuda(), 2.5, directx).cpu()
        assert torch.equal(got, ref_div(half.float(), 2.5, directx)), ("fp16: the oracle on the exact up-casts", directx)
    # a strided block: planes 11 elements further apart than H W, images 7 further than 3 planes, the divergence's images 5 apart
    B, H, W = 2, 37, 53
    ps, bs, ds = H * W + 11, 3 * (H * W + 11) + 7, H * W + 5
    block = torch.full((B * bs,), float("nan"))
    for i in range(B):
        for c in range(3):
            block[i * bs + c * ps:i * bs + c * ps + H * W] = pair[i, c].reshape(-1)
    block, div = block.cuda(), torch.full((B * ds,), 7.0, device="cuda")
    assert N.lib().pbr_normal_divergence(block.data_ptr(), bs, ps, div.data_ptr(), ds, B, H, W, 1.0, 0, N.F32, _stream()) == 0
    div = div.cpu()
    want = ref_div(pair, 1.0, False)
    for i in range(B):
        assert torch.equal(div[i * ds:i * ds + H * W].view(H, W), want[i]), i
        assert bool((div[i * ds + H * W:(i + 1) * ds] == 7.0).all())


def test_divergence_has_no_clamps():
    """n_z = -1e-8 makes zeps 0: +-inf in g, and inf - inf = NaN across the replicated edge -- where upstream's are."""
    from pypbr_amd import _height_ops as HO
    n = unit_normals((3, 6, 9), 5)
    n[2, 2, 3], n[2, 5, 8], n[0, 0, 0] = -1e-8, -1e-8, float("nan")
    want = ref_div(n, 1.5, False)
    assert bool(torch.isnan(want).any()) and bool(torch.isinf(want).any())
    got = HO._divergence_raw(n[None].cuda(), 1.5, False)[0].cpu()
    assert torch.equal(torch.nan_to_num(got, 123.0), torch.nan_to_num(want, 123.0))
    assert torch.equal(torch.isnan(got), torch.isnan(want))


# ---- stage 2: the eigenvalues ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("B,H,W", [(1, 4096, 4096), (2, 37, 53), (1, 1, 17), (1, 5, 1)])
def test_poisson_scale_denominators_track_float64(B, H, W):
    """A spectrum of (1 + 2i): the quotient gives every denominator back.  Relative 1e-5 against float64 on EVERY bin -- the low bins
    (kx, ky <= 8 and their mirror rows), where the cos form cancels, are reported separately -- and the DC bin exactly 0."""
    from pypbr_amd import _height_ops as HO
    Wh = W // 2 + 1
    spec = torch.full((B, H, Wh), 1.0 + 2.0j, dtype=torch.complex64, device="cuda")
    out = HO._poisson_scale_raw(spec, W)
    assert out.data_ptr() == spec.data_ptr()
    got = torch.view_as_real(out).cpu().double()
    want = torch.from_numpy(den64(H, W, Wh))
    for b in range(B):
        assert float(got[b, 0, 0].abs().max()) == 0.0
        for part, num in ((0, 1.0), (1, 2.0)):
            den = num / got[b, :, :, part]
            rel = ((den - want) / want).abs()
            rel[0, 0] = 0.0
            low = torch.cat([rel[:9, :9], rel[-8:, :9]]) if H > 16 and Wh > 9 else rel
            print("%dx%d image %d part %d: max relative error of den %.2e (low bins %.2e)" % (H, W, b, part, float(rel.max()), float(low.max())))
            assert float(rel.max()) <= 1e-5, (b, part, float(rel.max()))
    if W == 4096:       # what the bound separates: upstream's float32 cos form at kx = 1 is several per cent off
        x = torch.tensor(2 * math.pi / W, dtype=torch.float32)
        cos_form = float((2 * torch.cos(x) - 2).double())
        assert abs(cos_form / float(want[0, 1]) - 1) > 1e-3


# ---- forward parity -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("key", CASES)         # (a case each: the first transform of a new shape builds the FFT library's plan, 0.5 - 1.5 s)
def test_forward_against_float64_and_upstream(key):
    """Measured on an MI355X: max |hip - ref64| 9.4e-7 over all cases (37 x 53), 7.6e-7 on 72 x 200 where upstream's own float32 output
    is 1.4e-5 from float64."""
    from pypbr_amd import functional as F
    n, scale, conv = _case(key)
    ref32, ref64 = _t(GOLD, "ref32__" + key).double(), _t(GOLD, "ref64__" + key)
    got = F.height_from_normal(n.cuda(), scale, conv)
    assert got.shape == (1,) + tuple(n.shape[1:]) and got.dtype == torch.float32 and got.is_cuda
    got = got.cpu().double()
    e64, e32, envelope = (got - ref64).abs(), (got - ref32).abs(), (ref32 - ref64).abs()
    print("%-24s |hip - ref64| %.2e  |hip - ref32| %.2e  |ref32 - ref64| %.2e" % (key, float(e64.max()), float(e32.max()), float(envelope.max())))
    assert float(e64.max()) <= 2e-6, (key, float(e64.max()))
    assert bool((e32 <= envelope + 1e-5).all()), (key, float((e32 - envelope).max()))
    if n.shape[1] * n.shape[2] <= SMALL:
        assert float(e32.max()) <= 1e-5, (key, float(e32.max()))
    if got.numel() > 1:
        assert float(got.min()) == 0.0 and abs(float(got.max()) - 1.0) <= 1e-6


def test_multi_workgroup_paths_512():
    """512 x 512: 22 partials per image in stages 3 to 5, the last one ragged (4096 of 12288 pixels); forward against the float64
    evaluation, the normalisation's backward against float64 autograd of its formula on the same height map.  Measured on an MI355X:
    max |hip - float64| 1.10e-6 (above 1e-6; the gate stays DESIGN 4's 2e-6)."""
    from pypbr_amd import _height_ops as HO, _native as N, functional as F
    H = W = 512
    assert N.lib().pbr_height_workspace_bytes(1, H, W) == 22 * 24 and (H * W) % 12288 != 0
    n = unit_normals((3, H, W), 512)
    want = torch.from_numpy(height64(n, 1.0, False))
    got = F.height_from_normal(n.cuda(), 1.0, "opengl").cpu().double()
    err = float((got - want).abs().max())
    print("512 x 512: max |hip - float64| = %.3e" % err)
    assert err <= 2e-6, err
    g = torch.Generator().manual_seed(3)
    h, G = torch.rand(1, H, W, generator=g), torch.randn(1, 1, H, W, generator=g)
    _normalize_backward_case(HO, h, G, "512 x 512")


# ---- batches, determinism, staging, fp16 ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", [(37, 53), (64, 64), (256, 200)])
def test_a_batch_equals_its_single_calls_bit_for_bit(shape):
    from pypbr_amd import functional as F
    n = unit_normals((2, 3) + shape, 11).cuda()
    both = F.height_from_normal(n, 2.5, "directx")
    assert both.shape == (2, 1) + shape
    for b in range(2):
        assert torch.equal(both[b], F.height_from_normal(n[b], 2.5, "directx")), b
    assert not torch.equal(both[0], both[1])
    n.requires_grad_()
    G = torch.randn(both.shape, generator=torch.Generator().manual_seed(1)).cuda()
    (F.height_from_normal(n, 2.5, "directx") * G).sum().backward()
    for b in range(2):
        m = n[b].detach().clone().requires_grad_()
        (F.height_from_normal(m, 2.5, "directx") * G[b]).sum().backward()
        assert torch.equal(n.grad[b], m.grad), b


def test_two_runs_give_identical_bits():
    from pypbr_amd import functional as F
    n = unit_normals((3, 256, 200), 21).cuda()                                   # five partials per reduction
    G = torch.randn(1, 256, 200, generator=torch.Generator().manual_seed(2)).cuda()
    runs = []
    for _ in range(2):
        m = n.clone().requires_grad_()
        out = F.height_from_normal(m, 1.0)
        (out * G).sum().backward()
        runs.append((out.detach(), m.grad))
    assert torch.equal(runs[0][0], runs[1][0]) and torch.equal(runs[0][1], runs[1][1])


def test_cpu_tensors_are_staged_and_fp16_is_storage_only():
    from pypbr_amd import functional as F
    n = _case("n37x53__1__opengl")[0]
    on_device = F.height_from_normal(n.cuda(), 1.0)
    staged = F.height_from_normal(n, 1.0)
    assert staged.device.type == "cpu" and torch.equal(staged, on_device.cpu())
    m = n.clone().requires_grad_()
    F.height_from_normal(m, 1.0).square().sum().backward()
    assert m.grad is not None and m.grad.device.type == "cpu" and bool(torch.isfinite(m.grad).all())
    half = F.height_from_normal(n.half().cuda(), 1.0)
    assert half.dtype == torch.float16
    want = F.height_from_normal(n.half().float().cuda(), 1.0)                    # fp32 everywhere between the two storages
    assert torch.equal(half, want.half())
    with pytest.raises(NotImplementedError):
        F.height_from_normal(n.half().cuda().requires_grad_(), 1.0)


def test_flat_and_single_pixel_maps_give_exact_zeros_and_finite_gradients():
    from pypbr_amd import functional as F
    for shape in ((3, 64, 64), (3, 1, 1), (3, 37, 53)):
        n = torch.zeros(shape)
        n[2] = 1.0
        n = n.cuda().requires_grad_()
        out = F.height_from_normal(n, 2.0)
        assert torch.equal(out, torch.zeros_like(out)), shape
        (out * torch.randn(out.shape, generator=torch.Generator().manual_seed(4)).cuda()).sum().backward()
        assert bool(torch.isfinite(n.grad).all()), shape


# ---- gradients ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("key", GRAD_CASES)
def test_gradients_against_float64_autograd(key):
    """Measured on an MI355X: the worst error / bound is 0.25 (72 x 200, the one case under the envelope form), 0.10 on every other case
    (the 96 x 96 crop of `tiles` 0.02)."""
    from pypbr_amd import functional as F
    assert len(GRAD_CASES) == 8
    n, scale, conv = _case(key)
    G, g32, g64 = _t(GRAD, "G__" + key), _t(GRAD, "g32__" + key), _t(GRAD, "g64__" + key)
    m = n.cuda().requires_grad_()
    (F.height_from_normal(m, scale, conv) * G.cuda()).sum().backward()
    # at 72 x 200 upstream's own float32 gradient is up to 8e-4 from float64: it is the envelope there, and only there
    envelope = key.startswith("n72x200")
    _close(m.grad, g64, key, extra=(g32.double() - g64.double()).abs() if envelope else None)


def _normalize_backward_case(HO, h, G, what):
    """Stage 5 against float64 autograd of stage 4's formula (the mean subtraction included: its adjoint vanishes)."""
    hd = h.cuda().contiguous()
    out, stats = HO._normalize_raw(hd, torch.float32)
    x = h.double().requires_grad_()
    flat = x.reshape(x.shape[0], -1)
    hc = flat - flat.mean(1, keepdim=True)
    mn, mx = hc.min(1, keepdim=True).values, hc.max(1, keepdim=True).values
    ref = (hc - mn) / ((mx - mn) + 1e-8)
    assert float((out.cpu().double().reshape(ref.shape) - ref.detach()).abs().max()) <= 2e-6
    idx = stats[:, 3:].contiguous().view(torch.int32).cpu()
    assert torch.equal(idx[:, 0].long(), flat.argmin(1)) and torch.equal(idx[:, 1].long(), flat.argmax(1))
    (ref * G.double().reshape(ref.shape)).sum().backward()
    dh = HO._normalize_backward_raw(G.cuda().contiguous(), out, stats)
    _close(dh, x.grad, "normalize backward, " + what)


def test_normalize_backward_against_float64_autograd_of_its_formula():
    from pypbr_amd import _height_ops as HO
    g = torch.Generator().manual_seed(8)
    for B, H, W in ((1, 1, 1), (2, 37, 53), (2, 256, 200), (1, 5, 1)):           # 256 x 200: five partials, the last ragged
        h = torch.rand(B, H, W, generator=g) * 3.0 - 1.0
        _normalize_backward_case(HO, h, torch.randn(B, 1, H, W, generator=g), "%d x %d x %d" % (B, H, W))


def test_ties_give_the_gradient_to_the_first_extremum():
    """The stated difference from upstream: two equal minima, two equal maxima -- the first of each takes the gradient."""
    from pypbr_amd import _height_ops as HO
    h = torch.tensor([[[0.5, 0.0, 0.25, 0.0], [1.0, 0.75, 1.0, 0.5]]])
    out, stats = HO._normalize_raw(h.cuda(), torch.float32)
    idx = stats[:, 3:].contiguous().view(torch.int32).cpu()
    assert idx.tolist() == [[1, 4]]
    G = torch.arange(1.0, 9.0).view(1, 1, 2, 4)
    dh = HO._normalize_backward_raw(G.cuda(), out, stats).cpu().double()
    r = float(stats[0, 2])
    q, s = float((G.double() * out.cpu().double()).sum()) / r, float(G.sum()) / r
    want = G.double().view(1, 2, 4) / r
    want[0, 0, 1] += q - s
    want[0, 1, 0] -= q
    assert float((dh - want).abs().max()) <= 1e-5 and abs(float(dh.sum())) <= 1e-4


def test_divergence_backward_against_float64_autograd_of_its_formula():
    from pypbr_amd import _height_ops as HO
    g = torch.Generator().manual_seed(9)
    for shape, scale, directx in (((1, 3, 37, 53), 1.0, False), ((2, 3, 37, 53), 2.5, True), ((1, 3, 5, 1), 2.5, False),
                                  ((1, 3, 1, 17), 1.0, True), ((1, 3, 1, 1), 1.0, False), ((1, 3, 70, 130), 1.0, False)):
        n = unit_normals(shape, 100 + shape[-1])
        dd = torch.randn(shape[0], *shape[-2:], generator=g)
        x = n.double().requires_grad_()
        (ref_div(x, scale, directx) * dd.double()).sum().backward()
        got = HO._divergence_backward_raw(n.cuda(), dd.cuda(), scale, directx)
        _close(got, x.grad, "divergence backward %s" % (shape,))


# ---- the material API -----------------------------------------------------------------------------------------------------------------
def _tiles_without_height(golden):
    from pypbr_amd.materials import BasecolorMetallicMaterial
    z = golden("blend")
    mats = []
    for i in (1, 2):
        m = BasecolorMetallicMaterial(device=torch.device("cuda"))
        for key in z:
            if key.startswith("in_m%d_" % i) and not (i == 1 and key.endswith("_height")):
                m._maps[key[len("in_m%d_" % i):]] = torch.from_numpy(z[key]).cuda()
        mats.append(m)
    return mats, z


def test_a_material_without_a_height_map_gets_one_and_height_blends(golden):
    import pypbr_amd.blending as B
    (m1, m2), z = _tiles_without_height(golden)
    assert m1._raw.get("height") is None
    with pytest.raises(ValueError, match="height maps"):
        B.HeightBlend(blend_width=0.1, shift=-0.5)(m1, m2)
    assert m1.compute_height_from_normal(2.0) is m1
    h = m1._raw["height"]
    assert h.shape == (1, 96, 96) and h.is_cuda and h.dtype == torch.float32
    want = height64(torch.from_numpy(z["in_m1_normal"]), 2.0, False)
    assert float((h.cpu().double() - torch.from_numpy(want)).abs().max()) <= 2e-6
    assert torch.equal(m1._maps["height"], h)
    blended, mask = B.HeightBlend(blend_width=0.1, shift=-0.5)(m1, m2)
    assert type(blended) is type(m1) and mask.shape == (1, 96, 96) and bool(torch.isfinite(mask).all())
    assert 0.0 <= float(mask.min()) < float(mask.max()) <= 1.0
    assert blended._maps.get("height") is not None
    m1.normal_convention = "directx"                                            # the material's convention is the solve's
    m1.compute_height_from_normal(2.0)
    want = height64(torch.from_numpy(z["in_m1_normal"]), 2.0, True)
    assert float((m1._raw["height"].cpu().double() - torch.from_numpy(want)).abs().max()) <= 2e-6


def test_a_normal_map_that_requires_grad_is_fitted_under_a_height_loss(golden):
    from pypbr_amd.materials import BasecolorMetallicMaterial
    n = unit_normals((3, 37, 53), 31)
    target = torch.from_numpy(height64(unit_normals((3, 37, 53), 32), 1.5, False)).float().cuda()
    nd = n.cuda().requires_grad_()
    mat = BasecolorMetallicMaterial(albedo=torch.rand(3, 37, 53).cuda(), roughness=torch.rand(1, 37, 53).cuda(), metallic=torch.rand(1, 37, 53).cuda())
    mat._maps["normal"] = nd                                                    # as it is: an assignment would decode and renormalise it
    mat.compute_height_from_normal(1.5)
    loss = (mat._raw["height"] - target).square().mean()
    loss.backward()
    x = n.double().requires_grad_()
    hx = _height64_torch(x, 1.5, False)
    ((hx - target.cpu().double()).square().mean()).backward()
    assert nd.grad is not None and float(nd.grad.abs().max()) > 0
    _close(nd.grad, x.grad, "material, height loss")


def _height64_torch(n, scale, directx):
    """height64 in float64 torch (differentiable)."""
    div = ref_div(n, scale, directx)
    H, W = div.shape[-2:]
    den = torch.from_numpy(den64(H, W))
    den[0, 0] = 1.0
    keep = torch.ones(H, W, dtype=torch.float64)
    keep[0, 0] = 0.0
    h = torch.fft.ifft2(torch.fft.fft2(div) / den * keep).real
    h = h - h.mean()
    return ((h - h.min()) / (h.max() - h.min() + 1e-8))[None]


# ---- guard bands ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("H,W", [(19, 1), (19, 3), (19, 4), (19, 53), (20, 64), (19, 65), (19, 260), (1, 17), (200, 256)])
@pytest.mark.parametrize("dtype", [torch.float32, torch.float16])
def test_guard_bands(H, W, dtype):
    """Every stage with NaN margins around its inputs and sentinels around div, the spectrum, the workspace, stats, out, dh and
    grad_normal: nothing outside is written, every value inside is."""
    from pypbr_amd import _native as N
    lib, s = N.lib(), _stream()
    B, P, Wh = 2, H * W, W // 2 + 1
    code = N.F32 if dtype == torch.float32 else N.F16
    n = unit_normals((B, 3, H, W), 1000 + W).to(dtype)
    gen = torch.Generator().manual_seed(W)
    G = Guards()
    ni, div = G.input(n), G.output((B, H, W))
    assert lib.pbr_normal_divergence(ni.data_ptr(), 3 * P, P, div.data_ptr(), P, B, H, W, 2.0, 0, code, s) == 0
    spec = G.output((B, H, Wh, 2), init=torch.randn(B, H, Wh, 2, generator=gen))
    assert lib.pbr_poisson_scale(spec.data_ptr(), H * Wh, B, H, W, s) == 0
    h = G.input(torch.rand(B, H, W, generator=gen))
    nbytes = lib.pbr_height_workspace_bytes(B, H, W)
    ws, out, stats = G.workspace(nbytes), G.output((B, 1, H, W), dtype), G.output((B, 5))
    assert lib.pbr_height_stats(h.data_ptr(), P, ws.data_ptr(), B, H, W, s) == 0
    assert lib.pbr_height_normalize(h.data_ptr(), P, ws.data_ptr(), out.data_ptr(), P, stats.data_ptr(), B, H, W, code, s) == 0
    G.check(("forward", H, W, dtype))
    assert torch.equal(div.cpu(), ref_div(n.float(), 2.0, False))
    assert float(out.float().min()) == 0.0 and abs(float(out.float().max()) - 1.0) <= 1e-3
    if dtype != torch.float32:
        return
    out, stats = out.clone(), stats.clone()                      # (the indices in stats are small int32 bit patterns: denormals as floats)
    G = Guards()
    go, oi, si = G.input(torch.randn(B, 1, H, W, generator=gen)), G.input(out), G.input(stats)
    ws, dh = G.workspace(nbytes), G.output((B, H, W))
    assert lib.pbr_height_normalize_backward(go.data_ptr(), P, oi.data_ptr(), P, si.data_ptr(), ws.data_ptr(), dh.data_ptr(), P, B, H, W, s) == 0
    ni, dd, gn = G.input(n), G.input(torch.randn(B, H, W, generator=gen)), G.output((B, 3, H, W))
    assert lib.pbr_normal_divergence_backward(ni.data_ptr(), 3 * P, P, dd.data_ptr(), P, gn.data_ptr(), 3 * P, P, B, H, W, 2.0, 1, s) == 0
    G.check(("backward", H, W))
