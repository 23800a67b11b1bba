"""The normal-map operations on the device (csrc/normal_ops.hip): parity with the real reference (tests/golden/normal_ops.npz, written by
tools/gen_normal_golden.py), with an fp32 and a float64 restatement, gradients against float64 autograd, the material API, batches,
guard bands, 64-bit offsets, fp16 storage and the torch operators."""
import math
import os

import numpy as np
import pytest
import torch
import torch.nn.functional as TF

import torch_oracle as O
from test_gpu_write_guards import Guards

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = np.load(os.path.join(ROOT, "tests", "golden", "normal_ops.npz"))


def ref_height(h, scale, directx, dtype=torch.float64):
    """functions.py:146-175 restated: (.., 1, H, W) -> (.., 3, H, W)."""
    h = h.to(dtype)
    gx = TF.pad(h, (1, 0, 0, 0))[..., :, :-1] - TF.pad(h, (0, 1, 0, 0))[..., :, 1:]
    gy = TF.pad(h, (0, 0, 1, 0))[..., :-1, :] - TF.pad(h, (0, 0, 0, 1))[..., 1:, :]
    gx, gy = gx * scale, gy * scale
    b = gy if directx else -gy
    return TF.normalize(torch.cat([-gx, b, torch.ones_like(h)], dim=-3), dim=-3)


def ref_transform(n, m, renorm, dtype=torch.float64):
    n = n.to(dtype)
    x = m[0][0] * n[..., 0:1, :, :] + m[0][1] * n[..., 1:2, :, :]
    y = m[1][0] * n[..., 0:1, :, :] + m[1][1] * n[..., 1:2, :, :]
    v = torch.cat([x, y, n[..., 2:3, :, :]], dim=-3)
    return TF.normalize(v, dim=-3) if renorm else v


def _close(g, g64, what, rtol=2e-5):
    err = (g.detach().cpu().double() - g64.detach().cpu()).abs()
    ok = err <= rtol * (1 + g64.detach().cpu().abs())
    assert bool(ok.all()), (what, float(err.max()))


def _t(key):
    return torch.from_numpy(GOLD[key].copy())


def _rot(a):
    th = math.radians(a)
    return ((math.cos(th), -math.sin(th)), (math.sin(th), math.cos(th)))


# ---- parity ---------------------------------------------------------------------------------------------------------------------------
def test_every_golden_case():
    from pypbr_amd import functional as F, utils
    seen = 0
    for key in GOLD.files:
        kind, *rest = key.split("__")
        if kind == "cnfh":
            name, s, conv = rest
            got = F.normal_from_height(_t("in_height_" + name).cuda(), float(s), conv)
        elif kind == "rot":
            name, a = rest
            got = utils.rotate_normals(_t("in_normal_" + name).cuda(), float(a))
        elif kind == "str":
            name, f = rest
            f = float(f)
            got = F.transform_normals(_t("in_normal_" + name).cuda(), ((f, 0.0), (0.0, f)), True)
        elif kind == "inv":
            got = utils.invert_normal(_t("in_normal_" + rest[0]).cuda())
            assert torch.equal(got.cpu(), _t(key)), key
            seen += 1
            continue
        else:
            continue
        want = _t(key)
        assert got.shape == want.shape, key
        assert float((got.cpu() - want).abs().max()) <= 1e-6, (key, float((got.cpu() - want).abs().max()))
        seen += 1
    assert seen >= 60


@pytest.mark.parametrize("hw", [(4096, 4096), (33, 37), (7, 130), (1, 5), (65, 258), (3, 1023)])
@pytest.mark.parametrize("directx", [False, True])
def test_large_and_ragged_against_restatements(hw, directx):
    from pypbr_amd import functional as F
    g = torch.Generator().manual_seed(hw[0] * 7 + hw[1])
    h = torch.rand(1, *hw, generator=g)
    scale = 3.0
    got = F.normal_from_height(h.cuda(), scale, "directx" if directx else "opengl").cpu()
    assert float((got - ref_height(h, scale, directx, torch.float32)).abs().max()) <= 1e-6
    assert float((got.double() - ref_height(h, scale, directx)).abs().max()) <= 5e-7


def test_nan_masks_match_upstream():
    from pypbr_amd import functional as F
    g = torch.Generator().manual_seed(5)
    h = torch.rand(1, 40, 52, generator=g)
    h[0, 0, 0] = h[0, 17, 23] = h[0, 39, 51] = h[0, 5, 51] = float("nan")
    got = F.normal_from_height(h.cuda(), 2.0).cpu()
    assert torch.equal(torch.isnan(got), torch.isnan(ref_height(h, 2.0, False, torch.float32)))
    n = torch.rand(3, 9, 11, generator=g) - 0.5
    n[1, 4, 4] = float("nan")
    got = F.transform_normals(n.cuda(), _rot(30), True).cpu()
    assert torch.equal(torch.isnan(got), torch.isnan(ref_transform(n, _rot(30), True, torch.float32)))


# ---- gradients ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("hw", [(37, 53), (64, 64), (5, 1), (1, 9), (70, 260)])
@pytest.mark.parametrize("directx", [False, True])
def test_height_gradient(hw, directx):
    from pypbr_amd import functional as F
    g = torch.Generator().manual_seed(hw[0] + 100 * hw[1])
    h = torch.rand(1, *hw, generator=g)
    w = torch.randn(3, *hw, generator=g)
    hd = h.cuda().requires_grad_()
    (F.normal_from_height(hd, 2.5, "directx" if directx else "opengl") * w.cuda()).sum().backward()
    h64 = h.double().requires_grad_()
    (ref_height(h64, 2.5, directx) * w.double()).sum().backward()
    _close(hd.grad, h64.grad, "g_h")


@pytest.mark.parametrize("hw", [(37, 53), (40, 64), (6, 1)])
def test_height_gradient_of_a_batch(hw):
    """[B,1,H,W]: batch offsets and each image's own zero padding in the backward, image by image against float64."""
    from pypbr_amd import functional as F
    g = torch.Generator().manual_seed(17 * hw[0] + hw[1])
    h = torch.rand(3, 1, *hw, generator=g)
    w = torch.randn(3, 3, *hw, generator=g)
    hd = h.cuda().requires_grad_()
    (F.normal_from_height(hd, 1.5, "directx") * w.cuda()).sum().backward()
    for b in range(3):
        h64 = h[b].double().requires_grad_()
        (ref_height(h64, 1.5, True) * w[b].double()).sum().backward()
        _close(hd.grad[b], h64.grad, ("g_h", b))


@pytest.mark.parametrize("case", ["rotate", "strength", "invert"])
def test_transform_gradient(case):
    from pypbr_amd import functional as F
    m, renorm = {"rotate": (_rot(-45), True), "strength": (((0.5, 0.0), (0.0, 0.5)), True), "invert": (((1.0, 0.0), (0.0, -1.0)), False)}[case]
    g = torch.Generator().manual_seed(7)
    n = torch.rand(2, 3, 33, 40, generator=g) - 0.5
    w = torch.randn(2, 3, 33, 40, generator=g)
    nd = n.cuda().requires_grad_()
    (F.transform_normals(nd, m, renorm) * w.cuda()).sum().backward()
    n64 = n.double().requires_grad_()
    (ref_transform(n64, m, renorm) * w.double()).sum().backward()
    _close(nd.grad, n64.grad, case)


LIGHT = dict(view=torch.tensor([0.0, 0.0, 1.0]), light=torch.tensor([0.1, 0.1, 1.0]), intensity=torch.tensor([1.0, 1.0, 1.0]))


def test_height_through_cook_torrance():
    from pypbr_amd import functional as F
    g = torch.Generator().manual_seed(11)
    H, W = 48, 64
    a, r, m = torch.rand(3, H, W, generator=g), torch.rand(1, H, W, generator=g) * 0.8 + 0.2, torch.rand(1, H, W, generator=g)
    h = torch.rand(1, H, W, generator=g) * 0.1
    hd = h.cuda().requires_grad_()
    out = F.cook_torrance(a.cuda(), F.normal_from_height(hd, 4.0), r.cuda(), m.cuda(), view_dir=LIGHT["view"], light=LIGHT["light"],
                          light_intensity=LIGHT["intensity"], light_type="point")
    out.mean().backward()
    h64 = h.double().requires_grad_()
    ref = O.cook_torrance(a.double(), ref_height(h64, 4.0, False), r.double(), m.double(), None, light_type="point",
                          **{k: v.double() for k, v in LIGHT.items()})
    assert float((out.detach().cpu().double() - ref.detach()).abs().max()) <= 1e-5
    ref.mean().backward()
    _close(hd.grad, h64.grad, "g_h through the render")


def test_rendering_loss_fills_height_grad():
    from pypbr_amd.losses import RenderingLoss
    from pypbr_amd.materials import BasecolorMetallicMaterial
    g = torch.Generator().manual_seed(12)
    H, W = 32, 40
    a, r, m = torch.rand(3, H, W, generator=g), torch.rand(1, H, W, generator=g) * 0.8 + 0.2, torch.rand(1, H, W, generator=g)
    h, ht = torch.rand(1, H, W, generator=g) * 0.1, torch.rand(1, H, W, generator=g) * 0.1
    hd = h.cuda().requires_grad_()
    pred = BasecolorMetallicMaterial(albedo=a.cuda(), roughness=r.cuda(), metallic=m.cuda(), height=hd).compute_normal_from_height(4.0)
    target = BasecolorMetallicMaterial(albedo=a.cuda(), roughness=r.cuda(), metallic=m.cuda(), height=ht.cuda()).compute_normal_from_height(4.0)
    RenderingLoss(light_type="point")(pred, target).backward()
    assert hd.grad is not None
    h64 = h.double().requires_grad_()
    args = (a.double(),)

    def render(n):
        return O.cook_torrance(*args, n, r.double(), m.double(), None, light_type="point", **{k: v.double() for k, v in LIGHT.items()})
    loss = TF.mse_loss(render(ref_height(h64, 4.0, False)), render(ref_height(ht, 4.0, False)))
    loss.backward()
    scale = float(h64.grad.abs().max())
    err = float((hd.grad.cpu().double() - h64.grad).abs().max())
    assert err <= 2e-5 * (scale + 1e-30) + 1e-9, (err, scale)


# ---- material level -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("lazy", [False, True])
def test_material_chain_matches_golden(lazy):
    from pypbr_amd.io import load_material_from_folder
    mat = load_material_from_folder(os.path.join(ROOT, "tests", "golden", "tiles"), preferred_workflow="metallic")
    mat.resize(64)
    height = mat._raw["height"].detach().cpu().clone()          # _raw: reading _maps would carry out the repeat recorded below
    mat.tile(2, lazy=lazy)
    assert mat.lazy_tile == (2, 2)                                # the maps live on the device: the repeat is pending either way
    mat.compute_normal_from_height(3.0)
    got = mat._maps["normal"].cpu()
    # the stencil on the TILED height (upstream tiles, then differentiates: seams see the neighbouring tile), at the parity bar
    assert float((got - ref_height(height.repeat(1, 2, 2), 3.0, False, torch.float32)).abs().max()) <= 1e-6
    # the whole chain against the reference: resize's own last-bit deviation from F.interpolate enters the difference of two
    # neighbours times the scale, so the bar is 2 x 3 x that of the stencil alone
    want = _t("chain__tiles")
    assert got.shape == want.shape and float((got - want).abs().max()) <= 6e-6


def test_freshly_loaded_16_bit_height_matches_golden():
    """A folder material's height is still the PNG's 16-bit samples when compute_normal_from_height is the first operation."""
    from pypbr_amd import functional as F
    from pypbr_amd.io import load_material_from_folder
    mat = load_material_from_folder(os.path.join(ROOT, "tests", "golden", "tiles"), preferred_workflow="metallic")
    assert F.is_encoded(mat._raw["height"]) and mat._raw["height"].dtype == torch.uint16
    mat.compute_normal_from_height(10.0)
    got = mat._maps["normal"][:, :96, :96].cpu()
    assert float((got - _t("fresh__tiles")).abs().max()) <= 1e-6


def test_freshly_loaded_8_bit_height(tmp_path):
    from PIL import Image
    from pypbr_amd import functional as F
    from pypbr_amd.io import load_material_from_folder
    src = os.path.join(ROOT, "tests", "golden", "tiles")
    for name in ("basecolor.png", "roughness.png", "metallic.png"):
        Image.open(os.path.join(src, name)).save(str(tmp_path / name))
    h16 = np.array(Image.open(os.path.join(src, "height.png")), dtype=np.uint16)[:200, :136]
    Image.fromarray((h16 >> 8).astype(np.uint8), mode="L").save(str(tmp_path / "height.png"))
    mat = load_material_from_folder(str(tmp_path), preferred_workflow="metallic")
    assert F.is_encoded(mat._raw["height"]) and mat._raw["height"].dtype == torch.uint8
    mat.compute_normal_from_height(4.0)
    want = ref_height(torch.from_numpy((h16 >> 8).astype(np.float32))[None].div(255), 4.0, False, torch.float32)
    assert float((mat._maps["normal"].cpu() - want).abs().max()) <= 1e-6


def test_flat_height_gives_exact_up_normals():
    from pypbr_amd.materials import BasecolorMetallicMaterial
    up = torch.cat([torch.zeros(2, 16, 24), torch.ones(1, 16, 24)])
    for level in (0.0, 0.25):          # zero padding: a raised plateau slopes at the border, its interior is flat
        mat = BasecolorMetallicMaterial(albedo=torch.rand(3, 16, 24), roughness=torch.rand(1, 16, 24), metallic=torch.rand(1, 16, 24),
                                        height=torch.full((1, 16, 24), level))
        mat.compute_normal_from_height(5.0)
        n = mat._maps["normal"].cpu()
        assert torch.equal(n[:, 1:-1, 1:-1], up[:, 1:-1, 1:-1]), level
        if level == 0.0:
            assert torch.equal(n, up)


def test_material_transforms():
    from pypbr_amd.materials import BasecolorMetallicMaterial, NormalConvention
    g = torch.Generator().manual_seed(3)
    n = torch.rand(3, 20, 28, generator=g) - 0.5
    n = n / n.norm(dim=0, keepdim=True)
    mat = BasecolorMetallicMaterial(albedo=torch.rand(3, 20, 28).cuda(), roughness=torch.rand(1, 20, 28).cuda(),
                                    metallic=torch.rand(1, 20, 28).cuda(), normal=n.cuda())
    held = mat._maps["normal"]
    assert held.is_cuda
    before = held.clone()
    mat.adjust_normal_strength(2.0)
    assert mat._maps["normal"] is not held and torch.equal(held, before)   # a device tensor the caller held is not written
    before = before.cpu()
    assert float((mat._maps["normal"].cpu() - ref_transform(before, ((2.0, 0.0), (0.0, 2.0)), True)).abs().max()) <= 1e-6
    cur = mat._maps["normal"].cpu().clone()
    mat.invert_normal()
    assert mat.normal_convention == NormalConvention.DIRECTX
    assert torch.equal(mat._maps["normal"].cpu(), ref_transform(cur, ((1.0, 0.0), (0.0, -1.0)), False, torch.float32))


@pytest.mark.parametrize("device", ["cuda", "cpu"])
def test_utils_write_into_their_argument(device):
    from pypbr_amd import utils
    g = torch.Generator().manual_seed(4)
    n = (torch.rand(3, 10, 13, generator=g) - 0.5).to(device)
    orig = n.clone()
    assert utils.rotate_normals(n, 30.0) is n
    assert float((n.cpu() - ref_transform(orig.cpu(), _rot(30), True)).abs().max()) <= 1e-6
    orig, version = n.clone(), n._version
    assert utils.invert_normal(n) is n
    assert torch.equal(n[1], -orig[1]) and torch.equal(n[0], orig[0]) and torch.equal(n[2], orig[2])
    assert n._version > version                           # an in-place edit, as upstream's `normals[1] = -normals[1]`


def test_in_place_edit_of_a_saved_tensor_is_caught():
    """Upstream's in-place utilities bump the version counter, so autograd refuses a graph that saved the tensor before the edit."""
    from pypbr_amd import utils
    n = (torch.rand(3, 8, 8) - 0.5).cuda()
    x = torch.rand(3, 8, 8, device="cuda", requires_grad=True)
    y = (x * n).sum()
    utils.invert_normal(n)
    with pytest.raises(RuntimeError, match="modified by an inplace operation"):
        y.backward()


# ---- batches, bounds, addressing, fp16 ------------------------------------------------------------------------------------------------
def test_batch_images_are_independent():
    from pypbr_amd import functional as F
    g = torch.Generator().manual_seed(9)
    h = torch.rand(5, 1, 23, 68, generator=g).cuda()
    out = F.normal_from_height(h, 2.0)
    for b in range(5):
        assert torch.equal(out[b], F.normal_from_height(h[b], 2.0)), b
    n = torch.rand(5, 3, 23, 68, generator=g).cuda()
    out = F.transform_normals(n, _rot(30), True)
    for b in range(5):
        assert torch.equal(out[b], F.transform_normals(n[b], _rot(30), True)), b


WIDTHS = (1, 3, 4, 5, 7, 8, 127, 128, 130, 256, 260)


@pytest.mark.parametrize("W", WIDTHS)
@pytest.mark.parametrize("dtype", [torch.float32, torch.float16])
def test_guard_bands(W, dtype):
    from pypbr_amd import _native as N
    lib = N.lib()
    s = torch.cuda.current_stream().cuda_stream
    B, H = 2, 19
    g = torch.Generator().manual_seed(W)
    h, n = torch.rand(B, 1, H, W, generator=g).to(dtype), (torch.rand(B, 3, H, W, generator=g) - 0.5).to(dtype)
    code = N.F32 if dtype == torch.float32 else N.F16
    G = Guards()
    hi, out = G.input(h), G.output((B, 3, H, W), dtype)
    assert lib.pbr_normal_from_height(hi.data_ptr(), H * W, out.data_ptr(), 3 * H * W, H * W, B, H, W, 2.0, 0, code, s) == 0
    ni, out2 = G.input(n), G.output((B, 3, H, W), dtype)
    assert lib.pbr_normal_transform(ni.data_ptr(), 3 * H * W, H * W, out2.data_ptr(), 3 * H * W, H * W, B, H * W, 0.8, -0.6, 0.6, 0.8, 1, code, s) == 0
    G.check(("forwards", W, dtype))
    assert float((out.float().cpu() - ref_height(h.float(), 2.0, False, torch.float32)).abs().max()) <= (1e-6 if dtype == torch.float32 else 2e-3)
    if dtype != torch.float32:
        return
    G = Guards()
    hi, gn, gh = G.input(h), G.input(torch.randn(B, 3, H, W, generator=g)), G.output((B, 1, H, W))
    assert lib.pbr_normal_from_height_backward(hi.data_ptr(), H * W, gn.data_ptr(), 3 * H * W, H * W, gh.data_ptr(), H * W, B, H, W, 2.0, 1, s) == 0
    ni, go, gi = G.input(n), G.input(torch.randn(B, 3, H, W, generator=g)), G.output((B, 3, H, W))
    assert lib.pbr_normal_transform_backward(ni.data_ptr(), 3 * H * W, H * W, go.data_ptr(), 3 * H * W, H * W, gi.data_ptr(), 3 * H * W, H * W,
                                             B, H * W, 0.8, -0.6, 0.6, 0.8, 1, s) == 0
    G.check(("backwards", W))


def test_offsets_beyond_2_31_elements_are_right_in_the_last_image():
    """64-bit batch offsets: the last image's normals start past 2^31 elements (and 2^33 bytes), so an int32 element offset would wrap."""
    from pypbr_amd import functional as F
    B, H, W = 180, 2048, 2048
    g = torch.Generator(device="cuda").manual_seed(1)
    h = torch.rand(B, 1, H, W, device="cuda", generator=g)
    out = F.normal_from_height(h, 2.0)
    assert out[B - 1].storage_offset() > 2 ** 31
    last = F.normal_from_height(h[B - 1], 2.0)
    assert torch.equal(out[B - 1], last)
    # not vacuous: the images differ, so reading or writing another image's place would show
    assert float((last - out[0]).abs().max()) > 0.1
    t = F.transform_normals(out, _rot(30), True)
    assert t[B - 1].storage_offset() > 2 ** 31
    assert torch.equal(t[B - 1], F.transform_normals(last, _rot(30), True))
    del t
    from pypbr_amd import _native as N
    gh = torch.empty_like(h)
    s = torch.cuda.current_stream().cuda_stream
    P = H * W
    assert N.lib().pbr_normal_from_height_backward(h.data_ptr(), P, out.data_ptr(), 3 * P, P, gh.data_ptr(), P, B, H, W, 2.0, 0, s) == 0
    gl = torch.empty_like(h[B - 1:])
    assert N.lib().pbr_normal_from_height_backward(h[B - 1].data_ptr(), P, out[B - 1].data_ptr(), 3 * P, P, gl.data_ptr(), P, 1, H, W, 2.0, 0,
                                                   s) == 0
    assert torch.equal(gh[B - 1], gl[0]) and not torch.equal(gh[0], gl[0])
    del h, out, gh
    torch.cuda.empty_cache()


def test_fp16_storage_within_one_ulp():
    from pypbr_amd import functional as F
    g = torch.Generator().manual_seed(6)
    h = torch.rand(1, 50, 72, generator=g).half()
    got = F.normal_from_height(h.cuda(), 3.0).cpu().float()
    want = F.normal_from_height(h.float().cuda(), 3.0).cpu().half().float()
    ulp = torch.finfo(torch.float16).eps * torch.clamp(want.abs(), min=2 ** -14)
    assert bool(((got - want).abs() <= ulp).all())
    n = (torch.rand(3, 50, 72, generator=g) - 0.5).half()
    got = F.transform_normals(n.cuda(), _rot(30), True).cpu().float()
    want = F.transform_normals(n.float().cuda(), _rot(30), True).cpu().half().float()
    ulp = torch.finfo(torch.float16).eps * torch.clamp(want.abs(), min=2 ** -14)
    assert bool(((got - want).abs() <= ulp).all())
    with pytest.raises(NotImplementedError):
        F.normal_from_height(h.cuda().requires_grad_(), 1.0)


# ---- operators ------------------------------------------------------------------------------------------------------------------------
def test_opcheck_the_four_operators():
    from pypbr_amd import torch_ops
    assert torch_ops.available()
    g = torch.Generator().manual_seed(8)
    h = torch.rand(1, 12, 20, generator=g).cuda().requires_grad_()
    n = (torch.rand(3, 12, 20, generator=g) - 0.5).cuda().requires_grad_()
    gn = torch.randn(3, 12, 20, generator=g).cuda()
    torch.library.opcheck(torch.ops.pbr_hip.normal_from_height.default, (h, 2.0, False))
    torch.library.opcheck(torch.ops.pbr_hip.normal_from_height_backward.default, (h.detach(), gn, 2.0, True))
    torch.library.opcheck(torch.ops.pbr_hip.normal_transform.default, (n, 0.8, -0.6, 0.6, 0.8, True))
    torch.library.opcheck(torch.ops.pbr_hip.normal_transform_backward.default, (n.detach(), gn, 0.8, -0.6, 0.6, 0.8, True))
    out = torch.ops.pbr_hip.normal_from_height(h, 2.0, False)
    from pypbr_amd import functional as F
    assert torch.equal(out, F.normal_from_height(h.detach(), 2.0))
