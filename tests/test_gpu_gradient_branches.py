"""Render gradients where clamps, sRGB knees and back faces decide (ct_backward.hpp, ct_repeat_backward.hpp, ct_loss.hip).

Inputs: oracle/branch_cases.py -- normals tilted out to +-80 degrees, albedo from below 0 to above 1, lights that saturate or stay
under the encode knee, a view from behind.  tests/test_branch_cases_host.py holds every case to its populations on the CPU.
Ground truth: float64 autograd through the pinned ATen oracle of sum(out * W).  On DECIDED pixels (every quantity the reference
compares with a threshold is at least 1e-3 from it, and the oracle's own fp32 gradient agrees with its fp64 gradient) the
kernel's gradient must lie in the project's band |g - g64| <= 2e-5 (1 + |g64|); every gradient element must be finite on all
pixels; on back-lit decided pixels it must be exactly 0; and at least 95 % of a case's pixels must be decided.

Every case runs through each entry point that has its own copy or instantiation of the chain rule: fp32 vector lanes and
one-pixel kernels, three lights, fp16 maps (streamed and one-tile, bit-identical to each other), folded gradients of tiled
maps (sum-first, point light, two-kernel fallback), the one-kernel MSE step, and the view / light / intensity adjoints.

`closed_ends` (albedo exactly 0.0 and 1.0, metallic exactly 0 and 1): all four ends survive -- the oracle's float32 and float64
gradients agree within half the band on every such texel (torch's clamp passes the gradient at both ends in either precision,
and (1.0 + 0.055) / 1.055 raised to 2.4 does not exceed 1), so none of them is left out of the comparison.

fp16 maps: the kernel does the same fp32 arithmetic and rounds each gradient once to fp16, so the bound is the band plus the
rule of test_gradients_of_fp16_maps, 1e-3 (1e-3 + |g64|) (2^-11 relative, subnormal floor).

Several lights here are SUMMED into one image.  The light stack (one image, clamp and encode per light) runs on the fixture's stack
mode in tests/test_gpu_light_stack_branches.py, which shares _check_maps below."""
import pytest
import torch

import branch_cases as BC

pytestmark = pytest.mark.gpu

VARIANTS = BC.all_variants()
IDS = [BC.variant_id(n, kw) for n, kw in VARIANTS]
MAPS = ("albedo", "normal", "roughness", "metallic", "specular")


def _params(case):
    one = case.n_lights == 1
    return case.view.float(), (case.lights[0] if one else case.lights).float(), (case.intensities[0] if one else case.intensities).float()


def _device_gradients(case, dtype=torch.float32, params=False):
    """sum(out * W) through pypbr_amd.functional.cook_torrance and its backward kernels -> dict like branch_cases.gradients."""
    from pypbr_amd import functional as F
    leaves = [None if t is None else t.to(dtype).cuda().requires_grad_(True) for t in case.maps()]
    P = [t.clone().cuda().requires_grad_(params) for t in _params(case)]
    out = F.cook_torrance(*leaves, view_dir=P[0], light=P[1], light_intensity=P[2], **case.product_kwargs())
    (out * case.weight.float().cuda()).sum().backward()
    res = {n: t.grad.cpu() for n, t in zip(MAPS, leaves) if t is not None}
    if params:
        res.update(view=P[0].grad.cpu(), lights=P[1].grad.cpu().reshape(-1, 3), intensities=P[2].grad.cpu().reshape(-1, 3))
    return res


def _check_maps(case, got, want, tag, fp16=False, stored_scale=1.0):
    decided = BC.decided(case)
    share = float(decided.double().mean())
    assert share >= 0.95, (tag, "decided share", share)
    dark = BC.backlit(case) & decided
    for name in case.map_names():
        g, ref = got[name], want[name]
        assert g.shape == ref.shape and g.dtype == (torch.float16 if fp16 else torch.float32), (tag, name)
        assert bool(torch.isfinite(g).all()), (tag, name, "not finite at", torch.nonzero(~torch.isfinite(g))[:4].tolist())
        err = (g.double() - ref).abs()
        # the fp16 rule holds for the value the kernel STORES in fp16; `want` is stored_scale times that (the MSE step, below)
        band = BC.BAND * (1 + ref.abs()) + (1e-3 * (1e-3 * stored_scale + ref.abs()) if fp16 else 0.0)
        bad = (err > band) & decided
        worst = float((err / band)[:, decided].max())
        print("%s %-9s decided %.1f%%  worst error / band %.3f  max |g64| %.3g" % (tag, name, 100 * share, worst, float(ref.abs().max())))
        assert not bool(bad.any()), (tag, name, "worst error / band", worst, "at", torch.nonzero(bad)[:4].tolist())
        assert bool((g[:, dark] == 0).all()), (tag, name, "gradient on back-lit pixels", float(g[:, dark].abs().max()))
    if case.name == "backlit":
        assert float(dark.double().mean()) >= 0.10, tag


ENTRIES_FP32 = ["fp32-vector-lanes", "fp32-vector-lanes-point", "fp32-one-pixel", "multi-point", "multi-directional",
                "tiled-sum-first", "tiled-point", "tiled-two-kernels"]


@pytest.mark.parametrize("entry", ENTRIES_FP32)
@pytest.mark.parametrize("name,kw", VARIANTS, ids=IDS)
def test_fp32_map_gradients_on_every_branch(name, kw, entry):
    """a, b, d: cook_torrance_backward_kernel in its vector (24x40) and one-pixel (23x37) forms, the MULTI path with three
    lights, and pbr_cook_torrance_backward_folded on a map tiled 2 x 2 (12x16 directional: sum-first; point; 12x18: backward + fold)."""
    case = BC.build_for(entry, name, kw)
    _check_maps(case, _device_gradients(case), BC.reference(case), "%s %s" % (BC.variant_id(name, kw), entry))


@pytest.mark.parametrize("name,kw", VARIANTS, ids=IDS)
def test_fp16_map_gradients_streamed_and_one_tile(name, kw):
    """c: fp16 maps, one light.  16x128 rows take the streamed kernel, the same maps cropped to 120 columns the one-tile kernels
    (a directional light shades a pixel the same wherever it is): bit-identical on the shared columns.  A point light streamed too."""
    case = BC.build_for("fp16-streamed", name, kw)
    tag = BC.variant_id(name, kw)
    got = _device_gradients(case, torch.float16)
    _check_maps(case, got, BC.reference(case), tag + " streamed", fp16=True)
    crop = BC.crop(case, 120)
    one_tile = _device_gradients(crop, torch.float16)
    _check_maps(crop, one_tile, BC.reference(crop), tag + " one-tile", fp16=True)
    for n in case.map_names():
        assert torch.equal(one_tile[n], got[n][:, :, :120]), (tag, n, "streamed and one-tile kernels differ")
    point = BC.build_for("fp16-streamed-point", name, kw)
    _check_maps(point, _device_gradients(point, torch.float16), BC.reference(point), tag + " streamed point", fp16=True)


@pytest.mark.parametrize("entry,dtype", [("fp32-vector-lanes-point", torch.float32), ("fp32-one-pixel", torch.float32),
                                         ("multi-directional", torch.float32), ("fp16-streamed", torch.float16)])
@pytest.mark.parametrize("name,kw", VARIANTS, ids=IDS)
def test_mse_step_gradients_on_every_branch(name, kw, entry, dtype):
    """e: pbr_cook_torrance_mse_step, through losses.RenderingLoss where the module can express the case, else through the function it
    calls (functional.rendering_loss_mse).  The target is the oracle's
    rendering of ANOTHER material of the same case (next seed), so out - target has both signs on every branch.  The loss is scaled
    by N / 2, so that the upstream gradient is out - target itself and the band means what it means for the other entry points.
    The step stores its gradients BEFORE that upstream factor (d mean / d out = 2 / N), so with fp16 maps they are rounded to fp16 at
    2 / N of the size compared here, partly in fp16's subnormal range (spacing 2^-24): the subnormal floor of the fp16 rule, 1e-3 * 1e-3
    of the stored value, is N / 2 times that in the compared one."""
    from pypbr_amd import functional as F
    case = BC.build_for(entry, name, kw)
    target = BC.render(BC.build_for(entry, name, kw, seed=1)).float()
    scale = target.numel() / 2.0
    want = BC.gradients(case, loss_target=target.double())
    leaves = [None if t is None else t.to(dtype).cuda().requires_grad_(True) for t in case.maps()]
    view, light, inten = _params(case)
    if case.workflow == "metallic" and case.albedo_is_srgb and case.return_srgb and dtype == torch.float32:
        # what the module can express (it renders sRGB out, metallic or specular workflow): through losses.RenderingLoss itself
        from pypbr_amd.losses import RenderingLoss
        from pypbr_amd.materials import BasecolorMetallicMaterial
        mat = BasecolorMetallicMaterial(albedo=leaves[0], normal=None, roughness=leaves[2], metallic=leaves[3], device=torch.device("cuda"))
        mat._maps["normal"] = leaves[1]               # the stored (already decoded) normal map, as the oracle takes it
        loss = RenderingLoss(light_type=case.light_type, view_dir=view, light_dir=light, light_intensity=inten,
                             light_size=case.light_size)(mat, target.cuda())
    else:                                             # linear output, the converted workflow, fp16 maps: the call the module makes
        loss = F.rendering_loss_mse(*leaves, target=target.cuda(), view_dir=view, light=light, light_intensity=inten, **case.product_kwargs())
    assert type(loss.grad_fn).__name__ == "_MseStepFnBackward"
    (loss * scale).backward()
    got = {n: t.grad.cpu() for n, t in zip(MAPS, leaves) if t is not None}
    diff = want["out"] - target.double()
    assert float((diff > 1e-3).double().mean()) > 0.05 and float((diff < -1e-3).double().mean()) > 0.05
    _check_maps(case, got, {n: want[n] * scale for n in case.map_names()}, "%s %s mse" % (BC.variant_id(name, kw), entry), fp16=dtype == torch.float16, stored_scale=scale)


@pytest.mark.parametrize("entry", ["fp32-vector-lanes-point", "fp32-vector-lanes", "multi-point", "multi-directional"])
@pytest.mark.parametrize("name,kw", VARIANTS, ids=IDS)
def test_view_light_and_intensity_gradients_on_every_branch(name, kw, entry):
    """f: pbr_cook_torrance_backward_params.  These gradients are sums over all pixels, so the fixture's undecided texels take a
    decided neighbour's values first (none may be left); tolerance as in test_gradients_of_view_light_and_intensity."""
    case, left = BC.fill_undecided(BC.build_for(entry, name, kw))
    assert left == 0.0
    tag = "%s %s params" % (BC.variant_id(name, kw), entry)
    want = BC.gradients(case, params=True)
    got = _device_gradients(case, params=True)
    for pname in ("view", "lights", "intensities"):
        g, ref = got[pname].double().reshape(want[pname].shape), want[pname]
        assert bool(torch.isfinite(g).all()), (tag, pname)
        scale = ref.abs().max().item()
        err = (g - ref).abs()
        print("%s %-11s worst error / bound %.3f  scale %.3g" % (tag, pname, float(err.max()) / (2e-5 * (1.0 + scale)), scale))
        assert bool((err <= 2e-5 * (1.0 + scale)).all()), (tag, pname, float(err.max()), scale)
    _check_maps(case, got, want, tag)
