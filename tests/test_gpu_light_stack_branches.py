"""The light stack (csrc/ct_stack.hip) where each light lands on its own branch: pbr_cook_torrance_mse_stack_step and
pbr_cook_torrance_stack on the branch fixture in stack mode (oracle/branch_cases.py, stack=True; populations held on the CPU by
tests/test_light_stack_branches_host.py).

The step is backward_body_to with the StackMseLoss policy: the one-light chain rule inside a run-time light loop, every light with its
own clamp, encode slope, target and upstream gradient, all adjoints added into one PixelAdjointT.  Random maps lit from above never
have a light behind the surface, a saturated image or a colour under the encode knee; here every case of test_gpu_gradient_branches
is read as a stack of three images, and `split_lights` puts the three lights on different sides of the surface, so that the set of
lit lights changes from pixel to pixel and a light that renders exactly 0 against a target that is not 0 is one term of a sum.

Ground truth: float64 autograd through the pinned ATen oracle of mse_loss(stack, target); the target is the oracle's stack of another
material of the case (branch_cases.stack_target).  The loss is scaled by N / 2, so the upstream gradient is out - target and the band
means what it means in test_mse_step_gradients_on_every_branch.  The rules are _check_maps of test_gpu_gradient_branches: finite
everywhere, on decided pixels within BAND (1 + |g64|) (fp16 maps: plus the fp16 rule with stored_scale), exactly 0 where every light
is decided behind, decided share at least 95 %.  The forward stack is held to TRACK (test_gpu_parity) on ALL pixels -- clamps and
knees are continuous -- and the image of a light decided behind must be exactly 0.0 (linear_to_srgb(0) = 0 when encoded).

The forward's one-pixel-per-lane instantiation is reached through the public `tuning={"max_vec": 1}` and runs `stack-pairs` once more.
No tolerance here is new: BAND, the fp16 rule, TRACK and _tol (test_gpu_light_stack) are the project's."""
import functools

import pytest
import torch

import branch_cases as BC
from test_gpu_gradient_branches import MAPS, _check_maps
from test_gpu_light_stack import _tol
from test_gpu_parity import TRACK

pytestmark = pytest.mark.gpu

VARIANTS = BC.all_stack_variants()
IDS = [BC.variant_id(n, kw) for n, kw in VARIANTS]
KW = {BC.variant_id(n, kw): (n, kw) for n, kw in VARIANTS}
ENTRIES = list(BC.STACK_ENTRY_CONFIGS)


@functools.lru_cache(maxsize=None)
def _ref(entry, vid, seed=0):
    """Case, target and float64 reference of one (variant, entry, seed): computed once, shared, never written into."""
    name, kw = KW[vid]
    case = BC.build_for(entry, name, kw, seed=seed)
    target = BC.stack_target(entry, name, kw, seed=seed)
    want = BC.gradients(case, loss_target=target.double())
    loss64 = float(((want["out"] - target.double()) ** 2).mean())
    return dict(case=case, target=target, want=want, loss64=loss64, tag="%s %s" % (vid, entry),
                dtype=torch.float16 if BC.STACK_ENTRY_CONFIGS[entry][4] else torch.float32)


def _call_kwargs(case):
    return dict(view_dir=case.view.float(), light=case.lights.float(), light_intensity=case.intensities.float(), **case.product_kwargs())


def _leaves(cases, dtype, grad=True):
    """The maps of one case, or of several as a batch, on the device."""
    cols = zip(*[c.maps() for c in cases])
    return [None if ts[0] is None else (ts[0] if len(cases) == 1 else torch.stack(ts)).to(dtype).cuda().requires_grad_(grad) for ts in cols]


def _check_step(refs, loss, leaves, scale):
    """The step's loss and gradients of a batch of len(refs) materials (leaves unbatched for one) against each material's reference."""
    loss64 = sum(r["loss64"] for r in refs) / len(refs)
    print("%s: loss %.9g (float64 %.9g)" % (refs[0]["tag"], loss.item(), loss64))
    assert abs(loss.item() - loss64) <= 1e-6 * (1 + loss64)
    for b, r in enumerate(refs):
        case = r["case"]
        got = {n: (t.grad if len(refs) == 1 else t.grad[b]).cpu() for n, t in zip(MAPS, leaves) if t is not None}
        per_material = r["target"].numel() / 2.0                # the reference is the mean over ONE material's stack
        _check_maps(case, got, {n: r["want"][n] * per_material for n in case.map_names()}, "%s material %d stack step" % (r["tag"], b),
                    fp16=r["dtype"] == torch.float16, stored_scale=scale)


@pytest.mark.parametrize("entry", ENTRIES)
@pytest.mark.parametrize("vid", IDS)
def test_stack_step_gradients_on_every_branch(vid, entry):
    """pbr_cook_torrance_mse_stack_step through functional.rendering_loss_mse_stack: one step call, loss and summed gradients."""
    from pypbr_amd import functional as F
    r = _ref(entry, vid)
    case, target = r["case"], r["target"]
    scale = target.numel() / 2.0
    leaves = _leaves([case], r["dtype"])
    before = F.STACK_LAUNCHES["mse_stack_step"]
    loss = F.rendering_loss_mse_stack(*leaves, targets=target.cuda(), **_call_kwargs(case))
    assert type(loss.grad_fn).__name__ == "_MseStackStepFnBackward"
    assert F.STACK_LAUNCHES["mse_stack_step"] == before + 1
    (loss * scale).backward()
    _check_step([r], loss.detach(), leaves, scale)
    if entry == "stack-pairs" and case.workflow == "metallic" and case.albedo_is_srgb and case.return_srgb:
        # what the module can express (metallic workflow, sRGB in and out): through losses.MultiLightRenderingLoss itself
        from pypbr_amd.losses import MultiLightRenderingLoss
        from pypbr_amd.materials import BasecolorMetallicMaterial
        again = _leaves([case], r["dtype"])
        mat = BasecolorMetallicMaterial(albedo=again[0], normal=None, roughness=again[2], metallic=again[3], device=torch.device("cuda"))
        mat._maps["normal"] = again[1]                # the stored (already decoded) normal map, as the oracle takes it
        crit = MultiLightRenderingLoss(case.light_type, case.view.float(), case.lights.float(), case.intensities.float(), case.light_size)
        before = F.STACK_LAUNCHES["mse_stack_step"]
        via_module = crit(mat, target.cuda())
        assert type(via_module.grad_fn).__name__ == "_MseStackStepFnBackward" and F.STACK_LAUNCHES["mse_stack_step"] == before + 1
        (via_module * scale).backward()
        _check_step([dict(r, tag=r["tag"] + " module")], via_module.detach(), again, scale)


def _check_images(r, out, tag):
    """One material's stack [L,3,H,W] against float64: TRACK on all pixels, and exactly 0 for a light decided behind."""
    case = r["case"]
    assert out.shape == r["want"]["out"].shape and out.dtype == torch.float32
    err = (out.double() - r["want"]["out"]).abs()
    print("%s: worst error / TRACK per light %s" % (tag, ["%.3f" % (float(e) / TRACK) for e in err.amax(dim=(1, 2, 3))]))
    assert float(err.max()) <= TRACK, (tag, float(err.max()), torch.nonzero(err > TRACK)[:4].tolist())
    behind = BC.behind(case)
    if case.name in ("split_lights", "backlit", "dark"):
        assert float(behind.double().mean()) >= 0.10, tag
    masked = out.permute(1, 0, 2, 3)[:, behind]
    assert bool((masked == 0.0).all()), (tag, "image of a light behind the surface", float(masked.abs().max()))


@pytest.mark.parametrize("entry", ENTRIES)
@pytest.mark.parametrize("vid", IDS)
def test_forward_stack_images_on_every_branch(vid, entry):
    """pbr_cook_torrance_stack: the packed shade_light, the per-light encode and (23 x 37) the overlapping last lane on clamped, dark and
    back-lit colours; `stack-pairs` once more with one pixel per lane."""
    from pypbr_amd import functional as F
    r = _ref(entry, vid)
    case = r["case"]
    maps = _leaves([case], r["dtype"], grad=False)
    for tuning in ([None, {"max_vec": 1}] if entry == "stack-pairs" else [None]):
        before = F.STACK_LAUNCHES["cook_torrance_stack"]
        out = F.cook_torrance_stack(*maps, tuning=tuning, **_call_kwargs(case))
        assert F.STACK_LAUNCHES["cook_torrance_stack"] == before + 1 and not out.requires_grad
        _check_images(r, out.cpu(), r["tag"] + (" forward" if tuning is None else " forward, one pixel per lane"))


@pytest.mark.parametrize("entry", ["stack-pairs", "stack-fp16"])
@pytest.mark.parametrize("vid", [BC.variant_id("split_lights", kw) for kw in BC.VARIANTS["split_lights"]])
def test_batch_of_two_materials_on_masked_lights(vid, entry):
    """B = 2 from seeds 0 and 1 of `split_lights` (the tilts mirrored: other lights behind at the same pixel), per-material targets:
    targets + b L 3 HW in the step and the stack's o_bs in the forward, on lights that must be masked."""
    from pypbr_amd import functional as F
    refs = [_ref(entry, vid, seed) for seed in (0, 1)]
    cases = [r["case"] for r in refs]
    targets = torch.stack([r["target"] for r in refs])
    assert not torch.equal(BC.behind(cases[0]), BC.behind(cases[1]))
    scale = targets.numel() / 2.0
    leaves = _leaves(cases, refs[0]["dtype"])
    before = F.STACK_LAUNCHES["mse_stack_step"]
    loss = F.rendering_loss_mse_stack(*leaves, targets=targets.cuda(), **_call_kwargs(cases[0]))
    assert type(loss.grad_fn).__name__ == "_MseStackStepFnBackward" and F.STACK_LAUNCHES["mse_stack_step"] == before + 1
    (loss * scale).backward()
    _check_step(refs, loss.detach(), leaves, scale)
    before = F.STACK_LAUNCHES["cook_torrance_stack"]
    out = F.cook_torrance_stack(*_leaves(cases, refs[0]["dtype"], grad=False), **_call_kwargs(cases[0])).cpu()
    assert F.STACK_LAUNCHES["cook_torrance_stack"] == before + 1 and out.shape == targets.shape
    for b, r in enumerate(refs):
        _check_images(r, out[b], "%s material %d forward" % (r["tag"], b))


@pytest.mark.parametrize("vid", [BC.variant_id(n, kw) for n in ("split_lights", "saturated") for kw in BC.VARIANTS[n]])
def test_stack_step_against_the_sum_of_one_light_steps(vid):
    """The same device, the same chain rule, L one-light steps (pbr_cook_torrance_mse_step) each divided by L: what separates a wrong
    stack from a wrong chain rule when something above fails."""
    from pypbr_amd import functional as F
    r = _ref("stack-pairs", vid)
    case, target = r["case"], r["target"].cuda()
    kw = _call_kwargs(case)
    L = case.n_lights
    fused = _leaves([case], torch.float32)
    loss = F.rendering_loss_mse_stack(*fused, targets=target, **kw)
    assert type(loss.grad_fn).__name__ == "_MseStackStepFnBackward"
    loss.backward()
    steps = _leaves([case], torch.float32)
    total = 0.0
    for l in range(L):
        one = F.rendering_loss_mse(*steps, target=target[l], **dict(kw, light=kw["light"][l], light_intensity=kw["light_intensity"][l]))
        assert type(one.grad_fn).__name__ == "_MseStepFnBackward"
        (one / L).backward()
        total += one.item() / L
    assert abs(total - loss.item()) <= 2e-6 * (1 + loss.item())
    for name, x, y in zip(MAPS, fused, steps):
        if x is not None:
            scale = float(y.grad.abs().max())
            d = float((x.grad - y.grad).abs().max())
            print("%s %-9s stack - sum of one-light steps: %.3e, tolerance %.3e" % (r["tag"], name, d, _tol(torch.float32, scale)))
            assert d <= _tol(torch.float32, scale), (vid, name, d, scale)
