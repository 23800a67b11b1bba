"""Perspective-camera gradients where clamps, sRGB knees and back faces decide (csrc/ct_camera.hip, ct_camera_stack.hip, ct_view_stack.hip).

The camera kernels run ct_chain_rule.hpp over a per-pixel view: pixel_view and its rv, the camera's per-pixel Jacobian ahead of the parameter
sums, view_terms inside the light loop, N.V's adjoint closed per shot, parameter rows of 3 + 6 L and 9 L floats.  Their own tests
(test_gpu_camera*.py, test_gpu_view_stack.py) run on random normals and ordinary colours, built to stay AWAY from the branches.  Here the inputs
are oracle/branch_cases.py in camera mode -- a saturated channel, a colour under the encode knee, albedo outside (0.04045, 1), N.H < 0 < N.L,
a light behind the surface whose target is not 0, a shot seen from behind -- with N.V and N.H changing sign from pixel to pixel inside one
lane group; tests/test_camera_branches_host.py holds every case to its populations on the CPU.

Ground truth: float64 autograd through tools/camera_oracle.py (pinned to upstream pixel by pixel by test_camera_host).  No tolerance is new:

  * maps: _check_maps of test_gpu_gradient_branches -- finite everywhere, on decided pixels within BAND (1 + |g64|) (fp16 maps: plus the fp16
    rule with stored_scale), exactly 0 where every light is decided behind, decided share at least 95 %;
  * forward images: TRACK (test_gpu_parity) on ALL pixels, and in a stack exactly 0.0 for a light decided behind;
  * camera position(s), lights, intensities: test_gpu_camera._param_band, 2e-5 S + 1e-9, on fill_undecided cases (the host test holds the
    oracle's own float32 gradients to half of it);
  * losses: 1e-6 (1 + loss64); the localiser: _tol of test_gpu_light_stack.

Every comparison prints its worst error / band."""
import functools

import pytest
import torch

import branch_cases as BC
from test_camera_branches_host import BATCH_CASES, PARAM_ENTRIES
from test_gpu_camera import _param_band
from test_gpu_gradient_branches import MAPS, _check_maps
from test_gpu_light_stack import _tol
from test_gpu_parity import TRACK

pytestmark = pytest.mark.gpu

KW = {BC.variant_id(n, kw): (n, kw) for n, kw in BC.all_view_stack_variants()}
SUM_ENTRIES = BC.camera_entries("sum")
STACK_ENTRIES = BC.camera_entries("camera_stack") + BC.camera_entries("view_stack")
PARAMS = ("view", "lights", "intensities")


def _pairs(entries, names=None):
    """(variant id, entry) for every variant an entry runs (`split_lights` in stacks only, `split_views` with a camera per shot only)."""
    return [(BC.variant_id(n, kw), e) for e in entries for n, kw in BC.camera_variants(e) if names is None or n in names]


def _mode(entry):
    return BC.CAMERA_ENTRY_CONFIGS[entry][5]


def _dtype(entry):
    return torch.float16 if BC.CAMERA_ENTRY_CONFIGS[entry][4] else torch.float32


def _prefix(entry):
    """Launch-counter prefix and grad_fn stem of a stack entry."""
    return ("view", "_ViewStack") if _mode(entry) == "view_stack" else ("camera", "_CameraStack")


@functools.lru_cache(maxsize=None)
def _case(entry, vid, seed=0, filled=False):
    name, kw = KW[vid]
    case = BC.build_for(entry, name, kw, seed=seed)
    if filled:
        case, left = BC.fill_undecided(case)
        assert left == 0.0
    return case


@functools.lru_cache(maxsize=None)
def _sum_ref(entry, vid, filled=False):
    """float64 gradients of sum(out * W), parameters included: computed once, shared, never written into."""
    return BC.gradients(_case(entry, vid, 0, filled), params=True)


@functools.lru_cache(maxsize=None)
def _mse_ref(entry, vid, seed=0, filled=False):
    """Case, target (another seed's rendering) and float64 reference of mse_loss(out, target), parameters included."""
    name, kw = KW[vid]
    case = _case(entry, vid, seed, filled)
    target = BC.camera_target(entry, name, kw, seed=seed)
    want = BC.gradients(case, params=True, loss_target=target.double())
    return dict(case=case, target=target, want=want, loss64=float(((want["out"] - target.double()) ** 2).mean()),
                tag="%s %s" % (vid, entry), dtype=_dtype(entry))


def _param_tensors(case, where="cpu", wanted=()):
    one = case.n_lights == 1 and not case.stack
    src = dict(view=case.camera, lights=case.lights[0] if one else case.lights, intensities=case.intensities[0] if one else case.intensities)
    return {k: t.float().clone().to(where).requires_grad_(k in wanted) for k, t in src.items()}


def _call_kwargs(case, params=None):
    p = _param_tensors(case) if params is None else params
    return dict(view_dir=p["view"], light=p["lights"], light_intensity=p["intensities"], **case.product_kwargs())


def _leaves(cases, dtype, grad=True):
    """The maps of one case, or of several as a batch, on the device."""
    cols = zip(*[c.maps() for c in cases])
    return [None if ts[0] is None else (ts[0] if len(cases) == 1 else torch.stack(ts)).to(dtype).cuda().requires_grad_(grad) for ts in cols]


def _grads(leaves, b=None):
    return {n: (t.grad if b is None else t.grad[b]).cpu() for n, t in zip(MAPS, leaves) if t is not None}


def _check_image(out, want, tag):
    assert out.shape == want.shape and out.dtype == torch.float32 and bool(torch.isfinite(out).all()), tag
    err = float((out.double() - want).abs().max())
    print("%s: worst error / TRACK %.3f" % (tag, err / TRACK))
    assert err <= TRACK, (tag, err, torch.nonzero((out.double() - want).abs() > TRACK)[:4].tolist())


def _check_loss(loss, loss64, tag):
    print("%s: loss %.9g (float64 %.9g), error / bound %.3f" % (tag, float(loss), loss64, abs(float(loss) - loss64) / (1e-6 * (1 + loss64))))
    assert abs(float(loss) - loss64) <= 1e-6 * (1 + loss64), (tag, float(loss), loss64)


def _check_params(params, want, scale, tag, where):
    """Every parameter that was a leaf against float64, inside test_gpu_camera's band with S over all three (scaled as the loss was)."""
    want = {k: want[k] * scale for k in PARAMS}
    band = _param_band(want)
    for k, p in params.items():
        if not p.requires_grad:
            assert p.grad is None, (tag, k)
            continue
        assert p.grad is not None and p.grad.shape == p.shape and p.grad.device.type == where, (tag, k)
        g = p.grad.cpu().double().reshape(want[k].shape)
        assert bool(torch.isfinite(g).all()), (tag, k)
        err = float((g - want[k]).abs().max())
        print("%s %s %-11s worst error / band %.3f  (band %.3e)" % (tag, where, k, err / band, band))
        assert err <= band, (tag, where, k, err, band)


# ------------------------------------------------------------------ 1. cook_torrance(view_type="point"): forward and map gradients
@pytest.mark.parametrize("vid,entry", _pairs(SUM_ENTRIES))
def test_map_gradients_on_every_branch(vid, entry):
    """pbr_cook_torrance_camera_backward in its pair (24 x 40) and one-pixel (23 x 37) forms, MULTI, and float and __half maps; the image of
    the same call is held to TRACK."""
    from pypbr_amd import functional as F
    case, dtype = _case(entry, vid), _dtype(entry)
    leaves = _leaves([case], dtype)
    out = F.cook_torrance(*leaves, **_call_kwargs(case))
    (out * case.weight.float().cuda()).sum().backward()
    tag = "%s %s" % (vid, entry)
    _check_image(out.detach().cpu(), BC.reference(case)["out"], tag + " image")
    _check_maps(case, _grads(leaves), BC.reference(case), tag, fp16=dtype == torch.float16)


@pytest.mark.parametrize("vid,entry", _pairs(SUM_ENTRIES))
def test_forward_images_on_every_branch(vid, entry):
    """pbr_cook_torrance_camera with nothing to differentiate: the forward's form without the N.H select, under a view that varies per lane."""
    from pypbr_amd import functional as F
    case = _case(entry, vid)
    out = F.cook_torrance(*_leaves([case], _dtype(entry), grad=False), **_call_kwargs(case))
    assert not out.requires_grad
    _check_image(out.cpu(), BC.reference(case)["out"], "%s %s forward" % (vid, entry))


# ------------------------------------------------------------------ 2. camera position, lights, intensities
@pytest.mark.parametrize("where", ["cpu", "cuda"])
@pytest.mark.parametrize("vid,entry", _pairs([e for e in PARAM_ENTRIES if e in SUM_ENTRIES]))
def test_parameter_gradients_on_every_branch(vid, entry, where):
    """Each of the three a leaf alone, then all three together with the maps; parameters on the host and on the device; two identical calls
    agree bit for bit."""
    from pypbr_amd import functional as F
    case, want = _case(entry, vid, 0, True), _sum_ref(entry, vid, True)
    tag = "%s %s params" % (vid, entry)

    def run(wanted, maps_too):
        leaves = _leaves([case], torch.float32, grad=maps_too)
        params = _param_tensors(case, where, wanted)
        out = F.cook_torrance(*leaves, **_call_kwargs(case, params))
        (out * case.weight.float().cuda()).sum().backward()
        return leaves, params

    for wanted in (("view",), ("lights",), ("intensities",)):
        _, params = run(wanted, False)
        _check_params(params, want, 1.0, tag + " (%s alone)" % wanted[0], where)
    leaves, params = run(PARAMS, True)
    _check_params(params, want, 1.0, tag, where)
    _check_maps(case, _grads(leaves), want, tag)
    again_leaves, again = run(PARAMS, True)
    for k in PARAMS:
        assert torch.equal(params[k].grad, again[k].grad), (tag, k)
    for x, y in zip(leaves, again_leaves):
        assert x is None or torch.equal(x.grad, y.grad), tag


# ------------------------------------------------------------------ 3. the loss step
@pytest.mark.parametrize("vid,entry", _pairs(["camera-vector-lanes-point", "camera-one-pixel", "camera-multi-directional", "camera-fp16"]))
def test_loss_step_on_every_branch(vid, entry):
    """rendering_loss_mse(view_type="point"): one light is the camera stack's step of one image, three summed lights the composition.  The
    loss is scaled by N / 2, so the upstream gradient is out - target itself; the target is another seed's rendering."""
    from pypbr_amd import functional as F
    r = _mse_ref(entry, vid)
    case, target = r["case"], r["target"]
    scale = target.numel() / 2.0
    want = {n: r["want"][n] * scale for n in case.map_names()}

    def check(loss, leaves, tag):
        if case.n_lights == 1:
            assert type(loss.grad_fn).__name__ == "_CameraStackStepFnBackward", tag
        (loss * scale).backward()
        _check_loss(loss.detach(), r["loss64"], tag)
        _check_maps(case, _grads(leaves), want, tag, fp16=r["dtype"] == torch.float16, stored_scale=scale)

    leaves = _leaves([case], r["dtype"])
    before = F.STACK_LAUNCHES["camera_mse_stack_step"]
    loss = F.rendering_loss_mse(*leaves, target=target.cuda(), **_call_kwargs(case))
    assert F.STACK_LAUNCHES["camera_mse_stack_step"] == before + (1 if case.n_lights == 1 else 0)
    check(loss, leaves, r["tag"] + " mse")
    if entry == "camera-vector-lanes-point" and case.workflow == "metallic" and case.albedo_is_srgb and case.return_srgb:
        # what the module can express (metallic workflow, sRGB in and out): through losses.RenderingLoss itself
        from pypbr_amd.losses import RenderingLoss
        from pypbr_amd.materials import BasecolorMetallicMaterial
        again = _leaves([case], r["dtype"])
        mat = BasecolorMetallicMaterial(albedo=again[0], normal=None, roughness=again[2], metallic=again[3], device=torch.device("cuda"))
        mat._maps["normal"] = again[1]                # the stored (already decoded) normal map, as the oracle takes it
        p = _param_tensors(case)
        crit = RenderingLoss(case.light_type, p["view"], p["lights"], p["intensities"], case.light_size, view_type="point")
        check(crit(mat, target.cuda()), again, r["tag"] + " RenderingLoss")


# ------------------------------------------------------------------ 4. the stacks: one camera, and one camera per shot
def _check_step(refs, loss, leaves, scale, what):
    """The step's loss and map gradients of a batch of len(refs) materials (leaves unbatched for one) against each material's reference."""
    _check_loss(loss, sum(r["loss64"] for r in refs) / len(refs), "%s %s" % (refs[0]["tag"], what))
    for b, r in enumerate(refs):
        case = r["case"]
        per_material = r["target"].numel() / 2.0                # the reference is the mean over ONE material's stack
        _check_maps(case, _grads(leaves, None if len(refs) == 1 else b), {n: r["want"][n] * per_material for n in case.map_names()},
                    "%s material %d %s" % (r["tag"], b, what), fp16=r["dtype"] == torch.float16, stored_scale=scale)


def _check_images(r, out, tag):
    """One material's stack [L,3,H,W] against float64: TRACK on all pixels, and exactly 0 for a light decided behind."""
    case = r["case"]
    _check_image(out, r["want"]["out"], tag)
    behind = BC.behind(case)
    if case.name in ("split_lights", "backlit", "dark"):
        assert float(behind.double().mean()) >= 0.10, tag
    masked = out.permute(1, 0, 2, 3)[:, behind]
    assert bool((masked == 0.0).all()), (tag, "image of a light behind the surface", float(masked.abs().max()))


@pytest.mark.parametrize("vid,entry", _pairs(STACK_ENTRIES))
def test_stack_step_gradients_on_every_branch(vid, entry):
    """pbr_cook_torrance_camera_mse_stack_step / pbr_cook_torrance_view_mse_stack_step through functional.rendering_loss_mse_stack: one
    call, the loss and the map gradients summed over the shots."""
    from pypbr_amd import functional as F
    r = _mse_ref(entry, vid)
    case, target = r["case"], r["target"]
    key, stem = _prefix(entry)
    scale = target.numel() / 2.0
    leaves = _leaves([case], r["dtype"])
    before = F.STACK_LAUNCHES[key + "_mse_stack_step"]
    loss = F.rendering_loss_mse_stack(*leaves, targets=target.cuda(), **_call_kwargs(case))
    assert type(loss.grad_fn).__name__ == stem + "StepFnBackward"
    assert F.STACK_LAUNCHES[key + "_mse_stack_step"] == before + 1
    (loss * scale).backward()
    _check_step([r], loss.detach(), leaves, scale, "stack step")
    if entry in ("camera-stack-pairs-point", "view-stack-pairs-point") and case.workflow == "metallic" and case.albedo_is_srgb and case.return_srgb:
        from pypbr_amd.losses import MultiLightRenderingLoss
        from pypbr_amd.materials import BasecolorMetallicMaterial
        again = _leaves([case], r["dtype"])
        mat = BasecolorMetallicMaterial(albedo=again[0], normal=None, roughness=again[2], metallic=again[3], device=torch.device("cuda"))
        mat._maps["normal"] = again[1]
        p = _param_tensors(case)
        crit = MultiLightRenderingLoss(case.light_type, p["view"], p["lights"], p["intensities"], case.light_size, view_type="point")
        before = F.STACK_LAUNCHES[key + "_mse_stack_step"]
        via_module = crit(mat, target.cuda())
        assert type(via_module.grad_fn).__name__ == stem + "StepFnBackward" and F.STACK_LAUNCHES[key + "_mse_stack_step"] == before + 1
        (via_module * scale).backward()
        _check_step([r], via_module.detach(), again, scale, "module")


@pytest.mark.parametrize("vid,entry", _pairs(STACK_ENTRIES))
def test_forward_stack_images_on_every_branch(vid, entry):
    """pbr_cook_torrance_camera_stack / pbr_cook_torrance_view_stack on clamped, dark, back-lit and back-viewed colours, (23 x 37) with the
    overlapping last lane; the 24 x 40 point entries once more with one pixel per lane."""
    from pypbr_amd import functional as F
    r = _mse_ref(entry, vid)
    case = r["case"]
    key, _ = _prefix(entry)
    maps = _leaves([case], r["dtype"], grad=False)
    for tuning in ([None, {"max_vec": 1}] if entry in ("camera-stack-pairs-point", "view-stack-pairs-point") else [None]):
        before = dict(F.STACK_LAUNCHES)
        out = F.cook_torrance_stack(*maps, tuning=tuning, **_call_kwargs(case))
        moved = {k: F.STACK_LAUNCHES[k] - before[k] for k in before if F.STACK_LAUNCHES[k] != before[k]}
        assert moved == {key + "_stack": 1} and not out.requires_grad, moved
        _check_images(r, out.cpu(), r["tag"] + (" forward" if tuning is None else " forward, one pixel per lane"))


@pytest.mark.parametrize("where", ["cpu", "cuda"])
@pytest.mark.parametrize("vid,entry", _pairs([e for e in PARAM_ENTRIES if e in STACK_ENTRIES]))
def test_fit_step_on_every_branch(vid, entry, where):
    """Parameter leaves route to pbr_cook_torrance_camera_mse_stack_fit_step / pbr_cook_torrance_view_mse_stack_fit_step: the map gradients,
    and the camera position(s) ([3] / [L,3]), lights and intensities inside the parameter band; two calls agree bit for bit."""
    from pypbr_amd import functional as F
    r = _mse_ref(entry, vid, 0, True)
    case, target = r["case"], r["target"]
    key, stem = _prefix(entry)
    scale = target.numel() / 2.0

    def run():
        leaves, params = _leaves([case], r["dtype"]), _param_tensors(case, where, PARAMS)
        before = F.STACK_LAUNCHES[key + "_mse_stack_fit_step"]
        loss = F.rendering_loss_mse_stack(*leaves, targets=target.cuda(), **_call_kwargs(case, params))
        assert type(loss.grad_fn).__name__ == stem + "FitFnBackward" and F.STACK_LAUNCHES[key + "_mse_stack_fit_step"] == before + 1
        (loss * scale).backward()
        return loss.detach(), leaves, params

    loss, leaves, params = run()
    assert params["view"].grad.shape == ((case.n_lights, 3) if case.per_shot else (3,))
    _check_step([r], loss, leaves, scale, "fit step")
    _check_params(params, r["want"], scale, r["tag"] + " fit step", where)
    loss2, leaves2, params2 = run()
    assert torch.equal(loss, loss2)
    for k in PARAMS:
        assert torch.equal(params[k].grad, params2[k].grad), (r["tag"], k)
    for x, y in zip(leaves, leaves2):
        assert x is None or torch.equal(x.grad, y.grad), r["tag"]


# ------------------------------------------------------------------ 5. a batch of two materials
@pytest.mark.parametrize("vid,entry", [p for e, n in BATCH_CASES for p in _pairs([e], (n,))])
def test_batch_of_two_materials(vid, entry):
    """B = 2 from seeds 0 and 1 (the tilts mirrored: other lights behind, other shots seen from behind at the same pixel), per-material
    targets, in the step and in the forward stack."""
    from pypbr_amd import functional as F
    refs = [_mse_ref(entry, vid, seed) for seed in (0, 1)]
    cases = [r["case"] for r in refs]
    key, stem = _prefix(entry)
    targets = torch.stack([r["target"] for r in refs])
    front = lambda c: torch.stack([x[0] > 0 for x in BC._terms(c)["ndv_l"]])
    assert not torch.equal(BC.behind(cases[0]), BC.behind(cases[1])) or not torch.equal(front(cases[0]), front(cases[1]))
    scale = targets.numel() / 2.0
    leaves = _leaves(cases, refs[0]["dtype"])
    before = F.STACK_LAUNCHES[key + "_mse_stack_step"]
    loss = F.rendering_loss_mse_stack(*leaves, targets=targets.cuda(), **_call_kwargs(cases[0]))
    assert type(loss.grad_fn).__name__ == stem + "StepFnBackward" and F.STACK_LAUNCHES[key + "_mse_stack_step"] == before + 1
    (loss * scale).backward()
    _check_step(refs, loss.detach(), leaves, scale, "batch step")
    before = F.STACK_LAUNCHES[key + "_stack"]
    out = F.cook_torrance_stack(*_leaves(cases, refs[0]["dtype"], grad=False), **_call_kwargs(cases[0])).cpu()
    assert F.STACK_LAUNCHES[key + "_stack"] == before + 1 and out.shape == targets.shape
    for b, r in enumerate(refs):
        _check_images(r, out[b], "%s material %d forward" % (r["tag"], b))


# ------------------------------------------------------------------ 6. the localiser
@pytest.mark.parametrize("vid,entry", _pairs(["view-stack-pairs-point"], ("split_views", "saturated")) + _pairs(["camera-stack-pairs-point"], ("saturated",)))
def test_stack_step_against_the_sum_of_single_camera_steps(vid, entry):
    """The same device, the same chain rule: L single-photograph steps (camera l, light l), each divided by L.  What separates a wrong loop
    (view_terms per shot, N.V's adjoint closed per shot, one PixelAdjointT for all shots) from a wrong chain rule when something above fails."""
    from pypbr_amd import functional as F
    r = _mse_ref(entry, vid)
    case, target = r["case"], r["target"].cuda()
    _, stem = _prefix(entry)
    kw = _call_kwargs(case)
    L = case.n_lights
    fused = _leaves([case], torch.float32)
    loss = F.rendering_loss_mse_stack(*fused, targets=target, **kw)
    assert type(loss.grad_fn).__name__ == stem + "StepFnBackward"
    loss.backward()
    steps = _leaves([case], torch.float32)
    total = 0.0
    for l in range(L):
        one = F.rendering_loss_mse(*steps, target=target[l], **dict(kw, view_dir=kw["view_dir"][l] if case.per_shot else kw["view_dir"],
                                                                    light=kw["light"][l], light_intensity=kw["light_intensity"][l]))
        assert type(one.grad_fn).__name__ == "_CameraStackStepFnBackward"
        (one / L).backward()
        total += one.item() / L
    assert abs(total - loss.item()) <= 2e-6 * (1 + loss.item())
    for name, x, y in zip(MAPS, fused, steps):
        if x is not None:
            scale = float(y.grad.abs().max())
            d = float((x.grad - y.grad).abs().max())
            print("%s %-9s stack - sum of single-camera steps: %.3e, error / tolerance %.3f" % (r["tag"], name, d, d / _tol(torch.float32, scale)))
            assert d <= _tol(torch.float32, scale), (vid, name, d, scale)
