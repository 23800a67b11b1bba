"""The stack-fit step (csrc/ct_stack.hip: pbr_cook_torrance_mse_stack_fit_step; functional._MseStackFitFn): the light-stack rendering loss
with the gradients of view, lights and intensities out of the SAME pass as the map gradients.

Ground truth: float64 autograd through the ATen restatement of the reference (oracle/torch_oracle.py) of mse_loss(torch.stack(renders),
targets), over the maps AND view, lights and intensities together, built as test_gpu_light_stack._case builds its stack (fp16 maps: the exact
upcasts of the stored values).

Tolerances are the project's: loss 1e-6 (1 + loss); map gradients _tol of test_gpu_light_stack; parameter gradients -- EVERY element of view,
lights and intensities -- within 2e-5 S + 1e-9 with S the largest |g64| over the three tensors together (they are sums of the same per-pixel
colour adjoints: a view gradient of 5e-10 beside a light gradient of 3e-3 is noise, not a result).  The parameter results are fp32 sums for
fp16 maps too: the same band.  Where the unchanged composition (L one-light cook_torrance calls with the light requiring grad: the parent's
route) itself misses the band on a case, the fused form is held to twice the composition's measured error on that case, as DESIGN.md 3.14
records; nowhere else."""
import functools
import math

import pytest
import torch
import torch.nn.functional as TF

import branch_cases as BC
import torch_oracle as O
from test_gpu_gradient_branches import MAPS, _check_maps
from test_gpu_light_stack import NAMES, _tol
from test_gpu_loss_step import _maps
from test_light_stack_fit_host import param_band

pytestmark = pytest.mark.gpu

CASES = [
    # workflow, light type, L, B, H, W, dtype, intensity rows, normal       reaches
    ("metallic", "point", 3, 1, 24, 48, torch.float32, "L", True),         # pairs per lane, per-light intensity rows
    ("specular", "directional", 2, 2, 18, 40, torch.float32, 1, True),     # batch stride of targets and rows, F.normalize Jacobians, one shared intensity row
    ("converted", "directional", 4, 1, 16, 36, torch.float32, "L", True),  # the converted workflow
    ("metallic", "point", 5, 2, 15, 37, torch.float32, 1, True),           # odd width: one pixel per lane
    ("metallic", "point", 2, 1, 6, 130, torch.float32, "L", True),         # a partial tile behind a full one: lanes outside the map add nothing
    ("metallic", "point", 3, 2, 16, 64, torch.float16, 1, True),           # fp16 maps
    ("metallic", "directional", 16, 1, 12, 32, torch.float32, "L", True),  # a 99-float row
    ("metallic", "point", 1, 1, 20, 48, torch.float32, 1, True),           # a single light
    ("metallic", "point", 3, 1, 14, 44, torch.float32, "L", False),        # normal=None
]
IDS = ["%s-%s-L%d-B%d-%dx%d-%s%s" % (c[0], c[1], c[2], c[3], c[4], c[5], "f16" if c[6] == torch.float16 else "f32", "" if c[8] else "-nonormal")
       for c in CASES]
PNAMES = ("view", "lights", "intensities")


@functools.lru_cache(maxsize=None)
def _case(i):
    """Inputs and the float64 reference of case i, computed once and shared (nothing below writes into it)."""
    workflow, light_type, L, B, H, W, dtype, rows, has_normal = CASES[i]
    g = torch.Generator().manual_seed(1000 + H * W + L)          # test_gpu_light_stack's seeding rule
    maps = [None if t is None else t.to(dtype).float() for t in _maps(g, B, H, W, workflow)]        # the values the device sees
    if not has_normal:
        maps[1] = None                                                                              # the oracle takes +Z
    targets = torch.rand(B, L, 3, H, W, generator=g)
    view = torch.tensor([0.05, 0.1, 0.9])                                                           # not a unit vector: the Jacobian of F.normalize
    ang = torch.arange(L, dtype=torch.float32) * (2 * math.pi / max(L, 3)) + 0.3
    lights = torch.stack([0.55 * torch.cos(ang), 0.55 * torch.sin(ang), 0.7 + 0.02 * torch.arange(L)], 1)
    if light_type == "directional":
        lights = lights * 1.3
    intens = torch.rand(L if rows == "L" else 1, 3, generator=g) * 0.7 + 0.3
    size = 1.5 if light_type == "point" else None
    leaves = [None if t is None else t.double().requires_grad_(True) for t in maps]
    P = [t.double().requires_grad_(True) for t in (view, lights, intens)]
    per_light = P[2].expand(L, 3)
    kw64 = dict(view=P[0], light_type=light_type, light_size=size)
    images = []
    for b in range(B):
        args = [None if t is None else t[b] for t in leaves]
        render = (lambda l: O.cook_torrance_converted(args[0], args[1], args[2], args[3], light=P[1][l], intensity=per_light[l], **kw64)) \
            if workflow == "converted" else (lambda l: O.cook_torrance(*args, light=P[1][l], intensity=per_light[l], **kw64))
        images.append(torch.stack([render(l) for l in range(L)]))
    loss64 = TF.mse_loss(torch.stack(images), targets.double())
    loss64.backward()
    kw = dict(light_type=light_type, light_size=size, convert_to_diffuse_specular=(workflow == "converted"))
    return dict(maps=maps, targets=targets, kw=kw, dtype=dtype, L=L, B=B, params=(view, lights, intens), loss64=float(loss64.detach()),
                grads64=[None if t is None else t.grad for t in leaves], want=dict(zip(PNAMES, [p.grad for p in P])))


def _leaves(c, grad=True):
    return [None if t is None else t.to(c["dtype"]).cuda().requires_grad_(grad) for t in c["maps"]]


def _params(c, where=("cuda",) * 3, grad=(True,) * 3, shapes=(None,) * 3):
    return [(t if s is None else t.reshape(s)).clone().to(w).requires_grad_(g) for t, w, g, s in zip(c["params"], where, grad, shapes)]


def _call(c, leaves, params, targets=None):
    from pypbr_amd import functional as F
    return F.rendering_loss_mse_stack(*leaves, targets=c["targets"].cuda() if targets is None else targets, view_dir=params[0], light=params[1],
                                      light_intensity=params[2], **c["kw"])


def _fused(c, k=1.0, maps_grad=True, **pkw):
    """One fused call and its backward: exactly one stack-fit launch, nothing else of the stack family."""
    from pypbr_amd import functional as F
    leaves, params = _leaves(c, maps_grad), _params(c, **pkw)
    before = dict(F.STACK_LAUNCHES)
    loss = _call(c, leaves, params)
    assert loss.shape == () and type(loss.grad_fn).__name__ == "_MseStackFitFnBackward"
    after = dict(F.STACK_LAUNCHES)
    assert after["mse_stack_fit_step"] == before["mse_stack_fit_step"] + 1
    assert after["cook_torrance_stack"] == before["cook_torrance_stack"] and after["mse_stack_step"] == before["mse_stack_step"]
    (loss * k).backward()
    assert dict(F.STACK_LAUNCHES) == after                      # the backward hands the kept gradients over: no second launch
    return loss.detach(), leaves, params


def _composition_param_error(c):
    """The parent's route on the same device: L one-light cook_torrance calls with the parameters requiring grad, torch.stack, mse_loss.
    -> its worst parameter error against float64."""
    from pypbr_amd import functional as F
    leaves, (view, lights, intens) = _leaves(c), _params(c)
    per_light = intens.expand(c["L"], 3)
    images = [F.cook_torrance(*leaves, view_dir=view, light=lights[l], light_intensity=per_light[l], **c["kw"]) for l in range(c["L"])]
    TF.mse_loss(torch.stack(images, dim=-4).reshape(c["targets"].shape), c["targets"].cuda()).backward()
    return max(float((p.grad.cpu().double() - c["want"][n]).abs().max()) for n, p in zip(PNAMES, (view, lights, intens)))


def _check_params(c, params, tag, k=1.0, names=PNAMES):
    """Every element of the parameter gradients `names` (of k * loss) within the band; shapes, dtypes and devices are the leaves' own."""
    band = param_band(c["want"])
    worst = 0.0
    for n, p in zip(PNAMES, params):
        if n not in names:
            assert p.grad is None, (tag, n)
            continue
        assert p.grad is not None and p.grad.shape == p.shape and p.grad.dtype == p.dtype and p.grad.device == p.device, (tag, n)
        assert bool(torch.isfinite(p.grad).all()), (tag, n)
        want = c["want"][n].reshape(p.shape)
        worst = max(worst, float((p.grad.cpu().double() / k - want).abs().max()))
    print("%s: worst parameter error / band %.3f (S = %.3e)" % (tag, worst / band, (band - 1e-9) / 2e-5))
    if worst > band:
        comp = _composition_param_error(c)
        print("%s: the composition's error / band %.3f" % (tag, comp / band))
        if comp > band:                                         # the existing kernels miss it here: twice their error, on this case only
            band = 2.0 * comp
    assert worst <= band, (tag, worst, band)


@pytest.mark.parametrize("i", range(len(CASES)), ids=IDS)
def test_loss_map_and_parameter_gradients_against_float64(i):
    from pypbr_amd import functional as F
    c = _case(i)
    dtype = c["dtype"]
    loss, leaves, params = _fused(c)
    print("stack fit %s: loss %.9g (float64 %.9g)" % (IDS[i], loss.item(), c["loss64"]))
    assert abs(loss.item() - c["loss64"]) <= 1e-6 * (1 + c["loss64"])
    for name, x, y in zip(NAMES, leaves, c["grads64"]):
        if x is None:
            continue
        assert x.grad.dtype == dtype and x.grad.shape == x.shape
        err, scale = float((x.grad.float().cpu().double() - y).abs().max()), float(y.abs().max())
        assert err <= _tol(dtype, scale), (IDS[i], name, err, scale)
    _check_params(c, params, IDS[i])
    # the map-only step on the same inputs (lights detached): the same loss and map gradients
    again = _leaves(c)
    step = _call(c, again, _params(c, grad=(False,) * 3))
    assert type(step.grad_fn).__name__ == "_MseStackStepFnBackward"
    step.backward()
    assert abs(step.item() - loss.item()) <= 2e-6 * (1 + loss.item())
    for name, x, y in zip(NAMES, leaves, again):
        if x is not None:
            d = float((x.grad.float() - y.grad.float()).abs().max())
            assert d <= _tol(dtype, float(y.grad.float().abs().max())), (IDS[i], name, d)


def test_only_the_lights_are_fitted():
    """No map requires grad: every g_* is NULL.  A shared [3] intensity owns the sum over the lights; CPU leaves receive CPU gradients, device
    leaves device gradients of their own shapes; view on the CPU together with lights on the device."""
    c = _case(1)                                                # one shared intensity row, directional lights, B = 2
    loss, leaves, params = _fused(c, maps_grad=False, grad=(False, False, True), shapes=(None, None, (3,)))
    assert all(t is None or t.grad is None for t in leaves) and params[2].shape == (3,)
    _check_params(c, params, "shared [3] intensity alone", names=("intensities",))
    assert abs(loss.item() - c["loss64"]) <= 1e-6 * (1 + c["loss64"])
    c = _case(0)
    _, _, params = _fused(c, maps_grad=False, where=("cpu",) * 3)
    assert all(p.grad.device.type == "cpu" for p in params)
    _check_params(c, params, "CPU leaves")
    _, _, on_device = _fused(c, maps_grad=False)
    assert all(p.grad.is_cuda for p in on_device)
    _check_params(c, on_device, "device leaves")
    assert all(torch.equal(x.grad, y.grad.cpu()) for x, y in zip(params, on_device))              # the same sums wherever the leaves live
    _, _, mixed = _fused(c, maps_grad=False, where=("cpu", "cuda", "cpu"), grad=(True, True, False))
    assert mixed[0].grad.device.type == "cpu" and mixed[1].grad.is_cuda
    _check_params(c, mixed, "view on the CPU, lights on the device", names=("view", "lights"))


def test_upstream_gradient_determinism_second_backward_and_no_grad():
    from pypbr_amd import functional as F
    c = _case(0)
    l1, g1, p1 = _fused(c)
    l2, g2, p2 = _fused(c)
    assert torch.equal(l1, l2)
    assert all(torch.equal(x.grad, y.grad) for x, y in zip(p1, p2))                               # fixed summation order
    assert all(x is None or torch.equal(x.grad, y.grad) for x, y in zip(g1, g2))
    _, g3, p3 = _fused(c, k=3.0)
    for x, y in zip([t for t in g1 if t is not None] + p1, [t for t in g3 if t is not None] + p3):
        assert float((y.grad - 3.0 * x.grad).abs().max()) <= 1e-6 * (3.0 * float(x.grad.abs().max()) + 1e-12)
    _check_params(c, p3, "loss * 3", k=3.0)
    # a second backward through the same node launches again: the same gradients
    leaves, params = _leaves(c), _params(c)
    loss = _call(c, leaves, params)
    before = F.STACK_LAUNCHES["mse_stack_fit_step"]
    loss.backward(retain_graph=True)
    assert F.STACK_LAUNCHES["mse_stack_fit_step"] == before
    first = [None if t is None else t.grad.clone() for t in leaves + params]
    for t in leaves + params:
        if t is not None:
            t.grad = None
    loss.backward()
    assert F.STACK_LAUNCHES["mse_stack_fit_step"] == before + 1
    assert all(x is None or torch.equal(x, t.grad) for x, t in zip(first, leaves + params))
    # no_grad: nothing fused is launched, the value is the composition's
    before = dict(F.STACK_LAUNCHES)
    with torch.no_grad():
        plain = _call(c, _leaves(c), _params(c))
    assert plain.shape == () and not plain.requires_grad and plain.grad_fn is None
    assert F.STACK_LAUNCHES["mse_stack_fit_step"] == before["mse_stack_fit_step"] and F.STACK_LAUNCHES["mse_stack_step"] == before["mse_stack_step"]
    with torch.no_grad():
        composed = TF.mse_loss(F.cook_torrance_stack(*_leaves(c, False), view_dir=c["params"][0], light=c["params"][1],
                                                     light_intensity=c["params"][2], **c["kw"]), c["targets"].cuda())
    assert torch.equal(plain, composed)
    assert abs(plain.item() - l1.item()) <= 2e-6 * (1 + l1.item())


# ------------------------------------------------------------------ every branch of the chain rule
VARIANTS = BC.all_stack_variants()
VIDS = [BC.variant_id(n, kw) for n, kw in VARIANTS]
ENTRIES = ["stack-pairs", "stack-pairs-point", "stack-one-pixel", "stack-fp16-point"]


@pytest.mark.parametrize("entry", ENTRIES)
@pytest.mark.parametrize("name,kw", VARIANTS, ids=VIDS)
def test_parameter_gradients_on_every_branch(name, kw, entry):
    """The branch fixture in stack mode with every undecided texel filled (none may be left: the parameter gradients are sums over ALL
    pixels), target = stack_target.  `split_lights` is the case that matters: a light behind the surface hands exactly 0 to its own position
    and intensity sums while the same pixel feeds the other lights' sums.  Map gradients as test_gpu_light_stack_branches holds them (the
    loss scaled by N / 2); parameter gradients of the unscaled loss to the band."""
    from pypbr_amd import functional as F
    case, left = BC.fill_undecided(BC.build_for(entry, name, kw))
    assert left == 0.0
    tag = "%s %s fit" % (BC.variant_id(name, kw), entry)
    fp16 = BC.STACK_ENTRY_CONFIGS[entry][4]
    dtype = torch.float16 if fp16 else torch.float32
    target = BC.stack_target(entry, name, kw)
    want = BC.gradients(case, params=True, loss_target=target.double())
    loss64 = float(((want["out"] - target.double()) ** 2).mean())
    scale = target.numel() / 2.0
    leaves = [None if t is None else t.to(dtype).cuda().requires_grad_(True) for t in case.maps()]
    params = [t.float().cuda().requires_grad_(True) for t in (case.view, case.lights, case.intensities)]
    before = F.STACK_LAUNCHES["mse_stack_fit_step"]
    loss = F.rendering_loss_mse_stack(*leaves, targets=target.cuda(), view_dir=params[0], light=params[1], light_intensity=params[2],
                                      **case.product_kwargs())
    assert type(loss.grad_fn).__name__ == "_MseStackFitFnBackward" and F.STACK_LAUNCHES["mse_stack_fit_step"] == before + 1
    (loss * scale).backward()
    assert abs(loss.item() - loss64) <= 1e-6 * (1 + loss64), (tag, loss.item(), loss64)
    got = {n: t.grad.cpu() for n, t in zip(MAPS, leaves) if t is not None}
    _check_maps(case, got, {n: want[n] * scale for n in case.map_names()}, tag, fp16=fp16, stored_scale=scale)
    band = param_band(want)
    worst = max(float((p.grad.cpu().double() / scale - want[n]).abs().max()) for n, p in zip(PNAMES, params))
    print("%s: worst parameter error / band %.3f" % (tag, worst / band))
    assert all(bool(torch.isfinite(p.grad).all()) for p in params), tag
    if worst > band:                                            # the composition on the same case, as _check_params
        again = [None if t is None else t.to(dtype).cuda().requires_grad_(True) for t in case.maps()]
        ps = [t.float().cuda().requires_grad_(True) for t in (case.view, case.lights, case.intensities)]
        images = [F.cook_torrance(*again, view_dir=ps[0], light=ps[1][l], light_intensity=ps[2][l], **case.product_kwargs()) for l in range(case.n_lights)]
        TF.mse_loss(torch.stack(images), target.cuda()).backward()
        comp = max(float((p.grad.cpu().double() - want[n]).abs().max()) for n, p in zip(PNAMES, ps))
        print("%s: the composition's error / band %.3f" % (tag, comp / band))
        if comp > band:
            band = 2.0 * comp
    assert worst <= band, (tag, worst, band)


def test_a_captured_step_sees_the_lights_current_values():
    """View, lights and intensities on the device, all requiring grad: one forward + backward captured into a graph on one stream; after the
    lights are changed in place the replay gives the eager call's loss and gradients for the NEW lights."""
    c = _case(0)
    leaves, params = _leaves(c), _params(c)
    targets = c["targets"].cuda()
    live = [t for t in leaves + params if t is not None]

    def step():
        for t in live:
            t.grad = None
        loss = _call(c, leaves, params, targets)           # (already on the device: nothing inside the capture touches the host)
        loss.backward()
        return loss

    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        step()                                                  # warm-up outside the capture
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        loss = step()
    graph.replay()
    torch.cuda.synchronize()
    _check_params(c, params, "captured step, first replay")
    moved = c["params"][1] + torch.tensor([0.07, -0.05, 0.1])
    with torch.no_grad():
        params[1].copy_(moved)
    graph.replay()
    torch.cuda.synchronize()
    got = [loss.detach().clone()] + [t.grad.clone() for t in live]
    eager_leaves = _leaves(c)
    eager_params = [c["params"][0].clone().cuda().requires_grad_(True), moved.clone().cuda().requires_grad_(True),
                    c["params"][2].clone().cuda().requires_grad_(True)]
    eager = _call(c, eager_leaves, eager_params)
    eager.backward()
    want = [eager.detach()] + [t.grad for t in eager_leaves + eager_params if t is not None]
    assert all(torch.equal(x, y) for x, y in zip(got, want))
    assert not torch.equal(params[1].grad, _fused(c)[2][1].grad)                                  # and they differ from the old lights' gradients
