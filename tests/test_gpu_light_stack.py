"""Light stacks (csrc/ct_stack.hip): L images of one material batch, one per light, and the rendering loss over all of them as ONE pass --
pbr_cook_torrance_stack, pbr_cook_torrance_mse_stack_step, functional.cook_torrance_stack / rendering_loss_mse_stack,
losses.MultiLightRenderingLoss.  Held against float64 autograd of mse_loss(torch.stack(oracle renders), targets) through the ATen restatement
of the reference (oracle/torch_oracle.py), against the composition on the same device, and (L = 1) against the one-light step.

The L = 16 case also measures how fp32 rounding grows over sixteen summed adjoints, fused against sixteen one-light steps with autograd's
accumulation; the figures it prints are quoted in DESIGN.md 3.14."""
import functools
import math

import pytest
import torch
import torch.nn.functional as TF

import torch_oracle as O
from test_gpu_loss_step import _maps
from test_gpu_parity import TRACK

pytestmark = pytest.mark.gpu

CASES = [
    # workflow, light type, L, B, H, W, dtype                      reaches
    ("metallic", "point", 3, 1, 24, 48, torch.float32),          # two pixels per lane
    ("specular", "directional", 2, 2, 18, 40, torch.float32),    # the batch stride of the stack
    ("converted", "directional", 4, 1, 16, 36, torch.float32),   # the converted workflow
    ("metallic", "point", 5, 2, 15, 37, torch.float32),          # odd width: one pixel per lane
    ("metallic", "point", 2, 1, 6, 130, torch.float32),          # a partial tile behind a full one
    ("metallic", "point", 3, 2, 16, 64, torch.float16),          # fp16 maps
    ("specular", "point", 2, 1, 12, 48, torch.float16),          # fp16 maps, specular workflow
    ("metallic", "point", 1, 1, 20, 48, torch.float32),          # a single light
    ("metallic", "directional", 16, 1, 12, 32, torch.float32),   # the maximum light count
    ("metallic", "point", 3, 1, 14, 44, torch.float32),          # normal=None: the kernels shade +Z (NO_NORMAL below)
]
NO_NORMAL = (len(CASES) - 1,)
IDS = ["%s-%s-L%d-B%d-%dx%d-%s%s" % (c[0], c[1], c[2], c[3], c[4], c[5], "f16" if c[6] == torch.float16 else "f32", "-nonormal" if i in NO_NORMAL else "")
       for i, c in enumerate(CASES)]
NAMES = ("albedo", "normal", "roughness", "metallic", "specular")


def _tol(dtype, scale):
    return (2e-5 if dtype == torch.float32 else 2e-3) * (scale + 1e-12) + 1e-9


@functools.lru_cache(maxsize=None)
def _case(i):
    """Inputs and the float64 reference of case i, computed once and shared (nothing below writes into it).  Even cases carry one intensity
    row per light, odd cases a single row shared by all lights."""
    workflow, light_type, L, B, H, W, dtype = CASES[i]
    g = torch.Generator().manual_seed(1000 + H * W + L)          # test_gpu_loss_step's own seeding rule
    maps = [None if t is None else t.to(dtype).float() for t in _maps(g, B, H, W, workflow)]        # the values the device sees
    if i in NO_NORMAL:
        maps[1] = None                                                                              # the oracle takes +Z
    targets = torch.rand(B, L, 3, H, W, generator=g)                                                # a different image per light
    view = torch.tensor([0.05, 0.1, 0.9])
    ang = torch.arange(L, dtype=torch.float32) * (2 * math.pi / max(L, 3)) + 0.3
    lights = torch.stack([0.55 * torch.cos(ang), 0.55 * torch.sin(ang), 0.7 + 0.02 * torch.arange(L)], 1)     # distinct
    if light_type == "directional":
        lights = lights * 1.3
    intens = torch.rand(L if i % 2 == 0 else 1, 3, generator=g) * 0.7 + 0.3
    size = 1.5 if light_type == "point" else None
    leaves = [None if t is None else t.double().requires_grad_(True) for t in maps]
    kw64 = dict(view=view.double(), light_type=light_type, light_size=size)
    per_light = intens.double().expand(L, 3)
    images = []
    for b in range(B):
        args = [None if t is None else t[b] for t in leaves]
        row = []
        for l in range(L):
            if workflow == "converted":
                row.append(O.cook_torrance_converted(args[0], args[1], args[2], args[3], light=lights[l].double(), intensity=per_light[l], **kw64))
            else:
                row.append(O.cook_torrance(*args, light=lights[l].double(), intensity=per_light[l], **kw64))
        images.append(torch.stack(row))
    stack64 = torch.stack(images)
    loss64 = TF.mse_loss(stack64, targets.double())
    loss64.backward()
    kw = dict(view_dir=view, light=lights, light_intensity=intens, light_type=light_type, light_size=size,
              convert_to_diffuse_specular=(workflow == "converted"))
    return dict(maps=maps, targets=targets, kw=kw, dtype=dtype, L=L, B=B, stack64=stack64.detach(), loss64=float(loss64.detach()),
                grads64=[None if t is None else t.grad for t in leaves])


def _leaves(c, want=(True,) * 5):
    return [None if t is None else t.to(c["dtype"]).cuda().requires_grad_(w) for t, w in zip(c["maps"], want)]


def _fused(c, k=1.0, want=(True,) * 5):
    from pypbr_amd import functional as F
    leaves = _leaves(c, want)
    before = F.STACK_LAUNCHES["mse_stack_step"]
    loss = F.rendering_loss_mse_stack(*leaves, targets=c["targets"].cuda(), **c["kw"])
    assert loss.shape == () and type(loss.grad_fn).__name__ == "_MseStackStepFnBackward"
    assert F.STACK_LAUNCHES["mse_stack_step"] == before + 1                # one step call for all L lights
    (loss * k).backward()
    return loss.detach(), leaves


@pytest.mark.parametrize("i", range(len(CASES)), ids=IDS)
def test_forward_stack_every_image_against_float64(i):
    from pypbr_amd import functional as F
    c = _case(i)
    workflow, light_type, L, B, H, W, dtype = CASES[i]
    maps = [None if t is None else t.to(dtype).cuda() for t in c["maps"]]
    before = F.STACK_LAUNCHES["cook_torrance_stack"]
    out = F.cook_torrance_stack(*maps, **c["kw"])
    assert out.shape == (B, L, 3, H, W) and out.dtype == torch.float32 and not out.requires_grad
    assert F.STACK_LAUNCHES["cook_torrance_stack"] == before + 1           # one launch for all L images
    err = (out.cpu().double() - c["stack64"]).abs()
    per_image = err.amax(dim=(0, 2, 3, 4))
    print("forward stack %s: max |hip - ref64| per light %s" % (IDS[i], ["%.2e" % float(e) for e in per_image]))
    assert float(err.max()) <= TRACK, (IDS[i], float(err.max()))
    if B == 1:                                                   # unbatched maps give [L,3,H,W]: the same values
        single = F.cook_torrance_stack(*[None if t is None else t[0] for t in maps], **c["kw"])
        assert single.shape == (L, 3, H, W) and torch.equal(single, out[0])


@pytest.mark.parametrize("i", range(len(CASES)), ids=IDS)
def test_loss_and_summed_gradients_against_float64_and_the_composition(i):
    from pypbr_amd import functional as F
    c = _case(i)
    workflow, light_type, L, B, H, W, dtype = CASES[i]
    loss, leaves = _fused(c)
    print("stack step %s: loss %.9g (float64 %.9g)" % (IDS[i], loss.item(), c["loss64"]))
    assert abs(loss.item() - c["loss64"]) <= 1e-6 * (1 + c["loss64"])
    fused_err = {}
    for name, x, y in zip(NAMES, leaves, c["grads64"]):
        if x is None:
            continue
        assert x.grad.dtype == dtype and x.grad.shape == x.shape
        fused_err[name] = (float((x.grad.float().cpu().double() - y).abs().max()), float(y.abs().max()))
    comp_err = None
    if L == 16:
        # what the parent commit offers: sixteen one-light steps, autograd adding the sixteen gradient sets up
        steps = _leaves(c)
        per_light = c["kw"]["light_intensity"].expand(L, 3)
        kw1 = {k: v for k, v in c["kw"].items() if k not in ("light", "light_intensity")}
        for l in range(L):
            (F.rendering_loss_mse(*steps, target=c["targets"][:, l].cuda(), light=c["kw"]["light"][l], light_intensity=per_light[l], **kw1) / L).backward()
        comp_err = {name: float((x.grad.float().cpu().double() - y).abs().max()) for name, x, y in zip(NAMES, steps, c["grads64"]) if x is not None}
    for name, (err, scale) in fused_err.items():
        bound = _tol(dtype, scale)
        if comp_err is not None:
            print("L = 16 %s: fused error %.3e, sixteen steps' error %.3e, tolerance %.3e (max |grad| %.3e)" % (name, err, comp_err[name], bound, scale))
            bound = max(bound, 2.0 * comp_err[name])
        assert err <= bound, (IDS[i], name, err, scale)
    # the composition on the same device: the differentiable stack, then torch's MSE
    again = _leaves(c)
    unfused = TF.mse_loss(F.cook_torrance_stack(*again, **c["kw"]), c["targets"].cuda())
    assert type(unfused.grad_fn).__name__ != "_MseStackStepFnBackward"
    unfused.backward()
    assert abs(unfused.item() - loss.item()) <= 2e-6 * (1 + loss.item())
    for name, x, y in zip(NAMES, leaves, again):
        if x is not None:
            d = float((x.grad.float() - y.grad.float()).abs().max())
            assert d <= _tol(dtype, float(y.grad.float().abs().max())), (IDS[i], name, d)


def test_single_light_agrees_with_the_one_light_step():
    from pypbr_amd import functional as F
    i = next(k for k, c in enumerate(CASES) if c[2] == 1)
    c = _case(i)
    loss, leaves = _fused(c)
    one = _leaves(c)
    kw1 = dict(c["kw"], light=c["kw"]["light"][0], light_intensity=c["kw"]["light_intensity"][0])
    ref = F.rendering_loss_mse(*one, target=c["targets"][:, 0].cuda(), **kw1)
    assert type(ref.grad_fn).__name__ == "_MseStepFnBackward"
    ref.backward()
    assert abs(ref.item() - loss.item()) <= 2e-6 * (1 + loss.item())
    for name, x, y in zip(NAMES, leaves, one):
        if x is not None:
            d = float((x.grad - y.grad).abs().max())
            assert d <= _tol(torch.float32, float(y.grad.abs().max())), (name, d)


def test_upstream_gradient_unwanted_gradients_determinism_and_no_grad():
    from pypbr_amd import functional as F
    c = _case(0)
    l1, g1 = _fused(c)
    l2, g2 = _fused(c)
    assert torch.equal(l1, l2)
    assert all(x is None or torch.equal(x.grad, y.grad) for x, y in zip(g1, g2))                 # fixed summation order
    _, g3 = _fused(c, k=3.0)
    for x, y in zip(g1, g3):
        if x is not None:
            assert float((y.grad - 3.0 * x.grad).abs().max()) <= 1e-6 * (3.0 * float(x.grad.abs().max()) + 1e-12)
    _, gp = _fused(c, want=(True, False, False, True, False))
    assert gp[1].grad is None and gp[2].grad is None
    assert torch.equal(gp[0].grad, g1[0].grad) and torch.equal(gp[3].grad, g1[3].grad)
    with torch.no_grad():
        plain = F.rendering_loss_mse_stack(*[None if t is None else t.cuda() for t in c["maps"]], targets=c["targets"].cuda(), **c["kw"])
    assert plain.shape == () and not plain.requires_grad and plain.grad_fn is None
    assert abs(plain.item() - l1.item()) <= 2e-6 * (1 + l1.item())
    # a second backward through the same node evaluates again: same gradients
    leaves = _leaves(c)
    loss = F.rendering_loss_mse_stack(*leaves, targets=c["targets"].cuda(), **c["kw"])
    loss.backward(retain_graph=True)
    first = [None if t is None else t.grad.clone() for t in leaves]
    for t in leaves:
        if t is not None:
            t.grad = None
    loss.backward()
    assert all(x is None or torch.equal(x, t.grad) for x, t in zip(first, leaves))


def test_fallbacks_a_light_being_fitted_and_tiled_maps():
    from pypbr_amd import functional as F
    c = _case(0)
    loss, fused = _fused(c)
    # a light with requires_grad: the composition, and the light receives its gradient
    leaves = _leaves(c)
    light = c["kw"]["light"].clone().cuda().requires_grad_(True)
    fitted = F.rendering_loss_mse_stack(*leaves, targets=c["targets"].cuda(), **dict(c["kw"], light=light))
    assert type(fitted.grad_fn).__name__ != "_MseStackStepFnBackward"
    fitted.backward()
    assert light.grad is not None and light.grad.shape == light.shape and bool(torch.isfinite(light.grad).all()) and float(light.grad.abs().max()) > 0
    assert abs(fitted.item() - loss.item()) <= 2e-6 * (1 + loss.item())
    for name, x, y in zip(NAMES, fused, leaves):
        if x is not None:
            assert float((x.grad - y.grad).abs().max()) <= _tol(torch.float32, float(y.grad.abs().max())), name
    # tile=2: the composition over tiled maps; equivalent to the one-pass form over the materialised repeat, a texel owning the sum over its repeats
    g = torch.Generator().manual_seed(77)
    B, h, w, L = 1, 8, 12, 3
    small = _maps(g, B, h, w, "metallic")
    targets = torch.rand(B, L, 3, 2 * h, 2 * w, generator=g).cuda()
    kw = dict(c["kw"])
    tiled = [None if t is None else t.cuda().requires_grad_(True) for t in small]
    lt = F.rendering_loss_mse_stack(*tiled, targets=targets, tile=2, **kw)
    assert type(lt.grad_fn).__name__ != "_MseStackStepFnBackward"
    lt.backward()
    repeated = [None if t is None else t.repeat(1, 1, 2, 2).cuda().requires_grad_(True) for t in small]
    lr = F.rendering_loss_mse_stack(*repeated, targets=targets, **kw)
    assert type(lr.grad_fn).__name__ == "_MseStackStepFnBackward"
    lr.backward()
    assert abs(lt.item() - lr.item()) <= 2e-6 * (1 + lr.item())
    for name, x, y in zip(NAMES, tiled, repeated):
        if x is not None:
            folded = y.grad.reshape(B, -1, 2, h, 2, w).sum(dim=(2, 4))
            assert float((x.grad - folded).abs().max()) <= _tol(torch.float32, float(folded.abs().max())), name


def test_multi_light_rendering_loss_module():
    """losses.MultiLightRenderingLoss: a material and its rendered stack as ground truth give the same loss and gradients; with a material it
    is the tutorial's loss called once per light, averaged."""
    from pypbr_amd.losses import MultiLightRenderingLoss, RenderingLoss
    from pypbr_amd.materials import BasecolorMetallicMaterial
    g = torch.Generator().manual_seed(19)
    H, W, L = 20, 32, 3

    def material(grad):
        a, n, r, m, _ = [None if t is None else t[0] for t in _maps(g, 1, H, W, "metallic")]
        leaves = {"albedo": a.cuda().requires_grad_(grad), "roughness": r.cuda().requires_grad_(grad), "metallic": m.cuda().requires_grad_(grad)}
        mat = BasecolorMetallicMaterial(albedo=leaves["albedo"], normal=None, roughness=leaves["roughness"], metallic=leaves["metallic"],
                                        device=torch.device("cuda"))
        mat._maps["normal"] = TF.normalize(n, dim=0).cuda()
        return mat, leaves
    gt, _ = material(False)
    pred, leaves = material(True)
    view = torch.tensor([0.0, 0.0, 1.0])
    lights = torch.tensor([[0.1, 0.1, 1.0], [-0.4, 0.2, 0.7], [0.3, -0.3, 0.9]])
    intens = torch.tensor([[1.0, 0.9, 0.8], [0.4, 0.5, 0.6], [0.3, 0.35, 0.3]])
    crit = MultiLightRenderingLoss("point", view, lights, intens, 1.5)

    def grads():
        out = {k: v.grad.clone() for k, v in leaves.items()}
        for v in leaves.values():
            v.grad = None
        return out
    loss = crit(pred, gt)
    assert type(loss.grad_fn).__name__ == "_MseStackStepFnBackward"
    loss.backward()
    from_material = grads()
    with torch.no_grad():
        stack = crit._render(gt)
    assert stack.shape == (L, 3, H, W)
    again = crit(pred, stack)
    assert type(again.grad_fn).__name__ == "_MseStackStepFnBackward"
    again.backward()
    from_stack = grads()
    assert torch.equal(again.detach(), loss.detach()) and all(torch.equal(from_material[k], from_stack[k]) for k in leaves)
    total = sum(RenderingLoss("point", view, lights[l], intens[l], 1.5)(pred, gt) for l in range(L)) / L
    total.backward()
    tutorial = grads()
    assert abs(total.item() - loss.item()) <= 2e-6 * (1 + loss.item())
    for k in leaves:
        assert float((from_material[k] - tutorial[k]).abs().max()) <= _tol(torch.float32, float(tutorial[k].abs().max())), k
