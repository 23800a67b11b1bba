"""Per-pixel weights in the light-stack loss steps on the device (csrc/ct_stack_weighted.hip, ct_camera_stack_weighted.hip,
ct_view_stack_weighted.hip): functional.rendering_loss_mse_stack(weights=), rendering_loss_mse(weights=), the two loss modules, and the C ABI
behind them.

The reference is float64 autograd of (w * (stack64 - targets) ** 2).mean() over the oracles the three unweighted suites use:
test_gpu_light_stack._case (and, for the parameters of the orthographic fit step, test_gpu_light_stack_fit._case, which builds its stack the
same way) re-run with the weighted mean in the place of their mse_loss; test_gpu_camera_stack._stack_oracle for the fixed camera;
test_view_stack_host.shot_oracle for one camera per shot.  The weights are tests/test_weighted_stack_host.py's populations: uniform in [0, 2),
about a quarter exactly 0, a block that is 0 in every shot.  Bands are the project's: the loss 1e-6 (1 + loss64); map gradients
test_gpu_light_stack._tol; parameter gradients test_gpu_camera._param_band.

Shapes: from the camera fixture 7 x 12 (pairs), 5 x 9 (one pixel per lane, ragged), 2 x [6 x 16] fp16 (batch stride) and the sixteen-shot 5 x 9
case; from test_gpu_light_stack.CASES 15 x 37 B = 2, 6 x 130 (a partial tile behind a full one), fp16 and no normal map.  The weights move no
rendered value, so what the host files found about these images -- off the clamps, the knee and the zero dots -- stands: no pixel is excluded."""
import ctypes
import functools
import types

import pytest
import torch

import test_gpu_light_stack as LS
import test_gpu_light_stack_fit as LSF
from test_camera_host import fixture_case
from test_gpu_camera import BY_NAME, NAMES, _kw, _param_band
from test_gpu_camera_stack import _stack_oracle
from test_gpu_write_guards import Guards
from test_view_stack_host import cameras_of, shot_oracle, sixteen_shots
from test_weighted_stack_host import per_shot_weights, shared_weights, weight_seed, zero_block

pytestmark = pytest.mark.gpu

_tol = LS._tol
FIXTURE = ["A_converted_point_3", "B_metallic_directional_3", "C_converted_point_3_f16", "B_specular_point_16"]
ORTHO = {"step": [3, 4, 5, 9], "fit": [3, 4, 5, 8]}      # 15 x 37 B = 2, 6 x 130, fp16, no normal: in test_gpu_light_stack.CASES / test_gpu_light_stack_fit.CASES
STEP_CASES = [("ortho", i) for i in ORTHO["step"]] + [(f, n) for f in ("camera", "view") for n in FIXTURE]
FIT_CASES = [("ortho", i) for i in ORTHO["fit"]] + [(f, n) for f in ("camera", "view") for n in FIXTURE]
COUNTER = {"ortho": "weighted_mse_stack_%s", "camera": "camera_weighted_mse_stack_%s", "view": "view_weighted_mse_stack_%s"}
PLAIN_COUNTER = {"ortho": "mse_stack_%s", "camera": "camera_mse_stack_%s", "view": "view_mse_stack_%s"}
GRAD_FN = {"ortho": "_MseStack%sFnBackward", "camera": "_CameraStack%sFnBackward", "view": "_ViewStack%sFnBackward"}
_id = lambda case: "%s-%s" % case


def _weights(lead, H, W, plane):
    if plane == "ones":
        return torch.ones(*lead, 1, H, W)
    if plane == "shared":
        return shared_weights(lead[:-1], H, W, weight_seed(lead[:-1], H, W))
    return per_shot_weights(lead, H, W, weight_seed(lead, H, W))


def _weighted_mean(w):
    return lambda stack, targets: (w.double() * (stack - targets) ** 2).mean()


@functools.lru_cache(maxsize=None)
def _reference(family, key, plane="per_shot", fit=False):
    """Float64 autograd of the weighted mean for one case, computed once and shared (nothing below writes into it): maps as the device sees
    them, the library's keyword arguments with host parameters, targets, weights, the loss, the gradients of the maps and -- except for the
    orthographic step cases, whose oracle holds the parameters constant -- of view / cameras, lights and intensities."""
    if family == "ortho":
        module = LSF if fit else LS
        L, B, H, W = module.CASES[key][2:6]
        w = _weights((B, L), H, W, plane)
        real = module.TF
        module.TF = types.SimpleNamespace(mse_loss=_weighted_mean(w))      # the suite's own oracle, its mean replaced by the weighted one
        try:
            c = module._case.__wrapped__(key)
        finally:
            module.TF = real
        ref = dict(name=module.IDS[key], maps=c["maps"], targets=c["targets"], weights=w, dtype=c["dtype"], L=L, loss64=c["loss64"],
                   grads64=c["grads64"], stack64=c.get("stack64"), params=None, params64=None, kw=dict(c["kw"]))
        if fit:
            ref.update(params=dict(zip(LSF.PNAMES, c["params"])), params64=c["want"],
                       kw=dict(c["kw"], view_dir=c["params"][0], light=c["params"][1], light_intensity=c["params"][2]))
        return ref
    c = sixteen_shots() if key == "B_specular_point_16" else fixture_case(BY_NAME[key])
    view = c.get("cameras", cameras_of(c)) if family == "view" else c["C"]
    leaves = [None if t is None else t.float().double().requires_grad_(True) for t in c["maps"]]
    params = [t.double().requires_grad_(True) for t in (view, c["lights_t"], c["intens_t"])]
    if family == "view":
        stack64 = shot_oracle(c, torch.float64, maps=leaves, cameras=params[0], lights=params[1], intens=params[2])
    else:
        stack64 = _stack_oracle(c, torch.float64, maps=leaves, camera=params[0], lights=params[1], intens=params[2])
    targets = torch.rand(stack64.shape, generator=torch.Generator().manual_seed(811 + len(key)))
    w = _weights(tuple(stack64.shape[:-3]), *stack64.shape[-2:], plane)
    loss64 = _weighted_mean(w)(stack64, targets.double())
    loss64.backward()
    return dict(name=key, maps=c["maps"], targets=targets, weights=w, dtype=torch.float16 if c.get("f16") else torch.float32, L=c["L"],
                loss64=float(loss64.detach()), grads64=[None if t is None else t.grad for t in leaves], stack64=stack64.detach(),
                params=dict(view=view, lights=c["lights_t"], intensities=c["intens_t"]),
                params64=dict(view=params[0].grad, lights=params[1].grad, intensities=params[2].grad), kw=_kw(c, view_dir=view))


def _leaves(ref, grad=True):
    return [None if t is None else t.to(ref["dtype"]).cuda().requires_grad_(grad) for t in ref["maps"]]


def _params(ref, where, grad=True):
    return {k: t.clone().to(where).requires_grad_(grad) for k, t in ref["params"].items()}


def _call(ref, leaves, params=None, weights=None, targets=None, **over):
    from pypbr_amd import functional as F
    kw = dict(ref["kw"], **over)
    if params is not None:
        kw.update(view_dir=params["view"], light=params["lights"], light_intensity=params["intensities"])
    return F.rendering_loss_mse_stack(*leaves, targets=ref["targets"].cuda() if targets is None else targets,
                                      weights=ref["weights"].cuda() if weights is None else weights, **kw)


def _moved(before):
    from pypbr_amd import functional as F
    return {k: F.STACK_LAUNCHES[k] - before[k] for k in before if F.STACK_LAUNCHES[k] != before[k]}


def _check_loss(loss, ref, tag):
    got = float(loss.detach()) if isinstance(loss, torch.Tensor) else float(loss)
    print("%s %s: loss %.9g (float64 %.9g)" % (tag, ref["name"], got, ref["loss64"]))
    assert abs(got - ref["loss64"]) <= 1e-6 * (1 + ref["loss64"]), (tag, ref["name"], got, ref["loss64"])


def _check_maps(grads, ref, tag, like=None):
    """`grads`: one gradient (or None) per map, held to the float64 gradients of `ref`."""
    for name, g, want, x in zip(NAMES, grads, ref["grads64"], like or grads):
        if want is None:
            continue
        assert g is not None and g.dtype == ref["dtype"] and g.shape == x.shape, (tag, name)
        err, scale = float((g.float().cpu().double().reshape(want.shape) - want).abs().max()), float(want.abs().max())
        print("%s %s %-9s max |hip - float64| = %.3e, tolerance %.3e (max |grad| %.3e)" % (tag, ref["name"], name, err, _tol(ref["dtype"], scale), scale))
        assert err <= _tol(ref["dtype"], scale), (tag, ref["name"], name, err, scale)


def _check_params(params, ref, tag):
    band = _param_band(ref["params64"])
    for k, p in params.items():
        assert p.grad is not None and p.grad.shape == p.shape and p.grad.dtype == p.dtype and p.grad.device == p.device, (tag, k)
        err = float((p.grad.cpu().double() - ref["params64"][k].reshape(p.shape)).abs().max())
        print("%s %s %s %-11s max |hip - float64| = %.3e, band %.3e" % (tag, ref["name"], p.device.type, k, err, band))
        assert err <= band, (tag, ref["name"], k, err, band)


# ------------------------------------------------------------------ 1. the step: one weight plane per shot
@pytest.mark.parametrize("case", STEP_CASES, ids=_id)
def test_step_loss_and_map_gradients(case):
    from pypbr_amd import functional as F
    ref = _reference(*case)
    leaves = _leaves(ref)
    before = dict(F.STACK_LAUNCHES)
    loss = _call(ref, leaves)
    assert type(loss.grad_fn).__name__ == GRAD_FN[case[0]] % "Step"
    assert _moved(before) == {COUNTER[case[0]] % "step": 1}
    after = dict(F.STACK_LAUNCHES)
    loss.backward()
    assert F.STACK_LAUNCHES == after                            # forward kept the gradients: backward launches nothing
    _check_loss(loss, ref, "step")
    _check_maps([None if x is None else x.grad for x in leaves], ref, "step", leaves)


# ------------------------------------------------------------------ 2. the fit step
@pytest.mark.parametrize("maps_too", [True, False], ids=["with_maps", "parameters_only"])
@pytest.mark.parametrize("case", FIT_CASES, ids=_id)
def test_fit_step_on_host_parameters(case, maps_too):
    from pypbr_amd import functional as F
    ref = _reference(*case, fit=True)
    leaves, params = _leaves(ref, maps_too), _params(ref, "cpu")
    before = dict(F.STACK_LAUNCHES)
    loss = _call(ref, leaves, params)
    assert type(loss.grad_fn).__name__ == GRAD_FN[case[0]] % "Fit"
    assert _moved(before) == {COUNTER[case[0]] % "fit_step": 1}
    after = dict(F.STACK_LAUNCHES)
    loss.backward()
    assert F.STACK_LAUNCHES == after
    _check_loss(loss, ref, "fit")
    if case == ("view", "B_specular_point_16"):
        assert params["view"].grad.shape == (16, 3) and sum(p.grad.numel() for p in params.values()) == 9 * 16
    _check_params(params, ref, "fit")                           # every element: all 9 x 16 at L = 16 for the view family
    if maps_too:
        _check_maps([None if x is None else x.grad for x in leaves], ref, "fit", leaves)
    else:
        assert all(x is None or x.grad is None for x in leaves)


@pytest.mark.parametrize("case", [("ortho", 4), ("camera", "C_converted_point_3_f16"), ("view", "A_converted_point_3")], ids=_id)
def test_fit_step_on_device_parameters(case):
    ref = _reference(*case, fit=True)
    leaves, params = _leaves(ref), _params(ref, "cuda")
    loss = _call(ref, leaves, params)
    assert type(loss.grad_fn).__name__ == GRAD_FN[case[0]] % "Fit"
    loss.backward()
    _check_loss(loss, ref, "fit, device parameters")
    _check_params(params, ref, "fit, device parameters")
    _check_maps([None if x is None else x.grad for x in leaves], ref, "fit, device parameters", leaves)


# ------------------------------------------------------------------ 3. one plane for all shots
@pytest.mark.parametrize("case", [("ortho", 3), ("ortho", 4), ("camera", "A_converted_point_3"), ("camera", "C_converted_point_3_f16"),
                                  ("view", "B_specular_point_16"), ("view", "C_converted_point_3_f16")], ids=_id)
def test_one_plane_for_all_shots(case):
    """[1,1,H,W] / [B,1,1,H,W]: held to the float64 reference of that plane broadcast over the L shots, step and fit step."""
    from pypbr_amd import functional as F
    ref = _reference(*case, plane="shared", fit=True)
    assert ref["weights"].shape[-4] == 1 and ref["L"] > 1 and ref["weights"].dim() == ref["targets"].dim()
    leaves = _leaves(ref)
    before = dict(F.STACK_LAUNCHES)
    loss = _call(ref, leaves)
    assert _moved(before) == {COUNTER[case[0]] % "step": 1}
    loss.backward()
    _check_loss(loss, ref, "one plane, step")
    _check_maps([None if x is None else x.grad for x in leaves], ref, "one plane, step", leaves)
    expanded = _leaves(ref)
    full = ref["weights"].expand(*ref["targets"].shape[:-3], 1, *ref["targets"].shape[-2:]).contiguous()
    again = _call(ref, expanded, weights=full.cuda())
    again.backward()
    assert abs(again.item() - loss.item()) <= 1e-6 * (1 + ref["loss64"])
    leaves, params = _leaves(ref), _params(ref, "cpu")
    loss = _call(ref, leaves, params)
    assert type(loss.grad_fn).__name__ == GRAD_FN[case[0]] % "Fit"
    loss.backward()
    _check_loss(loss, ref, "one plane, fit")
    _check_params(params, ref, "one plane, fit")
    _check_maps([None if x is None else x.grad for x in leaves], ref, "one plane, fit", leaves)


# ------------------------------------------------------------------ 4. exact zeros
@pytest.mark.parametrize("case", [("ortho", 3), ("ortho", 5), ("camera", "B_metallic_directional_3"), ("camera", "C_converted_point_3_f16"),
                                  ("view", "A_converted_point_3"), ("view", "C_converted_point_3_f16")], ids=_id)
def test_zero_weights_give_exactly_zero_gradients(case):
    """At the pixels whose weight is 0 in every shot, every map gradient plane is == 0 (fp32 and fp16 maps), from the step and the fit step."""
    ref = _reference(*case, fit=True)
    block = zero_block(*ref["targets"].shape[-2:]).cuda()
    assert int(block.sum()) > 0 and bool((ref["weights"][..., block.cpu()] == 0).all())
    for params in (None, _params(ref, "cpu")):
        leaves = _leaves(ref)
        _call(ref, leaves, params).backward()
        for name, x in zip(NAMES, leaves):
            if x is not None:
                at = x.grad[..., block]
                assert at.numel() > 0 and bool((at == 0).all()), (case, name, float(at.float().abs().max()))
                assert bool((x.grad[..., ~block] != 0).any()), (case, name)


# ------------------------------------------------------------------ 5. all-ones weights
@pytest.mark.parametrize("case", [("ortho", 3), ("ortho", 5), ("camera", "A_converted_point_3"), ("view", "C_converted_point_3_f16")], ids=_id)
def test_all_ones_weights_meet_the_unweighted_reference(case):
    """w = 1 everywhere: the weighted call is held to the UNWEIGHTED suites' own float64 references, in the same bands; how far it is from the
    unweighted fused call is printed (another kernel: w d d and d (scale w) round like d d and d scale only where w = 1 is exact, which it is)."""
    from pypbr_amd import functional as F
    import test_gpu_camera_stack as CS
    import test_gpu_view_stack as VS
    family, key = case
    ref = _reference(family, key, plane="ones")
    plain = LS._case(key) if family == "ortho" else (CS if family == "camera" else VS)._reference(key)
    held = dict(ref, loss64=plain["loss64"], grads64=plain["grads64"], targets=plain["targets"])
    leaves = _leaves(held)
    before = dict(F.STACK_LAUNCHES)
    loss = _call(held, leaves)
    assert _moved(before) == {COUNTER[family] % "step": 1}
    loss.backward()
    _check_loss(loss, held, "all ones")
    _check_maps([None if x is None else x.grad for x in leaves], held, "all ones", leaves)
    unweighted = _leaves(held)
    before = dict(F.STACK_LAUNCHES)
    base = F.rendering_loss_mse_stack(*unweighted, targets=held["targets"].cuda(), **held["kw"])
    assert _moved(before) == {PLAIN_COUNTER[family] % "step": 1}          # weights=None: the unweighted kernel, the unweighted counter
    base.backward()
    worst = max(float((x.grad.float() - y.grad.float()).abs().max()) for x, y in zip(leaves, unweighted) if x is not None)
    print("all ones %s-%s: |weighted - unweighted| loss %.3e, largest gradient difference %.3e" % (family, key, abs(float(loss) - float(base)), worst))


# ------------------------------------------------------------------ 6. determinism
@pytest.mark.parametrize("case", [("ortho", 3), ("camera", "A_converted_point_3"), ("view", "B_specular_point_16")], ids=_id)
def test_two_identical_weighted_fit_calls_agree_bit_for_bit(case):
    ref = _reference(*case, fit=True)
    got = []
    for _ in range(2):
        leaves, params = _leaves(ref), _params(ref, "cpu")
        loss = _call(ref, leaves, params)
        loss.backward()
        got.append([loss.detach()] + [t.grad for t in leaves if t is not None] + [p.grad for p in params.values()])
    assert len(got[0]) >= 7
    for x, y in zip(*got):
        assert torch.equal(x, y)
    # differentiated a second time the step is evaluated again, with the saved weights: the same bits, accumulated
    leaves, params = _leaves(ref), _params(ref, "cpu")
    loss = _call(ref, leaves, params)
    loss.backward(retain_graph=True)
    loss.backward()
    twice = [t.grad for t in leaves if t is not None] + [p.grad for p in params.values()]
    for x, y in zip(got[0][1:], twice):
        assert torch.equal(x + x, y)


# ------------------------------------------------------------------ 7. fallbacks
@pytest.mark.parametrize("case", [("ortho", 4), ("camera", "A_converted_point_3"), ("view", "C_converted_point_3_f16")], ids=_id)
def test_weights_that_require_grad_take_the_composition(case):
    from pypbr_amd import functional as F
    ref = _reference(*case)
    leaves = _leaves(ref)
    w = ref["weights"].cuda().requires_grad_(True)
    before = dict(F.STACK_LAUNCHES)
    loss = _call(ref, leaves, weights=w)
    assert "Stack" not in type(loss.grad_fn).__name__
    loss.backward()
    assert not any(k for k in _moved(before) if "weighted" in k or "mse_stack" in k), _moved(before)
    _check_loss(loss, ref, "composition")
    _check_maps([None if x is None else x.grad for x in leaves], ref, "composition", leaves)
    want = ((ref["stack64"] - ref["targets"].double()) ** 2).sum(dim=-3, keepdim=True) / ref["targets"].numel()
    err, scale = float((w.grad.cpu().double() - want).abs().max()), float(want.abs().max())
    print("weights.grad %s-%s: max |hip - float64| = %.3e (max %.3e)" % (case + (err, scale)))
    assert w.grad.shape == w.shape and err <= _tol(torch.float32, scale), (case, err, scale)
    # ... and agrees with the fused route
    fused = _leaves(ref)
    one_pass = _call(ref, fused)
    one_pass.backward()
    assert abs(float(one_pass) - float(loss)) <= 1e-6 * (1 + float(loss))
    for name, x, y in zip(NAMES, fused, leaves):
        if x is not None:
            assert float((x.grad.float() - y.grad.float()).abs().max()) <= _tol(ref["dtype"], float(y.grad.float().abs().max())), (case, name)


def test_tiled_maps_take_the_composition():
    """tile=2 has no one-pass stack form: the tiled stack, then the weighted mean -- the weights in the TARGETS' H x W."""
    from pypbr_amd import functional as F
    ref = _reference("ortho", 3)
    H, W = ref["targets"].shape[-2:]
    g = torch.Generator().manual_seed(3)
    targets = torch.rand(*ref["targets"].shape[:-2], 2 * H, 2 * W, generator=g).cuda()
    w = per_shot_weights(tuple(targets.shape[:-3]), 2 * H, 2 * W, 9).cuda()
    leaves = _leaves(ref)
    before = dict(F.STACK_LAUNCHES)
    loss = _call(ref, leaves, weights=w, targets=targets, tile=2)
    assert "Stack" not in type(loss.grad_fn).__name__
    loss.backward()
    assert not any("weighted" in k for k in _moved(before)), _moved(before)
    by_hand = _leaves(ref)
    stack = F.cook_torrance_stack(*by_hand, tile=2, **ref["kw"])
    want = (w * (stack.float() - targets) ** 2).mean()
    want.backward()
    assert abs(float(loss) - float(want)) <= 1e-6 * (1 + float(want))
    for name, x, y in zip(NAMES, leaves, by_hand):
        if x is not None:
            assert float((x.grad.float() - y.grad.float()).abs().max()) <= _tol(ref["dtype"], float(y.grad.float().abs().max())), name
    with pytest.raises(ValueError, match="weights must be"):
        _call(ref, _leaves(ref), targets=targets, tile=2)       # weights in the maps' H x W


# ------------------------------------------------------------------ 8. the loss modules
def test_the_loss_modules_reach_the_weighted_routes():
    from pypbr_amd import functional as F
    from pypbr_amd.losses import MultiLightRenderingLoss, RenderingLoss
    from pypbr_amd.materials import BasecolorMetallicMaterial
    from test_gpu_loss_step import _maps
    g = torch.Generator().manual_seed(23)
    H, W, L = 10, 14, 3
    a, n, r, m, _ = [None if t is None else t[0] for t in _maps(g, 1, H, W, "metallic")]
    leaves = {"albedo": a.cuda().requires_grad_(True), "roughness": r.cuda().requires_grad_(True), "metallic": m.cuda().requires_grad_(True)}
    mat = BasecolorMetallicMaterial(albedo=leaves["albedo"], normal=None, roughness=leaves["roughness"], metallic=leaves["metallic"],
                                    device=torch.device("cuda"))
    mat._maps["normal"] = torch.nn.functional.normalize(n, dim=0).cuda()
    lights = torch.tensor([[0.1, 0.1, 1.0], [-0.4, 0.2, 0.7], [0.3, -0.3, 0.9]])
    intens = torch.tensor([[1.0, 0.9, 0.8], [0.4, 0.5, 0.6], [0.3, 0.35, 0.3]])
    photos = torch.rand(L, 3, H, W, generator=g).cuda()
    w = per_shot_weights((L,), H, W, 5).cuda()
    for view_type, view, step, plain in (("directional", torch.tensor([0.0, 0.0, 1.0]), "weighted_mse_stack_step", "mse_stack_step"),
                                         ("point", torch.tensor([0.0, 0.1, 0.8]), "camera_weighted_mse_stack_step", "camera_mse_stack_step"),
                                         ("point", torch.tensor([[0.0, 0.1, 0.8], [0.1, 0.0, 0.7], [-0.1, 0.0, 0.9]]), "view_weighted_mse_stack_step",
                                          "view_mse_stack_step")):
        crit = MultiLightRenderingLoss("point", view, lights, intens, 1.5, view_type=view_type)
        before = dict(F.STACK_LAUNCHES)
        loss = crit(mat, photos, weights=w)
        assert _moved(before) == {step: 1}, (view_type, _moved(before))
        with torch.no_grad():
            stack = crit._render(mat)
        want = float((w * (stack - photos) ** 2).mean())
        assert abs(float(loss) - want) <= 2e-6 * (1 + want)
        loss.backward()
        before = dict(F.STACK_LAUNCHES)
        crit(mat, photos)                                       # without weights every counter moves as before
        assert _moved(before) == {plain: 1}, (view_type, _moved(before))
    for view_type, view, step in (("directional", torch.tensor([0.0, 0.0, 1.0]), "weighted_mse_stack_step"),
                                  ("point", torch.tensor([0.0, 0.1, 0.8]), "camera_weighted_mse_stack_step")):
        crit = RenderingLoss("point", view, lights[0], intens[0], 1.5, view_type=view_type)
        before = dict(F.STACK_LAUNCHES)
        loss = crit(mat, photos[0], weights=w[0])
        assert _moved(before) == {step: 1}, (view_type, _moved(before))
        with torch.no_grad():
            image = crit.brdf(mat, view, lights[0], intens[0], 1.5)
        want = float((w[0] * (image - photos[0]) ** 2).mean())
        assert abs(float(loss) - want) <= 2e-6 * (1 + want)
        before = dict(F.STACK_LAUNCHES)
        plain = crit(mat, photos[0])
        assert not any("weighted" in k for k in _moved(before))
        assert type(plain.grad_fn).__name__ == ("_MseStepFnBackward" if view_type == "directional" else "_CameraStackStepFnBackward")


# ------------------------------------------------------------------ 9. the single photograph
@pytest.mark.parametrize("family,key", [("ortho", 7), ("camera", "A_metallic_point_1"), ("camera", "B_specular_point_1")])
def test_single_photograph(family, key):
    """rendering_loss_mse(weights=) in both view types: the L = 1 stack step against the float64 reference at L = 1."""
    from pypbr_amd import functional as F
    ref = _reference(family, key)
    assert ref["L"] == 1
    kw = dict(ref["kw"])
    if family == "ortho":
        kw.update(light=kw["light"][0], light_intensity=kw["light_intensity"].reshape(-1, 3)[0])
    leaves = _leaves(ref)
    before = dict(F.STACK_LAUNCHES)
    loss = F.rendering_loss_mse(*leaves, target=ref["targets"].squeeze(-4).cuda(), weights=ref["weights"].squeeze(-4).cuda(), **kw)
    assert _moved(before) == {COUNTER[family] % "step": 1}
    loss.backward()
    _check_loss(loss, ref, "single photograph")
    _check_maps([None if x is None else x.grad for x in leaves], ref, "single photograph", leaves)
    before = dict(F.STACK_LAUNCHES)
    plain = F.rendering_loss_mse(*_leaves(ref), target=ref["targets"].squeeze(-4).cuda(), **kw)      # without weights: where it went before
    assert type(plain.grad_fn).__name__ == ("_MseStepFnBackward" if family == "ortho" else "_CameraStackStepFnBackward")
    assert not any("weighted" in k for k in _moved(before))


# ------------------------------------------------------------------ 10. guard bands
@pytest.mark.parametrize("case", [("ortho", 3), ("camera", "B_metallic_directional_3"), ("view", "C_converted_point_3_f16")], ids=_id)
def test_every_written_buffer_sits_between_untouched_guards(case):
    """The gradients, g_params, the loss and the workspace (exactly the queried bytes) of the weighted step and fit step, through the C ABI,
    with the weights themselves a guarded input."""
    from pypbr_amd import _native as N
    from pypbr_amd import functional as F
    family, key = case
    ref = _reference(family, key, fit=True)
    lib = N.lib()
    stream = torch.cuda.current_stream().cuda_stream
    H, W = ref["targets"].shape[-2:]
    L = ref["L"]
    batched = ref["maps"][0].dim() == 4
    B = ref["maps"][0].shape[0] if batched else 1
    ptr = lambda t: None if t is None else t.data_ptr()
    kw = dict(ref["kw"])
    if family == "view":
        kw["view_dir"] = [0.0, 0.0, 1.0]                        # the plan's own view is not read
    kind = {"ortho": "", "camera": "camera_", "view": "view_"}[family]
    queries = {"ortho": lib.pbr_mse_stack_fit_workspace_bytes, "camera": lib.pbr_camera_mse_stack_fit_workspace_bytes,
               "view": lib.pbr_view_mse_stack_fit_workspace_bytes}
    for fit in (False, True):
        g = Guards()
        views = [None if t is None else g.input((t if batched else t.unsqueeze(0)).to(ref["dtype"])) for t in ref["maps"]]
        targets = g.input(ref["targets"].reshape(B, L, 3, H, W))
        weights = g.input(ref["weights"].reshape(B, L, H, W))
        plan = F._step_plan(views, kw)
        bufs = [g.output((B, ch, H, W), ref["dtype"]) if t is not None else None for t, ch in zip(views, (3, 3, 1, 1, 3))]
        loss = g.output((1,))
        nbytes = (queries[family] if fit else lib.pbr_mse_step_workspace_bytes)(ctypes.byref(plan.desc))
        assert nbytes > 0
        ws = g.workspace(nbytes)
        gp = g.output(((9 if family == "view" else 6) * L + (0 if family == "view" else 3),)) if fit else None
        cameras = (F._camera_rows(ref["params"]["view"], L, torch.device("cuda"))[0], None) if family == "view" else ()
        entry = getattr(lib, "pbr_cook_torrance_%sweighted_mse_stack_%s" % (kind, "fit_step" if fit else "step"))
        N.check(entry(ctypes.byref(plan.desc), *cameras, targets.data_ptr(), weights.data_ptr(), L * H * W, H * W, *[ptr(b) for b in bufs],
                      *([gp.data_ptr()] if fit else []), loss.data_ptr(), ws.data_ptr(), stream))
        g.check((case, "fit" if fit else "step"))
        _check_loss(loss[0], ref, "guarded")
        _check_maps([None if b is None else (b if batched else b[0]) for b in bufs], ref, "guarded")
        if fit:
            flat = torch.cat([ref["params64"][k].reshape(-1) for k in ("view", "lights", "intensities")])
            if family == "ortho" and flat.numel() != gp.numel():       # one shared intensity row: the entry point leaves one row per light
                flat = None
            if flat is not None:
                assert float((gp.cpu().double() - flat).abs().max()) <= _param_band(ref["params64"])
