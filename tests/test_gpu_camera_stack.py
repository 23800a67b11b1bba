"""Light stacks under the perspective camera on the device (csrc/ct_camera_stack.hip): functional.cook_torrance_stack,
rendering_loss_mse_stack and rendering_loss_mse with view_type="point", the loss modules, and the C ABI behind them
(pbr_cook_torrance_camera_stack, pbr_cook_torrance_camera_mse_stack_step, pbr_cook_torrance_camera_mse_stack_fit_step).

The reference is tools/camera_oracle.py, which tests/test_camera_host.py pins to tests/golden/camera.npz (upstream evaluated pixel by pixel):
image l of a stack is the oracle with light l alone.  Forward values: 1e-5 against the float32 oracle, 2e-6 against the float64 oracle
(criteria (i) and (ii); the fixture's roughness is >= 0.2).  The loss: 1e-6 (1 + loss64).  Map gradients: test_gpu_light_stack's
_tol against float64 autograd of mse_loss(stacked oracle, targets).  Camera position, lights and intensities: test_gpu_camera's _param_band,
2e-5 S + 1e-9 with S the largest float64 magnitude over the three.

The shapes are the fixture's: 7 x 12 (pairs in the steps, 4-pixel lanes forward), 5 x 9 (one-pixel lanes, ragged) and 2 x [6 x 16] fp16 maps.
None of these cases puts a per-light image value on a kink that fp32 and float64 could resolve differently (checked in float64 on the host:
no value within 3.5e-6 of the sRGB knee, the clamps are the ones test_gpu_camera's gradient tests pass through), so no pixel is excluded."""
import ctypes
import functools

import pytest
import torch

from test_camera_host import fixture_case, oracle
from test_gpu_camera import BY_NAME, NAMES, _device_maps, _kw, _param_band
from test_gpu_light_stack import _tol
from test_gpu_write_guards import Guards

pytestmark = pytest.mark.gpu

STACK_CASES = ["A_specular_directional_3", "A_converted_point_3", "A_metallic_point_1", "B_metallic_directional_3", "B_specular_point_1",
               "C_converted_point_3_f16", "C_specular_directional_3_f16"]


def _stack_oracle(c, dtype, maps=None, camera=None, lights=None, intens=None, **over):
    """[L,3,H,W] / [B,L,3,H,W]: image l is the oracle with light l alone."""
    lights = c["lights_t"] if lights is None else lights
    intens = c["intens_t"] if intens is None else intens
    images = [oracle(c, dtype, maps=maps, camera=camera, lights=lights[l:l + 1], intens=intens[l:l + 1], **over) for l in range(c["L"])]
    return torch.stack(images, dim=-4)


@functools.lru_cache(maxsize=None)
def _reference(name):
    """Float64 autograd of mse_loss(stacked oracle, targets) for one case, computed once and shared (nothing below writes into it): the
    stack in both precisions, the targets, the loss, the gradients of the maps and of camera / lights / intensities."""
    c = fixture_case(BY_NAME[name])
    leaves = [None if t is None else t.float().double().requires_grad_(True) for t in c["maps"]]
    params = [t.double().requires_grad_(True) for t in (c["C"], c["lights_t"], c["intens_t"])]
    stack64 = _stack_oracle(c, torch.float64, maps=leaves, camera=params[0], lights=params[1], intens=params[2])
    targets = torch.rand(stack64.shape, generator=torch.Generator().manual_seed(311 + len(name)))
    loss64 = torch.nn.functional.mse_loss(stack64, targets.double())
    loss64.backward()
    return dict(c, stack64=stack64.detach(), stack32=_stack_oracle(c, torch.float32), targets=targets, loss64=float(loss64.detach()),
                grads64=[None if t is None else t.grad for t in leaves],
                params64=dict(view=params[0].grad, lights=params[1].grad, intensities=params[2].grad),
                dtype=torch.float16 if c.get("f16") else torch.float32)


def _check_loss(loss, c, tag):
    got = float(loss.detach()) if isinstance(loss, torch.Tensor) else float(loss)
    print("%s %s: loss %.9g (float64 %.9g)" % (tag, c["name"], got, c["loss64"]))
    assert abs(got - c["loss64"]) <= 1e-6 * (1 + c["loss64"]), (tag, c["name"], got, c["loss64"])


def _check_map_gradients(leaves, c, tag, wanted=(True,) * 5):
    for name, x, want, on in zip(NAMES, leaves, c["grads64"], wanted):
        if x is None:
            continue
        if not on:
            assert x.grad is None, (tag, name)
            continue
        assert x.grad is not None and x.grad.dtype == c["dtype"] and x.grad.shape == x.shape, (tag, name)
        err, scale = float((x.grad.float().cpu().double() - want).abs().max()), float(want.abs().max())
        print("%s %s %-9s max |hip - float64| = %.3e, tolerance %.3e (max |grad| %.3e)" % (tag, c["name"], name, err, _tol(c["dtype"], scale), scale))
        assert err <= _tol(c["dtype"], scale), (tag, c["name"], name, err, scale)


def _check_parameters(params, c, tag, where):
    band = _param_band(c["params64"])
    for k, p in params.items():
        assert p.grad is not None and p.grad.shape == p.shape and p.grad.device.type == where, (tag, k)
        err = float((p.grad.cpu().double() - c["params64"][k]).abs().max())
        print("%s %s %s %-11s max |hip - float64| = %.3e, band %.3e" % (tag, c["name"], where, k, err, band))
        assert err <= band, (tag, c["name"], where, k, err, band)


def _params(c, where, grad=True):
    return {k: t.clone().to(where).requires_grad_(grad) for k, t in (("view", c["C"]), ("lights", c["lights_t"]), ("intensities", c["intens_t"]))}


def _loss_call(c, leaves, params=None, targets=None):
    from pypbr_amd import functional as F
    over = {} if params is None else dict(view_dir=params["view"], light=params["lights"], light_intensity=params["intensities"])
    return F.rendering_loss_mse_stack(*leaves, targets=c["targets"].cuda() if targets is None else targets, **_kw(c, **over))


# ------------------------------------------------------------------ 1. the forward stack
@pytest.mark.parametrize("name", STACK_CASES)
def test_forward_stack_parity(name):
    from pypbr_amd import functional as F
    c = _reference(name)
    before = dict(F.STACK_LAUNCHES)
    out = F.cook_torrance_stack(*_device_maps(c), **_kw(c))
    got = out.cpu()
    assert got.shape == c["stack64"].shape and got.dtype == torch.float32 and not out.requires_grad and bool(torch.isfinite(got).all())
    for l in range(c["L"]):
        image = got.select(-4, l)
        e32 = float((image - c["stack32"].select(-4, l)).abs().max())
        e64 = float((image.double() - c["stack64"].select(-4, l)).abs().max())
        print("%s image %d: max |hip - oracle32| = %.2e   max |hip - oracle64| = %.2e" % (name, l, e32, e64))
        assert e32 <= 1e-5 and e64 <= 2e-6, (name, l, e32, e64)
    if c["L"] == 3:
        assert F.STACK_LAUNCHES["camera_stack"] == before["camera_stack"] + 1
        assert F.STACK_LAUNCHES["cook_torrance_stack"] == before["cook_torrance_stack"]
    # a map that requires grad: the composition, differentiable
    before = dict(F.STACK_LAUNCHES)
    leaves = _device_maps(c, grad=True)
    composed = F.cook_torrance_stack(*leaves, **_kw(c))
    assert composed.requires_grad and F.STACK_LAUNCHES == before
    assert float((composed.detach().cpu().double() - c["stack64"]).abs().max()) <= 2e-6
    composed.sum().backward()
    assert leaves[0].grad is not None and bool(torch.isfinite(leaves[0].grad.float()).all())


# ------------------------------------------------------------------ 2. loss and map gradients
@pytest.mark.parametrize("name", STACK_CASES)
def test_loss_and_map_gradients(name):
    from pypbr_amd import functional as F
    c = _reference(name)
    leaves = _device_maps(c, grad=True)
    before = F.STACK_LAUNCHES["camera_mse_stack_step"]
    loss = _loss_call(c, leaves)
    if c["L"] == 3:
        assert type(loss.grad_fn).__name__ == "_CameraStackStepFnBackward"
        assert F.STACK_LAUNCHES["camera_mse_stack_step"] == before + 1
    after = F.STACK_LAUNCHES["camera_mse_stack_step"]
    loss.backward()
    assert F.STACK_LAUNCHES["camera_mse_stack_step"] == after       # forward kept the gradients: backward launches no step
    _check_loss(loss, c, "step")
    _check_map_gradients(leaves, c, "step")


# ------------------------------------------------------------------ 3. the fit step
@pytest.mark.parametrize("maps_too", [True, False], ids=["with_maps", "parameters_only"])
@pytest.mark.parametrize("name", STACK_CASES)
def test_fit_step_on_host_parameters(name, maps_too):
    from pypbr_amd import functional as F
    c = _reference(name)
    leaves, params = _device_maps(c, grad=maps_too), _params(c, "cpu")
    before = F.STACK_LAUNCHES["camera_mse_stack_fit_step"]
    loss = _loss_call(c, leaves, params)
    if c["L"] == 3:
        assert type(loss.grad_fn).__name__ == "_CameraStackFitFnBackward"
        assert F.STACK_LAUNCHES["camera_mse_stack_fit_step"] == before + 1
    loss.backward()
    _check_loss(loss, c, "fit")
    _check_parameters(params, c, "fit", "cpu")
    if maps_too:
        _check_map_gradients(leaves, c, "fit")
    else:
        assert all(x is None or x.grad is None for x in leaves)


def test_fit_step_on_device_parameters():
    c = _reference("A_converted_point_3")
    leaves, params = _device_maps(c, grad=True), _params(c, "cuda")
    loss = _loss_call(c, leaves, params)
    assert type(loss.grad_fn).__name__ == "_CameraStackFitFnBackward"
    loss.backward()
    _check_loss(loss, c, "fit, device parameters")
    _check_parameters(params, c, "fit", "cuda")
    _check_map_gradients(leaves, c, "fit, device parameters")


def test_one_intensity_for_all_lights_receives_the_sum():
    """A [3] intensity shared by the three lights: its gradient is the sum over the lights, shaped [3], on the CPU like the tensor."""
    from pypbr_amd import functional as F
    base = _reference("A_converted_point_3")
    c = fixture_case(BY_NAME["A_converted_point_3"])
    shared = c["intens_t"][1].clone()
    p64 = [t.double().requires_grad_(True) for t in (c["C"], c["lights_t"], shared)]
    stack64 = _stack_oracle(c, torch.float64, camera=p64[0], lights=p64[1], intens=p64[2].expand(3, 3))
    loss64 = torch.nn.functional.mse_loss(stack64, base["targets"].double())
    loss64.backward()
    want = dict(view=p64[0].grad, lights=p64[1].grad, intensities=p64[2].grad)
    params = dict(view=c["C"].clone().requires_grad_(True), lights=c["lights_t"].clone().requires_grad_(True), intensities=shared.clone().requires_grad_(True))
    loss = F.rendering_loss_mse_stack(*_device_maps(c), targets=base["targets"].cuda(),
                                      **_kw(c, view_dir=params["view"], light=params["lights"], light_intensity=params["intensities"]))
    assert type(loss.grad_fn).__name__ == "_CameraStackFitFnBackward"
    loss.backward()
    assert abs(loss.item() - loss64.item()) <= 1e-6 * (1 + loss64.item())
    band = _param_band(want)
    assert params["intensities"].grad.shape == (3,) and params["intensities"].grad.device.type == "cpu"
    for k, p in params.items():
        err = float((p.grad.double() - want[k]).abs().max())
        print("shared intensity %-11s max |hip - float64| = %.3e, band %.3e" % (k, err, band))
        assert err <= band, (k, err, band)


# ------------------------------------------------------------------ 4. a camera that lives on the device
def test_device_resident_camera_is_read_from_the_device():
    """ONE plan for two launches of the fit step: the position lives on the device, is edited in place between the launches and folded
    again on the device (RenderPlan.prepare_device_parameters: no host read); each loss is the oracle's at the camera's current value."""
    from pypbr_amd import functional as F
    c = _reference("A_converted_point_3")
    maps = _device_maps(c)
    camera = c["C"].clone().cuda()
    lights, intens = c["lights_t"].cuda(), c["intens_t"].cuda()
    kw = {k: v for k, v in _kw(c).items() if k not in ("view_dir", "light", "light_intensity")}
    plan = F._step_plan(maps, kw, (camera, lights, intens))
    assert plan.view_type == "point" and plan.desc.device_params
    targets = c["targets"].cuda()
    wanted = [t is not None for t in maps]
    _, gp1, loss1 = F._launch_loss_step("camera_fit", plan, maps, targets, wanted)
    first, gp_first = float(loss1), gp1.cpu()
    _check_loss(first, c, "device camera")
    moved = torch.tensor([-0.15, 0.25, 0.9])
    camera.copy_(moved)
    plan.prepare_device_parameters()
    _, gp2, loss2 = F._launch_loss_step("camera_fit", plan, maps, targets, wanted)
    p64 = [t.double().requires_grad_(True) for t in (moved, c["lights_t"], c["intens_t"])]
    want = torch.nn.functional.mse_loss(_stack_oracle(c, torch.float64, camera=p64[0], lights=p64[1], intens=p64[2]), c["targets"].double())
    want.backward()
    second = float(loss2)
    print("device camera moved: loss %.9g (float64 %.9g), first %.9g" % (second, want.item(), first))
    assert abs(second - want.item()) <= 1e-6 * (1 + want.item()) and abs(second - first) > 1e-4
    flat = lambda view, lights, intens: torch.cat([view, lights.reshape(-1), intens.reshape(-1)])
    at_first = flat(c["params64"]["view"], c["params64"]["lights"], c["params64"]["intensities"])
    assert float((gp_first.double() - at_first).abs().max()) <= _param_band(c["params64"])
    at_moved = dict(view=p64[0].grad, lights=p64[1].grad, intensities=p64[2].grad)
    assert float((gp2.cpu().double() - flat(*at_moved.values())).abs().max()) <= _param_band(at_moved)


# ------------------------------------------------------------------ 5. determinism
def test_two_identical_fit_calls_agree_bit_for_bit():
    from pypbr_amd import functional as F
    c = _reference("A_converted_point_3")
    maps = _device_maps(c)
    kw = {k: v for k, v in _kw(c).items() if k not in ("view_dir", "light", "light_intensity")}
    runs = []
    for _ in range(2):
        plan = F._step_plan(maps, kw, (c["C"], c["lights_t"], c["intens_t"]))
        bufs, gp, loss = F._launch_loss_step("camera_fit", plan, maps, c["targets"].cuda(), [t is not None for t in maps])
        runs.append([loss.clone(), gp.clone()] + [b.clone() for b in bufs if b is not None])
    assert len(runs[0]) >= 5
    for x, y in zip(*runs):
        assert torch.equal(x, y)
    # and through autograd
    got = []
    for _ in range(2):
        leaves, params = _device_maps(c, grad=True), _params(c, "cpu")
        loss = _loss_call(c, leaves, params)
        loss.backward()
        got.append([loss.detach()] + [t.grad for t in leaves if t is not None] + [p.grad for p in params.values()])
    for x, y in zip(*got):
        assert torch.equal(x, y)


# ------------------------------------------------------------------ 6. the single photograph, the loss modules
@pytest.mark.parametrize("name", ["A_metallic_point_1", "B_specular_point_1"])
def test_single_photograph(name):
    """rendering_loss_mse(view_type="point") with one light is the stack of one image: same loss, same gradients -- maps alone, and with the
    camera, the light and the intensity as leaves."""
    from pypbr_amd import functional as F
    c = _reference(name)
    target = c["targets"].squeeze(-4).cuda()
    kw = _kw(c, light=c["lights_t"][0], light_intensity=c["intens_t"][0])
    leaves = _device_maps(c, grad=True)
    loss = F.rendering_loss_mse(*leaves, target=target, **kw)
    loss.backward()
    _check_loss(loss, c, "rendering_loss_mse")
    _check_map_gradients(leaves, c, "rendering_loss_mse")
    leaves, params = _device_maps(c, grad=True), _params(c, "cpu")
    loss = F.rendering_loss_mse(*leaves, target=target, **_kw(c, view_dir=params["view"], light=params["lights"], light_intensity=params["intensities"]))
    loss.backward()
    _check_loss(loss, c, "rendering_loss_mse, parameters")
    _check_parameters(params, c, "rendering_loss_mse", "cpu")
    _check_map_gradients(leaves, c, "rendering_loss_mse, parameters")


def test_loss_modules_take_the_fused_route():
    """RenderingLoss (the first light's photograph) and MultiLightRenderingLoss (all three) on a material whose maps are leaves."""
    from pypbr_amd import functional as F
    from pypbr_amd.losses import MultiLightRenderingLoss, RenderingLoss
    from pypbr_amd.materials import DiffuseSpecularMaterial
    name = "A_specular_directional_3"
    c = fixture_case(BY_NAME[name])

    def material():
        leaves = _device_maps(c, grad=True)
        mat = DiffuseSpecularMaterial(albedo=leaves[0], normal=None, roughness=leaves[2], specular=leaves[4], albedo_is_srgb=c["srgb"],
                                      specular_is_srgb=c["srgb"], device=torch.device("cuda"))
        mat._maps["normal"] = leaves[1]
        return mat, leaves

    def reference(L):
        """The modules encode the result (return_srgb is upstream's default); the oracle with that, lights 0 .. L - 1."""
        leaves64 = [None if t is None else t.double().requires_grad_(True) for t in c["maps"]]
        images = [oracle(c, torch.float64, maps=leaves64, lights=c["lights_t"][l:l + 1], intens=c["intens_t"][l:l + 1], return_srgb=True) for l in range(L)]
        stack = torch.stack(images)
        targets = torch.rand(stack.shape, generator=torch.Generator().manual_seed(17 + L))
        loss64 = torch.nn.functional.mse_loss(stack, targets.double())
        loss64.backward()
        return dict(c, targets=targets, loss64=float(loss64), grads64=[None if t is None else t.grad for t in leaves64], dtype=torch.float32)

    ref = reference(1)
    mat, leaves = material()
    before = dict(F.STACK_LAUNCHES)
    crit = RenderingLoss(c["light_type"], c["C"], c["lights_t"][0], c["intens_t"][0], c["light_size"], view_type="point")
    loss = crit(mat, ref["targets"][0].cuda())
    assert F.STACK_LAUNCHES["camera_mse_stack_step"] == before["camera_mse_stack_step"] + 1
    loss.backward()
    _check_loss(loss, ref, "RenderingLoss")
    _check_map_gradients(leaves, ref, "RenderingLoss")
    ref = reference(3)
    mat, leaves = material()
    before = dict(F.STACK_LAUNCHES)
    crit = MultiLightRenderingLoss(c["light_type"], c["C"], c["lights_t"], c["intens_t"], c["light_size"], view_type="point")
    loss = crit(mat, ref["targets"].cuda())
    assert type(loss.grad_fn).__name__ == "_CameraStackStepFnBackward"
    assert F.STACK_LAUNCHES["camera_mse_stack_step"] == before["camera_mse_stack_step"] + 1
    loss.backward()
    _check_loss(loss, ref, "MultiLightRenderingLoss")
    _check_map_gradients(leaves, ref, "MultiLightRenderingLoss")


# ------------------------------------------------------------------ 7. fused against the composition
@pytest.mark.parametrize("name", STACK_CASES)
def test_fused_route_against_the_composition(name):
    """The same call forced onto the composition (targets that require grad): L camera renders, torch's MSE, L camera backwards.  The two
    agree within the tolerances each is held to against float64 -- not bit for bit: the composition rounds every image to memory."""
    from pypbr_amd import functional as F
    c = _reference(name)
    fused_leaves, fused_params = _device_maps(c, grad=True), _params(c, "cpu")
    fused = _loss_call(c, fused_leaves, fused_params)
    fused.backward()
    before = dict(F.STACK_LAUNCHES)
    leaves, params = _device_maps(c, grad=True), _params(c, "cpu")
    composed = _loss_call(c, leaves, params, targets=c["targets"].cuda().requires_grad_(True))
    assert F.STACK_LAUNCHES == before and "CameraStack" not in type(composed.grad_fn).__name__
    composed.backward()
    assert abs(fused.item() - composed.item()) <= 1e-6 * (1 + composed.item()), (name, fused.item(), composed.item())
    for nm, x, y in zip(NAMES, fused_leaves, leaves):
        if x is not None:
            scale = float(y.grad.float().abs().max())
            err = float((x.grad.float() - y.grad.float()).abs().max())
            assert err <= _tol(c["dtype"], scale), (name, nm, err, scale)
    band = 2e-5 * max(float(p.grad.abs().max()) for p in params.values()) + 1e-9
    for k in params:
        err = float((fused_params[k].grad - params[k].grad).abs().max())
        assert err <= band, (name, k, err, band)


# ------------------------------------------------------------------ 8. guard bands
@pytest.mark.parametrize("name", ["A_converted_point_3", "B_metallic_directional_3", "C_converted_point_3_f16"])
def test_every_written_buffer_sits_between_untouched_guards(name):
    """The stack, every gradient buffer, g_params, the loss and the workspaces (exactly the queried bytes), through the C ABI; then a step
    with only the albedo's and the roughness's gradients requested."""
    from pypbr_amd import _native as N
    from pypbr_amd import functional as F
    c = _reference(name)
    lib = N.lib()
    stream = torch.cuda.current_stream().cuda_stream
    H, W = c["shape"][-2:]
    L = c["L"]
    batched = c["maps"][0].dim() == 4
    B = c["maps"][0].shape[0] if batched else 1
    ptr = lambda t: None if t is None else t.data_ptr()
    channels = (3, 3, 1, 1, 3)
    byref = ctypes.byref

    g = Guards()
    maps = [None if t is None else g.input(t if batched else t.unsqueeze(0)) for t in c["maps"]]
    stack = g.output((B, L, 3, H, W))
    plan = F.plan_cook_torrance(*maps, out=stack.view(B * L, 3, H, W)[:B], **_kw(c))
    N.check(lib.pbr_cook_torrance_camera_stack(byref(plan.desc), stream))
    g.check((name, "stack"))
    want = c["stack64"] if batched else c["stack64"].unsqueeze(0)
    assert float((stack.cpu().double() - want).abs().max()) <= 2e-6

    def step(fit, only=None):
        gd = Guards()
        views = [None if t is None else gd.input(t if batched else t.unsqueeze(0)) for t in c["maps"]]
        targets = gd.input(c["targets"] if batched else c["targets"].unsqueeze(0))
        plan = F._step_plan(views, {k: v for k, v in _kw(c).items()})
        bufs = [gd.output((B, ch, H, W), c["dtype"]) if t is not None and (only is None or i in only) else None
                for i, (t, ch) in enumerate(zip(views, channels))]
        loss = gd.output((1,))
        query = lib.pbr_camera_mse_stack_fit_workspace_bytes if fit else lib.pbr_mse_step_workspace_bytes
        nbytes = query(byref(plan.desc))
        assert nbytes > 0
        ws = gd.workspace(nbytes)
        if fit:
            gp = gd.output((3 + 6 * L,))
            N.check(lib.pbr_cook_torrance_camera_mse_stack_fit_step(byref(plan.desc), targets.data_ptr(), *[ptr(b) for b in bufs], gp.data_ptr(),
                                                                    loss.data_ptr(), ws.data_ptr(), stream))
        else:
            gp = None
            N.check(lib.pbr_cook_torrance_camera_mse_stack_step(byref(plan.desc), targets.data_ptr(), *[ptr(b) for b in bufs], loss.data_ptr(),
                                                                ws.data_ptr(), stream))
        gd.check((name, "fit" if fit else "step", only))
        _check_loss(loss[0], c, "guarded")
        for nm, b, g64 in zip(NAMES, bufs, c["grads64"]):
            if b is not None:
                got = b if batched else b[0]
                err, scale = float((got.float().cpu().double() - g64).abs().max()), float(g64.abs().max())
                assert err <= _tol(c["dtype"], scale), (name, nm, err, scale)
        return bufs, gp

    all_bufs, _ = step(False)
    fit_bufs, gp = step(True)
    flat = torch.cat([c["params64"]["view"], c["params64"]["lights"].reshape(-1), c["params64"]["intensities"].reshape(-1)])
    assert float((gp.cpu().double() - flat).abs().max()) <= _param_band(c["params64"])
    for x, y in zip(all_bufs, fit_bufs):
        assert (x is None) == (y is None)
    some, _ = step(False, only=(0, 2))
    assert torch.equal(some[0], all_bufs[0]) and torch.equal(some[2], all_bufs[2])
