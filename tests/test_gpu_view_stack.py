"""Light stacks with one camera position per shot on the device (csrc/ct_view_stack.hip): functional.cook_torrance_stack and
rendering_loss_mse_stack with `view_dir` [L,3], MultiLightRenderingLoss, and the C ABI behind them (pbr_cook_torrance_view_stack,
pbr_cook_torrance_view_mse_stack_step, pbr_cook_torrance_view_mse_stack_fit_step).

The reference is tools/camera_oracle.py, which tests/test_camera_host.py pins to tests/golden/camera.npz, called once per image with camera l
and light l alone (test_view_stack_host.shot_oracle).  The cases are test_gpu_camera_stack's seven -- 7 x 12 (pairs in the steps, 4-pixel lanes
forward), 5 x 9 (one-pixel lanes, ragged), 2 x [6 x 16] fp16 maps -- with cameras C + DELTAS[l], and the 5 x 9 case under sixteen shots.
Forward values: 1e-5 against the float32 oracle, 2e-6 against the float64 oracle.  The loss: 1e-6 (1 + loss64).  Map gradients:
test_gpu_light_stack's _tol against float64 autograd of mse_loss(stacked oracle, targets).  Cameras, lights and intensities:
test_gpu_camera's _param_band, 2e-5 S + 1e-9 with S the largest float64 magnitude over the three.

tests/test_view_stack_host.py checks in float64 that none of these cameras puts a per-shot image value, or a raw N.V / N.L / N.H, on a kink
that fp32 and float64 could resolve differently: no pixel is excluded from any comparison."""
import ctypes
import functools

import pytest
import torch

from test_camera_host import fixture_case
from test_gpu_camera import BY_NAME, NAMES, _device_maps, _kw, _param_band
from test_gpu_light_stack import _tol
from test_gpu_write_guards import Guards
from test_view_stack_host import STACK_CASES, cameras_of, shot_oracle, sixteen_shots

pytestmark = pytest.mark.gpu


def _case(name):
    c = sixteen_shots() if name == "B_specular_point_16" else fixture_case(BY_NAME[name])
    return dict(c, cameras=c.get("cameras", cameras_of(c)))


@functools.lru_cache(maxsize=None)
def _reference(name):
    """Float64 autograd of mse_loss(stacked per-shot oracle, targets) for one case, computed once and shared (nothing below writes into it)."""
    c = _case(name)
    leaves = [None if t is None else t.float().double().requires_grad_(True) for t in c["maps"]]
    params = [t.double().requires_grad_(True) for t in (c["cameras"], c["lights_t"], c["intens_t"])]
    stack64 = shot_oracle(c, torch.float64, maps=leaves, cameras=params[0], lights=params[1], intens=params[2])
    targets = torch.rand(stack64.shape, generator=torch.Generator().manual_seed(523 + len(name)))
    loss64 = torch.nn.functional.mse_loss(stack64, targets.double())
    loss64.backward()
    return dict(c, stack64=stack64.detach(), stack32=shot_oracle(c, torch.float32, cameras=c["cameras"]), targets=targets,
                loss64=float(loss64.detach()), grads64=[None if t is None else t.grad for t in leaves],
                params64=dict(view=params[0].grad, lights=params[1].grad, intensities=params[2].grad),
                dtype=torch.float16 if c.get("f16") else torch.float32)


def _check_loss(loss, c, tag):
    got = float(loss.detach()) if isinstance(loss, torch.Tensor) else float(loss)
    print("%s %s: loss %.9g (float64 %.9g)" % (tag, c["name"], got, c["loss64"]))
    assert abs(got - c["loss64"]) <= 1e-6 * (1 + c["loss64"]), (tag, c["name"], got, c["loss64"])


def _check_map_gradients(leaves, c, tag):
    for name, x, want in zip(NAMES, leaves, c["grads64"]):
        if x is None:
            continue
        assert x.grad is not None and x.grad.dtype == c["dtype"] and x.grad.shape == x.shape, (tag, name)
        err, scale = float((x.grad.float().cpu().double() - want).abs().max()), float(want.abs().max())
        print("%s %s %-9s max |hip - float64| = %.3e, tolerance %.3e (max |grad| %.3e)" % (tag, c["name"], name, err, _tol(c["dtype"], scale), scale))
        assert err <= _tol(c["dtype"], scale), (tag, c["name"], name, err, scale)


def _check_parameters(params, c, tag, where):
    band = _param_band(c["params64"])
    for k, p in params.items():
        assert p.grad is not None and p.grad.shape == p.shape and p.grad.dtype == p.dtype and p.grad.device.type == where, (tag, k)
        err = float((p.grad.cpu().double() - c["params64"][k]).abs().max())
        print("%s %s %s %-11s max |hip - float64| = %.3e, band %.3e" % (tag, c["name"], where, k, err, band))
        assert err <= band, (tag, c["name"], where, k, err, band)


def _params(c, where, grad=True):
    return {k: t.clone().to(where).requires_grad_(grad) for k, t in (("view", c["cameras"]), ("lights", c["lights_t"]), ("intensities", c["intens_t"]))}


def _vkw(c, **over):
    return _kw(c, **dict(dict(view_dir=c["cameras"]), **over))


def _loss_call(c, leaves, params=None, targets=None):
    from pypbr_amd import functional as F
    over = {} if params is None else dict(view_dir=params["view"], light=params["lights"], light_intensity=params["intensities"])
    return F.rendering_loss_mse_stack(*leaves, targets=c["targets"].cuda() if targets is None else targets, **_vkw(c, **over))


# ------------------------------------------------------------------ 1. the forward stack
@pytest.mark.parametrize("name", STACK_CASES)
def test_forward_stack_parity(name):
    from pypbr_amd import functional as F
    c = _reference(name)
    before = dict(F.STACK_LAUNCHES)
    out = F.cook_torrance_stack(*_device_maps(c), **_vkw(c))
    got = out.cpu()
    assert got.shape == c["stack64"].shape and got.dtype == torch.float32 and not out.requires_grad and bool(torch.isfinite(got).all())
    for l in range(c["L"]):
        image = got.select(-4, l)
        e32 = float((image - c["stack32"].select(-4, l)).abs().max())
        e64 = float((image.double() - c["stack64"].select(-4, l)).abs().max())
        print("%s image %d: max |hip - oracle32| = %.2e   max |hip - oracle64| = %.2e" % (name, l, e32, e64))
        assert e32 <= 1e-5 and e64 <= 2e-6, (name, l, e32, e64)
    if c["L"] == 3:                                             # (for L = 1, [1,3] is one position for all shots: the camera stack's launch)
        moved = {k: F.STACK_LAUNCHES[k] - before[k] for k in before if F.STACK_LAUNCHES[k] != before[k]}
        assert moved == {"view_stack": 1}, moved
    # a map that requires grad: the composition, differentiable
    before = dict(F.STACK_LAUNCHES)
    leaves = _device_maps(c, grad=True)
    composed = F.cook_torrance_stack(*leaves, **_vkw(c))
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
    before = F.STACK_LAUNCHES["view_mse_stack_step"]
    loss = _loss_call(c, leaves)
    if c["L"] == 3:
        assert type(loss.grad_fn).__name__ == "_ViewStackStepFnBackward"
        assert F.STACK_LAUNCHES["view_mse_stack_step"] == before + 1
    after = dict(F.STACK_LAUNCHES)
    loss.backward()
    assert F.STACK_LAUNCHES == after                            # forward kept the gradients: backward launches no step
    _check_loss(loss, c, "step")
    _check_map_gradients(leaves, c, "step")


# ------------------------------------------------------------------ 3. the fit step
@pytest.mark.parametrize("maps_too", [True, False], ids=["with_maps", "parameters_only"])
@pytest.mark.parametrize("name", STACK_CASES)
def test_fit_step_on_host_parameters(name, maps_too):
    from pypbr_amd import functional as F
    c = _reference(name)
    leaves, params = _device_maps(c, grad=maps_too), _params(c, "cpu")
    before = F.STACK_LAUNCHES["view_mse_stack_fit_step"]
    loss = _loss_call(c, leaves, params)
    if c["L"] == 3:
        assert type(loss.grad_fn).__name__ == "_ViewStackFitFnBackward"
        assert F.STACK_LAUNCHES["view_mse_stack_fit_step"] == before + 1
    loss.backward()
    _check_loss(loss, c, "fit")
    _check_parameters(params, c, "fit", "cpu")
    if maps_too:
        _check_map_gradients(leaves, c, "fit")
    else:
        assert all(x is None or x.grad is None for x in leaves)


@pytest.mark.parametrize("maps_too", [True, False], ids=["with_maps", "parameters_only"])
@pytest.mark.parametrize("name", ["A_converted_point_3", "B_metallic_directional_3", "C_converted_point_3_f16"])
def test_fit_step_on_device_parameters(name, maps_too):
    c = _reference(name)
    leaves, params = _device_maps(c, grad=maps_too), _params(c, "cuda")
    loss = _loss_call(c, leaves, params)
    assert type(loss.grad_fn).__name__ == "_ViewStackFitFnBackward"
    loss.backward()
    _check_loss(loss, c, "fit, device parameters")
    _check_parameters(params, c, "fit", "cuda")
    if maps_too:
        _check_map_gradients(leaves, c, "fit, device parameters")


def test_one_intensity_for_all_shots_receives_the_sum():
    """A [3] intensity shared by the three shots: its gradient is the sum over the shots, shaped [3], on the CPU like the tensor; the cameras'
    gradient is [3,3] like the tensor, here float64 like it."""
    from pypbr_amd import functional as F
    base = _reference("A_converted_point_3")
    c = _case("A_converted_point_3")
    shared = c["intens_t"][1].clone()
    p64 = [t.double().requires_grad_(True) for t in (c["cameras"], c["lights_t"], shared)]
    stack64 = shot_oracle(c, torch.float64, cameras=p64[0], lights=p64[1], intens=p64[2].expand(3, 3))
    loss64 = torch.nn.functional.mse_loss(stack64, base["targets"].double())
    loss64.backward()
    want = dict(view=p64[0].grad, lights=p64[1].grad, intensities=p64[2].grad)
    params = dict(view=c["cameras"].clone().double().requires_grad_(True), lights=c["lights_t"].clone().requires_grad_(True),
                  intensities=shared.clone().requires_grad_(True))
    loss = F.rendering_loss_mse_stack(*_device_maps(c), targets=base["targets"].cuda(),
                                      **_kw(c, view_dir=params["view"], light=params["lights"], light_intensity=params["intensities"]))
    assert type(loss.grad_fn).__name__ == "_ViewStackFitFnBackward"
    loss.backward()
    assert abs(loss.item() - loss64.item()) <= 1e-6 * (1 + loss64.item())
    band = _param_band(want)
    assert params["intensities"].grad.shape == (3,) and params["intensities"].grad.device.type == "cpu"
    assert params["view"].grad.shape == (3, 3) and params["view"].grad.dtype == torch.float64 and params["view"].grad.device.type == "cpu"
    for k, p in params.items():
        err = float((p.grad.double() - want[k]).abs().max())
        print("shared intensity %-11s max |hip - float64| = %.3e, band %.3e" % (k, err, band))
        assert err <= band, (k, err, band)


# ------------------------------------------------------------------ 4. equal cameras: the fixed-camera fit step
@pytest.mark.parametrize("name", ["A_converted_point_3", "B_metallic_directional_3", "C_converted_point_3_f16"])
def test_equal_cameras_agree_with_the_fixed_camera_fit_step(name):
    """All L cameras at C: the per-shot camera gradients summed over l are the fixed camera's position gradient (two parameter bands: each
    side is within one of float64); loss and map gradients agree within the bands of both."""
    from pypbr_amd import functional as F
    c = _case(name)
    dtype = torch.float16 if c.get("f16") else torch.float32
    targets = torch.rand((*c["maps"][0].shape[:-3], c["L"], 3, *c["maps"][0].shape[-2:]), generator=torch.Generator().manual_seed(97)).cuda()
    same = c["C"].reshape(1, 3).expand(c["L"], 3).clone()
    runs = {}
    for tag, view in (("per shot", same), ("fixed", c["C"].clone())):
        leaves = _device_maps(c, grad=True)
        params = dict(view=view.requires_grad_(True), lights=c["lights_t"].clone().requires_grad_(True), intensities=c["intens_t"].clone().requires_grad_(True))
        loss = F.rendering_loss_mse_stack(*leaves, targets=targets, **_kw(c, view_dir=params["view"], light=params["lights"], light_intensity=params["intensities"]))
        loss.backward()
        runs[tag] = (loss, leaves, params)
    assert type(runs["per shot"][0].grad_fn).__name__ == "_ViewStackFitFnBackward" and type(runs["fixed"][0].grad_fn).__name__ == "_CameraStackFitFnBackward"
    (la, xa, pa), (lb, xb, pb) = runs["per shot"], runs["fixed"]
    assert abs(la.item() - lb.item()) <= 2e-6 * (1 + lb.item())
    # S of the band: the largest magnitude over the parameters' gradients, the per-shot cameras' included (the sum's terms)
    band = 2 * (2e-5 * max(float(p.grad.abs().max()) for p in list(pa.values()) + list(pb.values())) + 1e-9)
    err = float((pa["view"].grad.sum(dim=0) - pb["view"].grad).abs().max())
    print("%s: sum of per-shot camera gradients against the fixed camera's: %.3e, two bands %.3e" % (name, err, band))
    assert err <= band, (name, err, band)
    for k in ("lights", "intensities"):
        assert float((pa[k].grad - pb[k].grad).abs().max()) <= band, (name, k)
    for nm, x, y in zip(NAMES, xa, xb):
        if x is not None:
            scale = float(y.grad.float().abs().max())
            assert float((x.grad.float() - y.grad.float()).abs().max()) <= 2 * _tol(dtype, scale), (name, nm)


# ------------------------------------------------------------------ 5. sixteen shots: rows of 144 floats
def test_sixteen_shots_fit_step():
    from pypbr_amd import functional as F
    c = _reference("B_specular_point_16")
    assert c["L"] == 16 and c["params64"]["view"].shape == (16, 3)
    for where in ("cpu", "cuda"):
        leaves, params = _device_maps(c, grad=True), _params(c, where)
        before = F.STACK_LAUNCHES["view_mse_stack_fit_step"]
        loss = _loss_call(c, leaves, params)
        assert type(loss.grad_fn).__name__ == "_ViewStackFitFnBackward" and F.STACK_LAUNCHES["view_mse_stack_fit_step"] == before + 1
        loss.backward()
        _check_loss(loss, c, "sixteen shots")
        _check_parameters(params, c, "sixteen shots", where)           # every one of the 9 x 16 parameter gradients
        _check_map_gradients(leaves, c, "sixteen shots")


# ------------------------------------------------------------------ 6. one shot: [1,3] is [3]
@pytest.mark.parametrize("name", ["A_metallic_point_1", "B_specular_point_1"])
def test_one_shot_row_is_the_single_position(name):
    from pypbr_amd import functional as F
    c = _reference(name)
    maps = _device_maps(c)
    assert torch.equal(F.cook_torrance_stack(*maps, **_kw(c, view_dir=c["C"].reshape(1, 3))), F.cook_torrance_stack(*maps, **_kw(c)))
    got = []
    for view in (c["C"].reshape(1, 3).clone(), c["C"].clone()):
        leaves = _device_maps(c, grad=True)
        view.requires_grad_(True)
        loss = F.rendering_loss_mse_stack(*leaves, targets=c["targets"].cuda(), **_kw(c, view_dir=view))
        loss.backward()
        assert view.grad.shape == view.shape
        got.append([loss.detach(), view.grad.reshape(3)] + [t.grad for t in leaves if t is not None])
    for x, y in zip(*got):
        assert torch.equal(x, y)
    _check_loss(got[0][0], c, "one shot")


# ------------------------------------------------------------------ 7. cameras that live on the device
def test_device_resident_cameras_are_read_at_launch(monkeypatch):
    """The positions live on the device and are edited in place between two calls: the second loss is the oracle's at the new positions.
    The one place where the library copies a parameter to the host (functional._host_vec3) refuses device tensors meanwhile: nothing reads
    the positions back."""
    from pypbr_amd import functional as F
    c = _reference("A_converted_point_3")
    leaves = _device_maps(c, grad=True)
    cams = c["cameras"].clone().cuda()
    lights, intens = c["lights_t"].cuda(), c["intens_t"].cuda()
    targets = c["targets"].cuda()
    call = lambda: F.rendering_loss_mse_stack(*leaves, targets=targets, **_kw(c, view_dir=cams, light=lights, light_intensity=intens))
    moved = c["cameras"] + torch.tensor([[-0.15, 0.25, 0.3], [0.05, 0.1, -0.1], [0.2, -0.2, 0.2]])
    staged = moved.cuda()
    host_vec3 = F._host_vec3

    def no_device_tensors(v, rows=None):
        assert not (isinstance(v, torch.Tensor) and v.is_cuda), "a device-resident parameter was copied to the host"
        return host_vec3(v, rows)
    monkeypatch.setattr(F, "_host_vec3", no_device_tensors)
    first = call()
    cams.copy_(staged)                                          # device to device, in place
    second = call()
    assert type(second.grad_fn).__name__ == "_ViewStackStepFnBackward"
    _check_loss(first, c, "device cameras")
    want = torch.nn.functional.mse_loss(shot_oracle(c, torch.float64, cameras=moved.double()), c["targets"].double()).item()
    print("device cameras moved: loss %.9g (float64 %.9g), first %.9g" % (second.item(), want, first.item()))
    assert abs(second.item() - want) <= 1e-6 * (1 + want) and abs(second.item() - first.item()) > 1e-4
    # the forward stack reads them at launch too
    out = F.cook_torrance_stack(*_device_maps(c), **_kw(c, view_dir=cams, light=lights, light_intensity=intens))
    assert float((out.cpu().double() - shot_oracle(c, torch.float64, cameras=moved.double())).abs().max()) <= 2e-6


# ------------------------------------------------------------------ 8. determinism
def test_two_identical_fit_calls_agree_bit_for_bit():
    c = _reference("A_converted_point_3")
    got = []
    for _ in range(2):
        leaves, params = _device_maps(c, grad=True), _params(c, "cpu")
        loss = _loss_call(c, leaves, params)
        loss.backward()
        got.append([loss.detach()] + [t.grad for t in leaves if t is not None] + [p.grad for p in params.values()])
    assert len(got[0]) >= 8
    for x, y in zip(*got):
        assert torch.equal(x, y)
    # differentiated a second time the step is evaluated again (the first backward gave its buffers away): the same bits, accumulated
    leaves, params = _device_maps(c, grad=True), _params(c, "cpu")
    loss = _loss_call(c, leaves, params)
    loss.backward(retain_graph=True)
    loss.backward()
    twice = [t.grad for t in leaves if t is not None] + [p.grad for p in params.values()]
    for x, y in zip(got[0][1:], twice):
        assert torch.equal(x + x, y)


# ------------------------------------------------------------------ 9. guard bands
@pytest.mark.parametrize("name", ["A_converted_point_3", "B_metallic_directional_3", "C_converted_point_3_f16"])
@pytest.mark.parametrize("source", ["host", "device"])
def test_every_written_buffer_sits_between_untouched_guards(name, source):
    """The stack, every gradient buffer, g_params (9 L), the loss and the workspaces (exactly the queried bytes), through the C ABI, with the
    positions from the host and from a guarded device block."""
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
    kw = _kw(c, view_dir=[0.0, 0.0, 1.0])                       # the plan's own view is not read

    def cameras(g):
        if source == "host":
            return F._camera_rows(c["cameras"], L, torch.device("cuda"))[0], None
        return None, g.input(c["cameras"]).data_ptr()

    g = Guards()
    maps = [None if t is None else g.input(t if batched else t.unsqueeze(0)) for t in c["maps"]]
    stack = g.output((B, L, 3, H, W))
    plan = F.plan_cook_torrance(*maps, out=stack.view(B * L, 3, H, W)[:B], **kw)
    N.check(lib.pbr_cook_torrance_view_stack(byref(plan.desc), *cameras(g), stream))
    g.check((name, "stack"))
    want = c["stack64"] if batched else c["stack64"].unsqueeze(0)
    assert float((stack.cpu().double() - want).abs().max()) <= 2e-6

    def step(fit):
        gd = Guards()
        views = [None if t is None else gd.input(t if batched else t.unsqueeze(0)) for t in c["maps"]]
        targets = gd.input(c["targets"] if batched else c["targets"].unsqueeze(0))
        plan = F._step_plan(views, dict(kw))
        bufs = [gd.output((B, ch, H, W), c["dtype"]) if t is not None else None for t, ch in zip(views, channels)]
        loss = gd.output((1,))
        query = lib.pbr_view_mse_stack_fit_workspace_bytes if fit else lib.pbr_mse_step_workspace_bytes
        nbytes = query(byref(plan.desc))
        assert nbytes > 0
        ws = gd.workspace(nbytes)
        gp = gd.output((9 * L,)) if fit else None
        if fit:
            N.check(lib.pbr_cook_torrance_view_mse_stack_fit_step(byref(plan.desc), *cameras(gd), targets.data_ptr(), *[ptr(b) for b in bufs],
                                                                  gp.data_ptr(), loss.data_ptr(), ws.data_ptr(), stream))
        else:
            N.check(lib.pbr_cook_torrance_view_mse_stack_step(byref(plan.desc), *cameras(gd), targets.data_ptr(), *[ptr(b) for b in bufs],
                                                              loss.data_ptr(), ws.data_ptr(), stream))
        gd.check((name, "fit" if fit else "step"))
        _check_loss(loss[0], c, "guarded")
        for nm, b, g64 in zip(NAMES, bufs, c["grads64"]):
            if b is not None:
                got = b if batched else b[0]
                err, scale = float((got.float().cpu().double() - g64).abs().max()), float(g64.abs().max())
                assert err <= _tol(c["dtype"], scale), (name, nm, err, scale)
        return gp

    step(False)
    gp = step(True)
    flat = torch.cat([c["params64"]["view"].reshape(-1), c["params64"]["lights"].reshape(-1), c["params64"]["intensities"].reshape(-1)])
    assert float((gp.cpu().double() - flat).abs().max()) <= _param_band(c["params64"])


# ------------------------------------------------------------------ 10. fused against the composition
@pytest.mark.parametrize("name", STACK_CASES)
def test_fused_route_against_the_composition(name):
    """The same call forced onto the composition (targets that require grad): L camera renders, torch's MSE, L camera backwards."""
    from pypbr_amd import functional as F
    c = _reference(name)
    fused_leaves, fused_params = _device_maps(c, grad=True), _params(c, "cpu")
    fused = _loss_call(c, fused_leaves, fused_params)
    fused.backward()
    before = dict(F.STACK_LAUNCHES)
    leaves, params = _device_maps(c, grad=True), _params(c, "cpu")
    composed = _loss_call(c, leaves, params, targets=c["targets"].cuda().requires_grad_(True))
    assert F.STACK_LAUNCHES == before and "Stack" not in type(composed.grad_fn).__name__
    composed.backward()
    assert abs(fused.item() - composed.item()) <= 1e-6 * (1 + composed.item()), (name, fused.item(), composed.item())
    for nm, x, y in zip(NAMES, fused_leaves, leaves):
        if x is not None:
            scale = float(y.grad.float().abs().max())
            err = float((x.grad.float() - y.grad.float()).abs().max())
            assert err <= _tol(c["dtype"], scale), (name, nm, err, scale)
    band = 2e-5 * max(float(p.grad.abs().max()) for p in params.values()) + 1e-9
    for k in params:
        assert params[k].grad.shape == fused_params[k].grad.shape
        err = float((fused_params[k].grad - params[k].grad).abs().max())
        assert err <= band, (name, k, err, band)


# ------------------------------------------------------------------ 11. the loss module
def test_multi_light_rendering_loss_takes_the_fused_route():
    from pypbr_amd import functional as F
    from pypbr_amd.losses import MultiLightRenderingLoss
    from pypbr_amd.materials import DiffuseSpecularMaterial
    from test_camera_host import oracle
    c = _case("A_specular_directional_3")
    leaves = _device_maps(c, grad=True)
    mat = DiffuseSpecularMaterial(albedo=leaves[0], normal=None, roughness=leaves[2], specular=leaves[4], albedo_is_srgb=c["srgb"],
                                  specular_is_srgb=c["srgb"], device=torch.device("cuda"))
    mat._maps["normal"] = leaves[1]
    # the module encodes the result (return_srgb is upstream's default): the oracle with that
    leaves64 = [None if t is None else t.double().requires_grad_(True) for t in c["maps"]]
    stack = shot_oracle(c, torch.float64, maps=leaves64, cameras=c["cameras"].double(), return_srgb=True)
    targets = torch.rand(stack.shape, generator=torch.Generator().manual_seed(29))
    loss64 = torch.nn.functional.mse_loss(stack, targets.double())
    loss64.backward()
    ref = dict(c, targets=targets, loss64=float(loss64.detach()), grads64=[None if t is None else t.grad for t in leaves64], dtype=torch.float32)
    before = dict(F.STACK_LAUNCHES)
    crit = MultiLightRenderingLoss(c["light_type"], c["cameras"], c["lights_t"], c["intens_t"], c["light_size"], view_type="point")
    loss = crit(mat, targets.cuda())
    assert type(loss.grad_fn).__name__ == "_ViewStackStepFnBackward"
    assert F.STACK_LAUNCHES["view_mse_stack_step"] == before["view_mse_stack_step"] + 1
    loss.backward()
    _check_loss(loss, ref, "MultiLightRenderingLoss")
    _check_map_gradients(leaves, ref, "MultiLightRenderingLoss")
    # a material as ground truth, nothing differentiated: both renderings are ONE launch of the per-shot stack each
    before = dict(F.STACK_LAUNCHES)
    with torch.no_grad():
        zero = crit(mat, mat)
    assert F.STACK_LAUNCHES["view_stack"] == before["view_stack"] + 2 and float(zero) == 0.0      # ground truth and prediction: one launch each


# ------------------------------------------------------------------ 12. one orthographic direction per shot
def test_orthographic_directions_per_shot_are_the_composition():
    """view_type="directional" with [L,3] directions has no kernel of its own: image l IS cook_torrance(view_dir=view_dir[l], light=light[l])."""
    from pypbr_amd import functional as F
    c = _case("A_converted_point_3")
    maps = _device_maps(c)
    dirs = torch.tensor([[0.0, 0.0, 1.0], [0.2, -0.1, 0.9], [-0.3, 0.2, 0.8]])
    kw = _kw(c, view_type="directional")
    before = dict(F.STACK_LAUNCHES)
    out = F.cook_torrance_stack(*maps, **dict(kw, view_dir=dirs))
    assert F.STACK_LAUNCHES == before and out.shape == (3, 3) + tuple(maps[0].shape[-2:])
    for l in range(3):
        one = F.cook_torrance(*maps, **dict(kw, view_dir=dirs[l], light=c["lights_t"][l], light_intensity=c["intens_t"][l]))
        assert torch.equal(out[l], one), l
    # and the loss over it is differentiable through the composition, directions included
    leaves = _device_maps(c, grad=True)
    d = dirs.clone().requires_grad_(True)
    loss = F.rendering_loss_mse_stack(*leaves, targets=torch.rand(out.shape, generator=torch.Generator().manual_seed(5)).cuda(), **dict(kw, view_dir=d))
    assert F.STACK_LAUNCHES == before and "Stack" not in type(loss.grad_fn).__name__
    loss.backward()
    assert d.grad.shape == (3, 3) and bool(torch.isfinite(d.grad).all()) and leaves[0].grad is not None
