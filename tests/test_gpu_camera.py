"""The perspective camera on the device (csrc/ct_camera.hip): functional.cook_torrance(view_type="point"), CookTorranceBRDF(view_type="point"),
the loss modules, and the C ABI behind them (pbr_cook_torrance_camera, pbr_cook_torrance_camera_backward).

Forward values are held to tests/golden/camera.npz -- upstream's forward evaluated pixel by pixel with view_dir = C - P(y, x), in float32
(`ref32`, criterion (i): 1e-5) and in float64 (`ref64`, criterion (ii): 2e-6).  Gradients are held to float64 autograd
through tools/camera_oracle.py, which tests/test_camera_host.py pins to the same fixture: map gradients inside test_gpu_light_stack's _tol,
the camera position, lights and intensities inside test_gpu_light_stack_fit's rule, 2e-5 S + 1e-9 with S the largest float64 magnitude over
the three.  The shapes are the fixture's: 7 x 12 (4-pixel lanes forward, pairs backward), 5 x 9 (one-pixel lanes; the grid holds (0, 0)) and
2 x [6 x 16] fp16 maps."""
import ctypes
import functools

import pytest
import torch

from test_camera_host import CASES, CO, fixture_case, oracle
from test_gpu_light_stack import _tol
from test_gpu_write_guards import Guards

pytestmark = pytest.mark.gpu

NAMES = ("albedo", "normal", "roughness", "metallic", "specular")
GRAD_CASES = [c for c in CASES if not c.get("forward_only")]
GRAD_IDS = [c["name"] for c in GRAD_CASES]
A_CASES = [c for c in GRAD_CASES if c["name"].startswith("A_")]
BY_NAME = {c["name"]: c for c in CASES}


def _kw(c, **over):
    """The library's keyword arguments of a fixture case (host parameters)."""
    converted = c["workflow"] == "converted"
    kw = dict(view_dir=c["C"], light=c["lights_t"], light_intensity=c["intens_t"], light_type=c["light_type"], light_size=c["light_size"],
              albedo_is_srgb=c["srgb"], specular_is_srgb=c["srgb"] or converted, return_srgb=c["srgb"], convert_to_diffuse_specular=converted,
              view_type="point")
    kw.update(over)
    return kw


def _device_maps(c, grad=False):
    return [None if t is None else t.cuda().requires_grad_(grad) for t in c["maps"]]


@functools.lru_cache(maxsize=None)
def _reference(name):
    """Float64 autograd through the oracle for one case, computed once and shared (nothing below writes into it): the weights of the scalar
    that is differentiated, the gradients of the maps and of camera / lights / intensities."""
    c = fixture_case(BY_NAME[name])
    g = torch.Generator().manual_seed(77 + len(name))
    weights = torch.rand(c["ref64"].shape, generator=g) - 0.4
    leaves = [None if t is None else t.float().double().requires_grad_(True) for t in c["maps"]]
    params = [t.double().requires_grad_(True) for t in (c["C"], c["lights_t"], c["intens_t"])]
    out = oracle(c, torch.float64, maps=leaves, camera=params[0], lights=params[1], intens=params[2])
    (out * weights.double()).sum().backward()
    return dict(c, weights=weights, out64=out.detach(), grads64=[None if t is None else t.grad for t in leaves],
                params64=dict(view=params[0].grad, lights=params[1].grad, intensities=params[2].grad))


def _param_band(want):
    """test_gpu_light_stack_fit's rule: all three are sums of the same per-pixel adjoints, so one scale holds every element."""
    return 2e-5 * max(float(v.abs().max()) for v in want.values()) + 1e-9


def _check_forward(out, c, tag):
    got = out.detach().cpu()
    assert got.shape == c["ref32"].shape and got.dtype == torch.float32 and bool(torch.isfinite(got).all()), tag
    e32, e64 = float((got - c["ref32"]).abs().max()), float((got.double() - c["ref64"]).abs().max())
    print("%s %s: max |hip - ref32| = %.2e   max |hip - ref64| = %.2e" % (tag, c["name"], e32, e64))
    assert e32 <= 1e-5 and e64 <= 2e-6, (tag, c["name"], e32, e64)


# ------------------------------------------------------------------ 1. forward parity
@pytest.mark.parametrize("case", CASES, ids=[c["name"] for c in CASES])
def test_forward_parity_functional(case):
    """Every case, the camera-on-a-pixel edge case included (finite, same tolerances); fp16 maps against upstream on the rounded maps."""
    from pypbr_amd import functional as F
    c = fixture_case(case)
    _check_forward(F.cook_torrance(*_device_maps(c), **_kw(c)), c, "functional")


@pytest.mark.parametrize("case", CASES, ids=[c["name"] for c in CASES])
def test_forward_parity_module(case):
    """CookTorranceBRDF(view_type="point") on real materials: the second argument of forward is the camera's position.  (Materials hold
    float32 maps: the fp16 cases go in as the float32 values of their rounded maps, which is what the fixture evaluated.)"""
    from pypbr_amd.materials import BasecolorMetallicMaterial, DiffuseSpecularMaterial
    from pypbr_amd.models import CookTorranceBRDF
    c = fixture_case(case)
    a, n, r, m, s = [None if t is None else t.float().cuda() for t in c["maps"]]
    dev = torch.device("cuda")
    if c["workflow"] == "specular":
        mat = DiffuseSpecularMaterial(albedo=a, normal=None, roughness=r, specular=s, albedo_is_srgb=c["srgb"], specular_is_srgb=c["srgb"], device=dev)
    else:
        mat = BasecolorMetallicMaterial(albedo=a, normal=None, roughness=r, metallic=m, albedo_is_srgb=c["srgb"], device=dev)
    mat._maps["normal"] = n                                   # as stored: already decoded (or absent: +Z)
    if c["workflow"] == "converted":
        mat = mat.to_diffuse_specular_material()
    brdf = CookTorranceBRDF(light_type=c["light_type"], view_type="point")
    lights, intens = (c["lights_t"], c["intens_t"]) if c["L"] > 1 else (c["lights_t"][0], c["intens_t"][0])
    _check_forward(brdf(mat, c["C"], lights, intens, c["light_size"], return_srgb=c["srgb"]), c, "module")


# ------------------------------------------------------------------ 2. actually perspective
def test_the_camera_is_not_the_orthographic_view():
    """Case A differs from the orthographic render along C by more than 1e-3 somewhere.  Where C - P is parallel to C -- P = 0: the centre
    pixel of a grid with odd extents, which case B has and case A (12 columns) has not -- the two agree: each is within 2e-6 of the same
    float64 value (criterion (ii)), so within 4e-6 of the other."""
    from pypbr_amd import functional as F
    for name in ("A_metallic_point_1", "B_specular_point_1"):
        c = fixture_case(BY_NAME[name])
        maps = _device_maps(c)
        cam = F.cook_torrance(*maps, **_kw(c)).cpu()
        ortho = F.cook_torrance(*maps, **_kw(c, view_type="directional")).cpu()
        diff = (cam - ortho).abs()
        print("%s: max |camera - orthographic| = %.3e" % (name, float(diff.max())))
        assert float(diff.max()) > 1e-3, name
        H, W = c["shape"][-2:]
        P = CO.surface_points(H, W, c["light_size"])
        centre = (P.abs().sum(0) == 0).nonzero()
        assert len(centre) == (1 if name.startswith("B_") else 0)
        for y, x in centre.tolist():
            assert float(diff[:, y, x].max()) <= 4e-6, (name, y, x, float(diff[:, y, x].max()))


# ------------------------------------------------------------------ 3. row bands
@pytest.mark.parametrize("case", A_CASES, ids=[c["name"] for c in A_CASES])
def test_row_bands_are_bit_equal(case):
    """Rows 2..4 rendered with y_offset=2, height_total=7 against those rows of the whole render, result and map gradients."""
    from pypbr_amd import functional as F
    c = _reference(case["name"])
    whole = _device_maps(c, grad=True)
    out = F.cook_torrance(*whole, **_kw(c))
    (out * c["weights"].cuda()).sum().backward()
    band = [None if t is None else t.detach()[:, 2:5].clone().requires_grad_(True) for t in whole]
    part = F.cook_torrance(*band, y_offset=2, height_total=7, **_kw(c))
    (part * c["weights"][:, 2:5].cuda()).sum().backward()
    assert torch.equal(part, out[:, 2:5])
    for name, x, y in zip(NAMES, band, whole):
        if x is not None:
            assert torch.equal(x.grad, y.grad[:, 2:5]), (case["name"], name)


# ------------------------------------------------------------------ 4. map gradients
@pytest.mark.parametrize("case", GRAD_CASES, ids=GRAD_IDS)
def test_map_gradients_against_float64_autograd(case):
    from pypbr_amd import functional as F
    c = _reference(case["name"])
    dtype = torch.float16 if c.get("f16") else torch.float32
    leaves = _device_maps(c, grad=True)
    out = F.cook_torrance(*leaves, **_kw(c))
    (out * c["weights"].cuda()).sum().backward()
    for name, x, want in zip(NAMES, leaves, c["grads64"]):
        if x is None:
            continue
        assert x.grad.dtype == dtype and x.grad.shape == x.shape
        err, scale = float((x.grad.float().cpu().double() - want).abs().max()), float(want.abs().max())
        print("%s %-9s max |hip - float64| = %.3e, tolerance %.3e (max |grad| %.3e)" % (case["name"], name, err, _tol(dtype, scale), scale))
        assert err <= _tol(dtype, scale), (case["name"], name, err, scale)


# ------------------------------------------------------------------ 5. camera position, lights, intensities
def _param_run(c, where, wanted, maps_too):
    """One differentiable call with the parameters named in `wanted` as leaves on `where` -> (leaves, parameter tensors)."""
    from pypbr_amd import functional as F
    leaves = _device_maps(c, grad=maps_too)
    params = {k: t.clone().to(where).requires_grad_(k in wanted) for k, t in (("view", c["C"]), ("lights", c["lights_t"]), ("intensities", c["intens_t"]))}
    out = F.cook_torrance(*leaves, **_kw(c, view_dir=params["view"], light=params["lights"], light_intensity=params["intensities"]))
    (out * c["weights"].cuda()).sum().backward()
    return leaves, params


@pytest.mark.parametrize("where", ["cpu", "cuda"])
@pytest.mark.parametrize("case", GRAD_CASES, ids=GRAD_IDS)
def test_parameter_gradients_against_float64_autograd(case, where):
    """Each of the three alone, then all together with the maps; parameters on the host and on the device; two identical calls agree
    bit for bit (one-wave workgroups, rows added up in fp64 in a fixed order)."""
    c = _reference(case["name"])
    want, band = c["params64"], _param_band(c["params64"])
    dtype = torch.float16 if c.get("f16") else torch.float32
    for wanted, maps_too in ((("view",), False), (("lights",), False), (("intensities",), False), (("view", "lights", "intensities"), True)):
        leaves, params = _param_run(c, where, wanted, maps_too)
        for k, p in params.items():
            if k not in wanted:
                assert p.grad is None
                continue
            assert p.grad.shape == p.shape and p.grad.device.type == where
            err = float((p.grad.cpu().double() - want[k]).abs().max())
            print("%s %s %-11s (of %s) max |hip - float64| = %.3e, band %.3e" % (case["name"], where, k, "+".join(wanted), err, band))
            assert err <= band, (case["name"], where, k, wanted, err, band)
        if maps_too:
            for name, x, g64 in zip(NAMES, leaves, c["grads64"]):
                if x is not None:
                    err, scale = float((x.grad.float().cpu().double() - g64).abs().max()), float(g64.abs().max())
                    assert err <= _tol(dtype, scale), (case["name"], name, err, scale)
            _, again = _param_run(c, where, wanted, maps_too)
            for k in wanted:
                assert torch.equal(params[k].grad, again[k].grad), (case["name"], k)


# ------------------------------------------------------------------ 6. a camera that lives on the device
def test_device_resident_camera_is_read_at_every_launch():
    """ONE plan, captured into a graph (a host read of the position would raise under capture); the tensor is edited in place between two
    replays and the second image is the new position's."""
    from pypbr_amd import functional as F
    c = fixture_case(BY_NAME["A_converted_point_3"])
    maps = _device_maps(c)
    camera = c["C"].clone().cuda()
    plan = F.plan_cook_torrance(*maps, **_kw(c, view_dir=camera))
    assert plan.view_type == "point" and plan.desc.device_params
    plan.launch()                                            # warm-up outside the capture
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        out = plan.launch()
    graph.replay()
    first = out.clone()
    moved = torch.tensor([-0.15, 0.25, 0.9])
    camera.copy_(moved)
    graph.replay()
    torch.cuda.synchronize()
    _check_forward(first, c, "device camera")
    want = oracle(c, torch.float64, camera=moved)
    err = float((out.cpu().double() - want).abs().max())
    print("device camera moved: max |hip - float64| = %.2e, |moved - first| = %.2e" % (err, float((out - first).abs().max())))
    assert err <= 2e-6 and float((out - first).abs().max()) > 1e-3


# ------------------------------------------------------------------ 7. guard bands
GUARD_CASES = ["A_metallic_point_1", "A_specular_directional_3", "A_metallic_directional_1_flat", "B_specular_point_1", "B_metallic_directional_3"]


@pytest.mark.parametrize("name", GUARD_CASES)
def test_every_written_buffer_sits_between_untouched_guards(name):
    """Result, every gradient buffer, g_params and the workspace (exactly the queried bytes), through the C ABI; the values are the autograd
    path's, bit for bit (the same descriptor, the same kernels)."""
    from pypbr_amd import _native as N
    from pypbr_amd import functional as F
    c = _reference(name)
    lib = N.lib()
    stream = torch.cuda.current_stream().cuda_stream
    H, W = c["shape"][-2:]
    L = c["L"]
    g = Guards()
    maps = [None if t is None else g.input(t.unsqueeze(0)) for t in c["maps"]]
    out = g.output((1, 3, H, W))
    plan = F.plan_cook_torrance(*maps, out=out, **_kw(c))
    plan.launch()
    g.check((name, "forward"))
    _check_forward(out[0], c, "guarded")
    gout = g.input(c["weights"].unsqueeze(0))
    channels = (3, 3, 1, 1, 3)
    bufs = [None if t is None else g.output((1, ch, H, W)) for t, ch in zip(maps, channels)]
    gp = g.output((3 + 6 * L,))
    nbytes = lib.pbr_camera_backward_workspace_bytes(ctypes.byref(plan.desc))
    assert nbytes > 0
    ws = g.workspace(nbytes)
    ptr = lambda t: None if t is None else t.data_ptr()
    N.check(lib.pbr_cook_torrance_camera_backward(ctypes.byref(plan.desc), gout.data_ptr(), *[ptr(b) for b in bufs], gp.data_ptr(), ws.data_ptr(), stream))
    g.check((name, "backward with g_params"))
    leaves, params = _param_run(c, "cpu", ("view", "lights", "intensities"), True)
    for nm, b, x in zip(NAMES, bufs, leaves):
        if b is not None:
            assert torch.equal(b[0], x.grad), (name, nm)
    assert torch.equal(gp[:3].cpu(), params["view"].grad) and torch.equal(gp[3:3 + 3 * L].cpu().reshape(L, 3), params["lights"].grad)
    assert torch.equal(gp[3 + 3 * L:].cpu().reshape(L, 3), params["intensities"].grad)
    # the maps alone: no g_params, no workspace -- and only some of the maps
    g2 = Guards()
    maps2 = [None if t is None else g2.input(t.unsqueeze(0)) for t in c["maps"]]
    plan2 = F.plan_cook_torrance(*maps2, out=g2.output((1, 3, H, W)), **_kw(c))
    gout2 = g2.input(c["weights"].unsqueeze(0))
    only = [g2.output((1, ch, H, W)) if (t is not None and i in (0, 2)) else None for i, (t, ch) in enumerate(zip(maps2, channels))]
    plan2.launch()
    N.check(lib.pbr_cook_torrance_camera_backward(ctypes.byref(plan2.desc), gout2.data_ptr(), *[ptr(b) for b in only], None, None, stream))
    g2.check((name, "backward, albedo and roughness only"))
    assert torch.equal(only[0], bufs[0]) and torch.equal(only[2], bufs[2])


# ------------------------------------------------------------------ 8. losses
def test_losses_take_the_camera():
    """RenderingLoss(view_type="point") and rendering_loss_mse(view_type="point") against mse_loss(oracle render, target) in float64:
    the loss within 1e-6 (1 + loss), the map gradients inside _tol."""
    from pypbr_amd import functional as F
    from pypbr_amd.losses import MultiLightRenderingLoss, RenderingLoss
    from pypbr_amd.materials import BasecolorMetallicMaterial
    c = fixture_case(BY_NAME["A_metallic_point_1"])
    target = torch.rand(c["ref64"].shape, generator=torch.Generator().manual_seed(5))
    leaves64 = [None if t is None else t.double().requires_grad_(True) for t in c["maps"]]
    loss64 = torch.nn.functional.mse_loss(oracle(c, torch.float64, maps=leaves64), target.double())
    loss64.backward()

    def check(loss, leaves, tag):
        loss.backward()
        print("%s: loss %.9g (float64 %.9g)" % (tag, loss.item(), loss64.item()))
        assert abs(loss.item() - loss64.item()) <= 1e-6 * (1 + loss64.item()), tag
        for name, x, y in zip(NAMES, leaves, leaves64):
            if x is not None:
                err, scale = float((x.grad.cpu().double() - y.grad).abs().max()), float(y.grad.abs().max())
                assert err <= _tol(torch.float32, scale), (tag, name, err, scale)

    leaves = _device_maps(c, grad=True)
    check(F.rendering_loss_mse(*leaves, target=target.cuda(), **_kw(c)), leaves, "rendering_loss_mse")
    leaves = _device_maps(c, grad=True)
    mat = BasecolorMetallicMaterial(albedo=leaves[0], normal=None, roughness=leaves[2], metallic=leaves[3], albedo_is_srgb=c["srgb"], device=torch.device("cuda"))
    mat._maps["normal"] = leaves[1]
    crit = RenderingLoss(c["light_type"], c["C"], c["lights_t"][0], c["intens_t"][0], c["light_size"], view_type="point")
    check(crit(mat, target.cuda()), leaves, "RenderingLoss")
    leaves = _device_maps(c, grad=True)
    mat = BasecolorMetallicMaterial(albedo=leaves[0], normal=None, roughness=leaves[2], metallic=leaves[3], albedo_is_srgb=c["srgb"], device=torch.device("cuda"))
    mat._maps["normal"] = leaves[1]
    stack = MultiLightRenderingLoss(c["light_type"], c["C"], c["lights_t"], c["intens_t"], c["light_size"], view_type="point")
    check(stack(mat, target.cuda().unsqueeze(0)), leaves, "MultiLightRenderingLoss, one light")


def test_a_recorded_tile_is_carried_out_first():
    """material.tile(2) on device-resident maps only records the repeat; the camera renders real maps, so the module (and the loss
    module through it) materialises them: the image of the repeated maps, bit for bit."""
    from pypbr_amd import functional as F
    from pypbr_amd.losses import RenderingLoss
    from pypbr_amd.materials import DiffuseSpecularMaterial
    from pypbr_amd.models import CookTorranceBRDF
    c = fixture_case(BY_NAME["B_specular_point_1"])
    a, n, r, _, s = _device_maps(c)

    def tiled():
        mat = DiffuseSpecularMaterial(albedo=a, normal=None, roughness=r, specular=s, albedo_is_srgb=c["srgb"], specular_is_srgb=c["srgb"], device=torch.device("cuda"))
        mat._maps["normal"] = n
        mat.tile(2)
        assert mat.lazy_tile == (2, 2)
        return mat
    want = F.cook_torrance(*[None if t is None else t.repeat(1, 2, 2) for t in (a, n, r, None, s)], **_kw(c))
    mat = tiled()
    got = CookTorranceBRDF(c["light_type"], view_type="point")(mat, c["C"], c["lights_t"][0], c["intens_t"][0], c["light_size"], return_srgb=c["srgb"])
    assert mat.lazy_tile == (1, 1) and got.shape == (3, 10, 18) and torch.equal(got, want)
    target = torch.rand(3, 10, 18, generator=torch.Generator().manual_seed(3)).cuda()
    loss = RenderingLoss(c["light_type"], c["C"], c["lights_t"][0], c["intens_t"][0], c["light_size"], view_type="point")(tiled(), target)
    assert torch.equal(loss, torch.nn.functional.mse_loss(want, target))


# ------------------------------------------------------------------ 9. the default is untouched
@pytest.mark.parametrize("case", A_CASES, ids=[c["name"] for c in A_CASES])
def test_directional_view_type_is_the_default(case):
    """view_type="directional" passed explicitly against omitting it: bit-equal, forward and gradients (maps and parameters)."""
    from pypbr_amd import functional as F
    c = _reference(case["name"])
    got = []
    for explicit in (False, True):
        leaves = _device_maps(c, grad=True)
        params = [t.clone().requires_grad_(True) for t in (c["C"], c["lights_t"], c["intens_t"])]
        kw = _kw(c, view_dir=params[0], light=params[1], light_intensity=params[2])
        del kw["view_type"]
        if explicit:
            kw["view_type"] = "directional"
        plain = F.cook_torrance(*[t if t is None else t.detach() for t in leaves], **{**kw, "view_dir": c["C"], "light": c["lights_t"], "light_intensity": c["intens_t"]})
        out = F.cook_torrance(*leaves, **kw)
        (out * c["weights"].cuda()).sum().backward()
        got.append([plain, out.detach()] + [t.grad for t in leaves if t is not None] + [p.grad for p in params])
    for x, y in zip(*got):
        assert torch.equal(x, y)
