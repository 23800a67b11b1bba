"""Guard bands around everything pbr_cook_torrance_mse_stack_fit_step writes (csrc/ct_stack.hip), launched through the C ABI: the maps and the
target stack sit inside NaN margins; every gradient, g_params and the loss are pre-filled with UNWRITTEN inside EDGE margins; the workspace has
exactly the queried byte count (0xFF inside 0xA5 margins).  Margins intact, every element of g_params and of every gradient written and finite,
values at the tolerances of tests/test_gpu_light_stack_fit.py against float64."""
import ctypes

import pytest
import torch

from test_gpu_write_guards import Guards, P, _leaves64, _lib, _material, _params, _plan, _render64, _stream
from test_light_stack_fit_host import param_band

pytestmark = pytest.mark.gpu

WIDTHS = (1, 3, 4, 5, 7, 8, 127, 128, 130)
H, B, L = 3, 2, 3


@pytest.mark.parametrize("dt", ["f32", "f16"])
@pytest.mark.parametrize("W", WIDTHS)
def test_stack_fit_step_writes_only_its_outputs_and_all_of_them(W, dt):
    N, lib = _lib()
    dtype = torch.float16 if dt == "f16" else torch.float32
    g = torch.Generator().manual_seed(9300 + W + (1000 if dt == "f16" else 0))
    maps = _material(g, B, H, W, "metallic", dtype)
    kw = _params("point", L)
    targets = torch.rand(B, L, 3, H, W, generator=g)
    leaves = _leaves64(maps)
    view = torch.tensor(kw["view_dir"], dtype=torch.float64, requires_grad=True)
    lights = torch.tensor(kw["light"], dtype=torch.float64, requires_grad=True)
    intens = torch.tensor(kw["light_intensity"], dtype=torch.float64, requires_grad=True)
    stack64 = torch.stack([_render64(leaves, "metallic", kw, view=view, lights=lights[l:l + 1], intens=intens[l:l + 1]) for l in range(L)], dim=1)
    loss64 = ((stack64 - targets.double()) ** 2).mean()
    loss64.backward()
    want = dict(view=view.grad, lights=lights.grad, intensities=intens.grad)
    gd = Guards()
    views = [None if t is None else gd.input(t) for t in maps]
    tgt = gd.input(targets)
    plan = _plan(views, kw)
    tag = (W, dt)
    nbytes = lib.pbr_mse_stack_fit_workspace_bytes(ctypes.byref(plan.desc))
    assert nbytes > lib.pbr_mse_step_workspace_bytes(ctypes.byref(plan.desc)) > 0
    ws = gd.workspace(nbytes)
    loss = gd.output((1,))
    gp = gd.output((3 + 6 * L,))
    grads = [None if t is None else gd.output(t.shape, dtype) for t in maps]
    N.check(lib.pbr_cook_torrance_mse_stack_fit_step(ctypes.byref(plan.desc), P(tgt), *[P(t) for t in grads], P(gp), P(loss), P(ws), _stream()))
    gd.check(tag)
    ref = float(loss64.detach())
    assert abs(float(loss) - ref) <= 1e-6 * (1 + ref), (tag, float(loss), ref)
    for name, got, leaf in zip(("albedo", "normal", "roughness", "metallic", "specular"), grads, leaves):
        if got is None:
            continue
        scale = float(leaf.grad.abs().max())
        e = float((got.float().cpu().double() - leaf.grad).abs().max())
        assert e <= (2e-5 if dtype == torch.float32 else 2e-3) * scale + 1e-9, (tag, name, e, scale)
    flat = torch.cat([want["view"], want["lights"].reshape(-1), want["intensities"].reshape(-1)])
    err = float((gp.cpu().double() - flat).abs().max())
    band = param_band(want)
    print("stack fit guards W=%d %s: worst parameter error / band %.3f" % (W, dt, err / band))
    assert err <= band, (tag, err, band)
