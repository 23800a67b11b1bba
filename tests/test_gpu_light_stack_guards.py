"""Guard bands around everything the light-stack entry points write (csrc/ct_stack.hip), launched through the C ABI: the maps and the target
stack sit inside NaN margins, the stack output and every gradient are pre-filled with UNWRITTEN inside EDGE margins, the workspace has exactly
the queried byte count (0xFF inside 0xA5 margins).  Margins intact, every value written and finite, values at the value tests' tolerances
(tests/test_gpu_light_stack.py) against float64."""
import ctypes

import pytest
import torch

from test_gpu_parity import TRACK
from test_gpu_write_guards import Guards, P, _leaves64, _lib, _material, _params, _plan, _render64, _stream

pytestmark = pytest.mark.gpu

WIDTHS = (1, 3, 4, 5, 7, 8, 127, 128, 130)
H, B, L = 3, 2, 3


@pytest.mark.parametrize("dt", ["f32", "f16"])
@pytest.mark.parametrize("W", WIDTHS)
def test_stack_and_stack_step_write_only_their_outputs_and_all_of_them(W, dt):
    N, lib = _lib()
    dtype = torch.float16 if dt == "f16" else torch.float32
    g = torch.Generator().manual_seed(9100 + W + (1000 if dt == "f16" else 0))
    maps = _material(g, B, H, W, "metallic", dtype)
    kw = _params("point", L)
    targets = torch.rand(B, L, 3, H, W, generator=g)
    leaves = _leaves64(maps)
    lights = torch.tensor(kw["light"], dtype=torch.float64)
    intens = torch.tensor(kw["light_intensity"], dtype=torch.float64)
    stack64 = torch.stack([_render64(leaves, "metallic", kw, lights=lights[l:l + 1], intens=intens[l:l + 1]) for l in range(L)], dim=1)
    loss64 = ((stack64 - targets.double()) ** 2).mean()
    loss64.backward()
    gd = Guards()
    views = [None if t is None else gd.input(t) for t in maps]
    tgt = gd.input(targets)
    plan = _plan(views, kw)
    tag = (W, dt)
    # ---- the stack itself
    out = gd.output((B, L, 3, H, W))
    plan.desc.out = out.data_ptr()
    N.check(lib.pbr_cook_torrance_stack(ctypes.byref(plan.desc), _stream()))
    gd.check(tag + ("stack",))
    err = float((out.cpu().double() - stack64.detach()).abs().max())
    assert err <= TRACK, (tag, err)
    # ---- the loss step: exact workspace, a guarded loss, every gradient
    nbytes = lib.pbr_mse_step_workspace_bytes(ctypes.byref(plan.desc))
    assert nbytes > 0
    ws = gd.workspace(nbytes)
    loss = gd.output((1,))
    grads = [None if t is None else gd.output(t.shape, dtype) for t in maps]
    N.check(lib.pbr_cook_torrance_mse_stack_step(ctypes.byref(plan.desc), P(tgt), *[P(t) for t in grads], P(loss), P(ws), _stream()))
    gd.check(tag + ("step",))
    want = float(loss64.detach())
    assert abs(float(loss) - want) <= 1e-6 * (1 + want), (tag, float(loss), want)
    for name, got, leaf in zip(("albedo", "normal", "roughness", "metallic", "specular"), grads, leaves):
        if got is None:
            continue
        scale = float(leaf.grad.abs().max())
        e = float((got.float().cpu().double() - leaf.grad).abs().max())
        assert e <= (2e-5 if dtype == torch.float32 else 2e-3) * scale + 1e-9, (tag, name, e, scale)
