"""The stack-fit step, host side (no device): pbr_cook_torrance_mse_stack_fit_step and pbr_mse_stack_fit_workspace_bytes are declared, exported
and bound; the entry point returns the documented codes before any launch; the size query is the documented layout; the routing of
functional.rendering_loss_mse_stack; and the inputs of the GPU branch test are fair -- the oracle's OWN float32 autograd stays well inside
the band the kernels are held to."""
import ctypes

import pytest
import torch

import branch_cases as BC
from pypbr_amd import _native as N
from pypbr_amd import functional as F
from test_light_stack_host import LIGHTS3, _desc


def param_band(want):
    """The band of the stack-fit tests for view, lights and intensities TOGETHER: all three are sums of the same per-pixel colour adjoints, so
    one scale -- the largest |g64| over the three -- holds every element: 2e-5 S + 1e-9."""
    S = max(float(want[k].abs().max()) for k in ("view", "lights", "intensities"))
    return 2e-5 * S + 1e-9


def _fit(d, g_params=1, targets=1, loss=1, workspace=1):
    """The entry point through ctypes with dummy non-NULL addresses: every case here must return before anything is launched or read."""
    buf = (ctypes.c_float * 64)()
    at = lambda on: ctypes.addressof(buf) if on else None
    return N.lib().pbr_cook_torrance_mse_stack_fit_step(ctypes.byref(d), at(targets), None, None, None, None, None, at(g_params), at(loss),
                                                        at(workspace), None)


def test_names_declared_exported_and_bound():
    lib = N.lib()
    assert N.ABI_VERSION == 9 and lib.pbr_abi_version() == 9          # the descriptor did not change
    assert "mse_stack_fit_step" in F.STACK_LAUNCHES


def test_entry_point_returns_its_codes_before_any_launch():
    lib = N.lib()
    d = _desc()
    assert _fit(d, g_params=0) == N.ERR_NULL_MAP
    assert _fit(d, targets=0) == N.ERR_NULL_MAP
    assert _fit(d, loss=0) == N.ERR_NULL_MAP
    assert _fit(d, workspace=0) == N.ERR_NULL_MAP
    d = _desc(tile=(2, 2))
    assert _fit(d) == N.ERR_UNSUPPORTED
    assert lib.pbr_mse_stack_fit_workspace_bytes(ctypes.byref(d)) == 0
    d = _desc()
    d.out_dtype = N.F16
    assert _fit(d) == N.ERR_DTYPE
    assert lib.pbr_mse_stack_fit_workspace_bytes(ctypes.byref(d)) == 0
    d = _desc()
    d.light_size = float("nan")
    assert _fit(d) == N.ERR_UNSUPPORTED
    assert lib.pbr_mse_stack_fit_workspace_bytes(ctypes.byref(d)) == 0


@pytest.mark.parametrize("hw", [(23, 37), (6, 130)])
@pytest.mark.parametrize("L", [1, 3, 16])
def test_workspace_is_the_documented_layout(L, hw):
    """The loss partials and their stage sums as pbr_mse_step_workspace_bytes lays them out, then one row of 3 + 6 L floats per workgroup of
    the one-pixel decomposition (8-byte aligned), then 256 rows of doubles."""
    lib = N.lib()
    H, W = hw
    B = 2
    d = _desc(lights=[[0.1 * i, 0.0, 1.0] for i in range(L)], B=B, H=H, W=W)
    lg = 0
    while (1 << lg) < W and lg < 6:
        lg += 1
    bx, by = 1 << lg, 64 >> lg
    tiles = -(-W // bx) * -(-(B * H) // by)
    n_param = 3 + 6 * L
    loss_part = ((tiles * 4 + 7) & ~7) + 256 * 8
    assert lib.pbr_mse_step_workspace_bytes(ctypes.byref(d)) == loss_part
    want = loss_part + ((tiles * n_param * 4 + 7) & ~7) + 256 * n_param * 8
    assert lib.pbr_mse_stack_fit_workspace_bytes(ctypes.byref(d)) == want, (L, hw, tiles)


def test_routing():
    """functional._stack_route on CPU tensors, the device requirement factored out."""
    a, n, r, m = torch.rand(3, 6, 8), torch.rand(3, 6, 8), torch.rand(1, 6, 8), torch.rand(1, 6, 8)
    maps = (a, n, r, m, None)
    grad_maps = (a.clone().requires_grad_(True), n, r, m, None)
    view, lights, inten = torch.tensor([0.0, 0.0, 1.0]), torch.tensor(LIGHTS3), torch.tensor([1.0, 1.0, 1.0])
    targets = torch.rand(3, 3, 6, 8)
    kw = dict(light_type="point")
    route = lambda maps, params, targets=targets, kw=kw, on=True: F._stack_route(maps, params, targets, kw, on_device=on)
    assert route(maps, (view, lights, inten)) is None                                          # nothing requires grad
    assert route(grad_maps, (view, lights, inten)) == "step"
    for which in range(3):                                                                     # view, a light, an intensity: each alone
        params = [view, lights, inten]
        params[which] = params[which].clone().requires_grad_(True)
        assert route(maps, tuple(params)) == "fit"                                             # only the lights are fitted
        assert route(grad_maps, tuple(params)) == "fit"                                        # together with the maps
        assert route(grad_maps, tuple(params), kw=dict(kw, tile=2)) is None                    # tiled maps
        assert route(grad_maps, tuple(params), targets=targets.clone().requires_grad_(True)) is None
        assert route(grad_maps, tuple(params), on=False) is None                               # no ROCm device
        assert route(grad_maps, tuple(params), kw=dict(kw, out_dtype=torch.float16)) is None
        with torch.no_grad():
            assert route(grad_maps, tuple(params)) is None
        batched = (a.expand(2, 3, 6, 8).clone().requires_grad_(True), n, r.expand(2, 1, 6, 8), m.expand(2, 1, 6, 8), None)   # the normal is shared
        assert route(batched, tuple(params)) is None
    fitted = (view, lights.clone().requires_grad_(True), inten)
    assert route(grad_maps, fitted, kw=dict(kw, tile=1)) == "fit"
    assert route(grad_maps, (view.tolist(), fitted[1], inten.tolist())) == "fit"      # plain lists beside a fitted light
    # and the function the route names carries the class name the GPU tests look for
    assert F._MseStackFitFn.__name__ == "_MseStackFitFn" and F._MseStackFitFn is not F._MseStackStepFn


FP32_ENTRIES = [e for e, cfg in BC.STACK_ENTRY_CONFIGS.items() if not cfg[4]]
VARIANTS = BC.all_stack_variants()


@pytest.mark.parametrize("entry", FP32_ENTRIES)
@pytest.mark.parametrize("name,kw", VARIANTS, ids=[BC.variant_id(n, kw) for n, kw in VARIANTS])
def test_the_inputs_are_fair(name, kw, entry):
    """The parameter gradients are sums over all pixels: every undecided texel takes a decided neighbour's values (none may be left), and
    on that case the oracle's own float32 autograd must stay within a quarter of the band the kernels are held to (worst seen: 0.072,
    `albedo_range`, specular workflow, 24 x 40)."""
    case, left = BC.fill_undecided(BC.build_for(entry, name, kw))
    assert left == 0.0, (name, entry, left)
    target = BC.stack_target(entry, name, kw)
    want = BC.gradients(case, params=True, loss_target=target)
    f32 = BC.gradients(case, dtype=torch.float32, params=True, loss_target=target)
    band = param_band(want)
    worst = max(float((f32[k].double() - want[k]).abs().max()) for k in ("view", "lights", "intensities"))
    print("%s %s: float32 autograd error / band %.3f" % (BC.variant_id(name, kw), entry, worst / band))
    assert worst <= 0.25 * band, (name, entry, worst / band)
