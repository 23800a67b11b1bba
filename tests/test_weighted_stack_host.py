"""Per-pixel weights in the light-stack loss steps, host side (no device): the six weighted entry points are declared, exported and bound
without touching the ABI version or the descriptor; they return the documented codes before any launch (NULL weights, a light stride that is
neither 0 nor H W); the Python layer validates the weights' shape before device work and accepts masks of any dtype; the three routes answer
"step" / "fit" with weights as without -- the step classes then launch the weighted kinds -- and send weights that require grad to the
composition; `weights=None` changes no answer.

Also here, for tests/test_gpu_weighted_stack.py: the weight populations (`per_shot_weights`, `shared_weights`, `zero_block`), checked in float64.
The weights multiply squared differences and move no rendered value, so what test_camera_stack_host / test_view_stack_host found about the
images of the fixture cases -- off the clamps, the sRGB knee and the zero dots -- holds for the weighted tests unchanged: no pixel is excluded."""
import ctypes
import os
import re

import pytest
import torch

import abi_header
from pypbr_amd import _native as N
from pypbr_amd import functional as F
from test_light_stack_host import LIGHTS3, _desc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# name, arguments: the unweighted call's and (weights, w_batch_stride, w_light_stride)
NAMES = (("pbr_cook_torrance_weighted_mse_stack_step", 13), ("pbr_cook_torrance_weighted_mse_stack_fit_step", 14),
         ("pbr_cook_torrance_camera_weighted_mse_stack_step", 13), ("pbr_cook_torrance_camera_weighted_mse_stack_fit_step", 14),
         ("pbr_cook_torrance_view_weighted_mse_stack_step", 15), ("pbr_cook_torrance_view_weighted_mse_stack_fit_step", 16))
KINDS = {"stack_w": NAMES[0][0], "fit_w": NAMES[1][0], "camera_stack_w": NAMES[2][0], "camera_fit_w": NAMES[3][0],
         "view_stack_w": NAMES[4][0], "view_fit_w": NAMES[5][0]}


# ------------------------------------------------------------------ the weight populations of the GPU tests
def zero_block(H, W):
    """[H,W] bool: the pixels whose weight is 0 in EVERY shot -- the last row and the first two columns."""
    block = torch.zeros(H, W, dtype=torch.bool)
    block[-1, :] = True
    block[:, :2] = True
    return block


def per_shot_weights(lead, H, W, seed):
    """[*lead, 1, H, W] float32 (`lead` = (L,) or (B, L)): uniform in [0, 2) from a seeded generator, about a quarter of the pixels of every
    shot set to exactly 0, and exactly 0 on `zero_block` in every shot."""
    g = torch.Generator().manual_seed(seed)
    w = torch.rand(*lead, 1, H, W, generator=g) * 2.0
    w[torch.rand(*lead, 1, H, W, generator=g) < 0.25] = 0.0
    w[..., zero_block(H, W)] = 0.0
    return w


def shared_weights(lead, H, W, seed):
    """[*lead, 1, 1, H, W] (`lead` = () or (B,)): ONE plane for all shots, drawn like a shot's of `per_shot_weights`."""
    return per_shot_weights(tuple(lead) + (1,), H, W, seed)


def weight_seed(lead, H, W):
    """The seed of a case's weights in tests/test_gpu_weighted_stack.py: by shape, so that this file checks the very populations used there.
    (The base is the first for which every population below has the properties test_weight_populations asks of it: a draw is an input,
    and at 6 x 16 one shot in six of an arbitrary draw falls a pixel or two short of half.)"""
    return 4106 + 7 * H * W + sum(lead)


# what the GPU tests draw: (lead, H, W) per case -- the camera fixture's shapes (the sixteen shots and the single photograph included) and the
# four orthographic ones
POPULATIONS = [((3,), 7, 12), ((1,), 7, 12), ((3,), 5, 9), ((1,), 5, 9), ((16,), 5, 9), ((2, 3), 6, 16), ((2, 5), 15, 37), ((1, 2), 6, 130),
               ((2, 3), 16, 64), ((1, 3), 14, 44)]


@pytest.mark.parametrize("lead,H,W", POPULATIONS)
def test_weight_populations(lead, H, W):
    """In float64: values in [0, 2), the fixed block exactly 0 in every shot and not empty (17 of 45 pixels at 5 x 9), and every shot with at
    least half of its pixels positive.  5 x 9 is the one shape where the last condition is taken over the pixels OUTSIDE the block: there
    the block alone is 38 % of the plane, so with a quarter of the rest at 0 no population as described can have half of ALL pixels positive
    (28 x 3/4 = 21 of 45); every other shape is held to half of all pixels.  "About a quarter" is checked over all populations together
    (test_about_a_quarter_of_the_weights_is_zero): one 28-pixel shot is too few to say."""
    w = per_shot_weights(lead, H, W, weight_seed(lead, H, W)).double()
    block = zero_block(H, W)
    assert w.shape == tuple(lead) + (1, H, W) and float(w.min()) >= 0.0 and float(w.max()) < 2.0
    assert int(block.sum()) == W + 2 * (H - 1) > 0 and bool((w[..., block] == 0).all())
    outside = w[..., ~block].reshape(-1, int((~block).sum()))                       # one row per shot
    share = (outside if (H, W) == (5, 9) else w.reshape(-1, H * W)) > 0
    assert float(share.double().mean(dim=1).min()) >= 0.5, share.double().mean(dim=1)
    assert bool((outside == 0).any(dim=0).sum() < outside.shape[1]) or len(outside) > 8    # the random zeros are per shot, not one more block
    plane = shared_weights(lead[:-1], H, W, weight_seed(lead[:-1], H, W))
    assert plane.shape == tuple(lead[:-1]) + (1, 1, H, W) and bool((plane[..., block] == 0).all())
    kept = plane[..., ~block].reshape(-1, int((~block).sum())) if (H, W) == (5, 9) else plane.reshape(-1, H * W)
    assert float((kept > 0).double().mean(dim=1).min()) >= 0.5


def test_about_a_quarter_of_the_weights_is_zero():
    """Outside the fixed block, over all populations: the share of exact zeros is 1/4 within four standard deviations of the count drawn."""
    zeros = total = 0
    for lead, H, W in POPULATIONS:
        w = per_shot_weights(lead, H, W, weight_seed(lead, H, W))[..., ~zero_block(H, W)]
        zeros, total = zeros + int((w == 0).sum()), total + w.numel()
    assert abs(zeros / total - 0.25) <= 4 * (0.25 * 0.75 / total) ** 0.5, (zeros, total)


# ------------------------------------------------------------------ ABI and binding
def test_abi_and_descriptor_are_unchanged():
    lib = N.lib()
    assert N.ABI_VERSION == 9 and lib.pbr_abi_version() == 9
    assert lib.pbr_render_desc_size() == ctypes.sizeof(N.RenderDesc) == 632
    assert "#define PBR_HIP_ABI_VERSION 9" in re.sub(r"[ \t]+", " ", abi_header.TEXT)


def test_names_declared_exported_and_bound():
    lib = N.lib()
    for name, n_args in NAMES:
        fn = getattr(lib, name)
        declared = abi_header.declared(name)
        assert len(re.findall(r"int64_t w_(?:batch|light)_stride", declared)) == 2 and fn.argtypes.count(ctypes.c_int64) == 2, name
        # the unweighted sibling keeps its signature: the same arguments without the three
        sibling = getattr(lib, name.replace("weighted_", ""))
        assert len(sibling.argtypes) == n_args - 3, name


def test_step_kinds_and_counters():
    for kind, entry in KINDS.items():
        assert F._STEP_KINDS[kind][0] == entry and F._STEP_KINDS[kind][1] == F._STEP_KINDS[kind[:-2]][1]      # the unweighted kind's workspace
        assert kind in F._WEIGHTED_KINDS and entry[len("pbr_cook_torrance_"):] in F.STACK_LAUNCHES
        assert (kind in F._FIT_KINDS) == ("fit" in kind) and (kind in F._VIEW_KINDS) == kind.startswith("view")
        assert (kind in F._POINT_KINDS) == (kind.startswith("view") or kind.startswith("camera"))
        assert F._step_kind(kind[:-2], torch.ones(1)) == kind and F._step_kind(kind[:-2], None) == kind[:-2]
    assert len(F._WEIGHTED_KINDS) == 6 and "step_w" not in F._STEP_KINDS            # the single-light step has no weighted form


def _call(name, d, weights=1, light_stride=None, batch_stride=None, targets=1, loss=1, workspace=1, g_params=1):
    """An entry point through ctypes with dummy non-NULL addresses: every case here must return before anything is launched or read."""
    buf = (ctypes.c_float * 64)()
    at = lambda on: ctypes.addressof(buf) if on else None
    plane = d.height * d.width
    strides = (d.n_lights * plane if batch_stride is None else batch_stride, plane if light_stride is None else light_stride)
    cams = ((ctypes.c_float * 48)(*([0.0, 0.0, 1.0] * 16)), None) if "_view_" in name else ()
    fit = (at(g_params),) if name.endswith("fit_step") else ()
    return getattr(N.lib(), name)(ctypes.byref(d), *cams, at(targets), at(weights), *strides, None, None, None, None, None, *fit, at(loss),
                                  at(workspace), None)


@pytest.mark.parametrize("name", [n for n, _ in NAMES])
def test_entry_points_return_their_codes_before_any_launch(name):
    d = _desc()
    assert _call(name, d, weights=0) == N.ERR_NULL_MAP                                # NULL weights: like the other pointers
    assert _call(name, d, targets=0) == N.ERR_NULL_MAP and _call(name, d, loss=0) == N.ERR_NULL_MAP and _call(name, d, workspace=0) == N.ERR_NULL_MAP
    if name.endswith("fit_step"):
        assert _call(name, d, g_params=0) == N.ERR_NULL_MAP
    plane = d.height * d.width
    for bad in (1, plane - 1, plane + 1, 2 * plane, -plane, 3 * plane):               # a light stride that is neither 0 nor H W
        assert _call(name, d, light_stride=bad) == N.ERR_SHAPE, bad
    d.n_lights = 17
    assert _call(name, d) == N.ERR_SHAPE and _call(name, d, weights=0) == N.ERR_SHAPE  # the descriptor's own codes come first
    d = _desc(tile=(2, 2))                                                            # tiled maps
    assert _call(name, d) == N.ERR_UNSUPPORTED and _call(name, d, light_stride=1) == N.ERR_UNSUPPORTED
    d = _desc()
    d.out_dtype = N.F16
    assert _call(name, d) == N.ERR_DTYPE
    d = _desc()
    d.albedo.data = None
    assert _call(name, d) == N.ERR_NULL_MAP


# ------------------------------------------------------------------ Python validation
def _cpu_call(weights, B=0, L=3, H=6, W=8, **over):
    lead = (B,) if B else ()
    a, n, r, m = torch.rand(*lead, 3, H, W), torch.rand(*lead, 3, H, W), torch.rand(*lead, 1, H, W), torch.rand(*lead, 1, H, W)
    kw = dict(view_dir=[0.0, 0.0, 1.0], light=torch.tensor((LIGHTS3 * 6)[:L]), light_intensity=[1.0, 1.0, 1.0], light_type="point")
    kw.update(over)
    return F.rendering_loss_mse_stack(a, n, r, m, targets=torch.rand(*lead, L, 3, H, W), weights=weights, **kw)


def test_weight_shapes_are_validated_before_device_work():
    good = [((3, 1, 6, 8), 0), ((1, 1, 6, 8), 0), ((2, 3, 1, 6, 8), 2), ((2, 1, 1, 6, 8), 2)]
    for shape, B in good:
        F._stack_weights(torch.ones(shape), ((B,) if B else ()) + (3, 3, 6, 8))
        for dtype in (torch.float32, torch.float64, torch.float16, torch.bool, torch.uint8):
            F._stack_weights(torch.ones(shape, dtype=dtype), ((B,) if B else ()) + (3, 3, 6, 8))
    bad = [((3, 1, 5, 8), 0), ((3, 1, 6, 9), 0),            # a wrong H, a wrong W
           ((3, 3, 6, 8), 0),                               # a channel count of 3
           ((2, 1, 6, 8), 0), ((4, 1, 6, 8), 0),            # a wrong L
           ((3, 6, 8), 0), ((6, 8), 0),                     # no channel dimension
           ((3, 1, 6, 8), 2), ((1, 3, 1, 6, 8), 2), ((2, 2, 1, 6, 8), 2), ((2, 3, 3, 6, 8), 2), ((1, 1, 1, 6, 8), 0)]
    for shape, B in bad:
        with pytest.raises(ValueError, match="weights must be"):
            F._stack_weights(torch.ones(shape), ((B,) if B else ()) + (3, 3, 6, 8))
        # the public call says so before any device work: CPU maps reach the composition otherwise
        with pytest.raises(ValueError, match="weights must be"):
            _cpu_call(torch.ones(shape), B=B)
    with pytest.raises(ValueError, match="weights must be"):
        F._stack_weights([[1.0]], (3, 3, 6, 8))
    # the single photograph: [1,H,W] / [B,1,H,W]
    a, n, r, m = torch.rand(3, 6, 8), torch.rand(3, 6, 8), torch.rand(1, 6, 8), torch.rand(1, 6, 8)
    kw = dict(view_dir=[0.0, 0.0, 1.0], light=[0.1, 0.1, 1.0], light_intensity=[1.0, 1.0, 1.0], light_type="point")
    for shape in ((3, 6, 8), (6, 8), (1, 5, 8), (1, 1, 6, 8)):
        with pytest.raises(ValueError, match="weights must be"):
            F.rendering_loss_mse(a, n, r, m, target=torch.rand(3, 6, 8), weights=torch.ones(shape), **kw)


def test_the_composition_s_weighted_mean():
    """functional._weighted_mse, the line every fallback ends in: mean over ALL elements of w (out - targets)^2 with the weights broadcast
    over channels (and shots), masks of any dtype converted, differentiable in the weights."""
    g = torch.Generator().manual_seed(5)
    out, targets = torch.rand(2, 3, 3, 6, 8, generator=g, dtype=torch.float64), torch.rand(2, 3, 3, 6, 8, generator=g)
    for w in (per_shot_weights((2, 3), 6, 8, 7), shared_weights((2,), 6, 8, 7)):
        want = float((w.double() * (out.float().double() - targets.double()) ** 2).sum() / out.numel())
        assert abs(float(F._weighted_mse(out, targets, w)) - want) <= 1e-6 * (1 + want)
        for mask in (w > 0, (w > 0).to(torch.uint8)):
            want = float(((w > 0).double() * (out.float().double() - targets.double()) ** 2).sum() / out.numel())
            assert abs(float(F._weighted_mse(out, targets, mask)) - want) <= 1e-6 * (1 + want)
        learned = w.clone().requires_grad_(True)
        F._weighted_mse(out, targets, learned).backward()
        d2 = ((out.float() - targets) ** 2).sum(dim=2, keepdim=True)
        if w.shape[1] == 1:
            d2 = d2.sum(dim=1, keepdim=True)
        assert float((learned.grad - d2 / out.numel()).abs().max()) <= 1e-7
    # an all-ones weight is torch's MSE
    assert abs(float(F._weighted_mse(out, targets, torch.ones(2, 1, 1, 6, 8))) - float(torch.nn.functional.mse_loss(out.float(), targets))) <= 1e-7


# ------------------------------------------------------------------ routing
def test_routing_with_weights():
    a, n, r, m = torch.rand(3, 6, 8), torch.rand(3, 6, 8), torch.rand(1, 6, 8), torch.rand(1, 6, 8)
    maps = (a, n, r, m, None)
    grad_maps = (a.clone().requires_grad_(True), n, r, m, None)
    view, cameras = torch.tensor([0.0, 0.0, 0.6]), torch.tensor([[0.0, 0.0, 0.6], [0.1, 0.0, 0.7], [-0.1, 0.1, 0.5]])
    lights, inten = torch.tensor(LIGHTS3), torch.tensor([1.0, 1.0, 1.0])
    targets = torch.rand(3, 3, 6, 8)
    w = per_shot_weights((3,), 6, 8, 3)
    families = ((F._stack_route, dict(light_type="point"), view, ""), (F._camera_stack_route, dict(light_type="point", view_type="point"), view, "camera_"),
                (F._view_stack_route, dict(light_type="point", view_type="point"), cameras, "view_"))
    for route, kw, v, family in families:
        fitted = (v, lights.clone().requires_grad_(True), inten)
        for weights in (w, w > 0, shared_weights((), 6, 8, 3)):
            # weights and maps requiring grad: the weighted step; weights and a parameter requiring grad: the weighted fit step
            assert route(grad_maps, (v, lights, inten), targets, kw, True, weights) == "step"
            assert route(grad_maps, fitted, targets, kw, True, weights) == "fit" and route(maps, fitted, targets, kw, True, weights) == "fit"
            assert route(maps, (v, lights, inten), targets, kw, True, weights) is None                 # nothing requires grad
            assert route(grad_maps, fitted, targets, kw, False, weights) is None                       # no ROCm device
            assert route(grad_maps, fitted, targets, dict(kw, height_total=12), True, weights) is None  # a row band
            assert route(grad_maps, fitted, targets.clone().requires_grad_(True), kw, True, weights) is None
        # ... and the kinds those answers launch with weights
        stack_kind, fit_kind = {"": ("stack", "fit")}.get(family, (family + "stack", family + "fit"))
        assert F._STEP_KINDS[F._step_kind(stack_kind, w)][0] == "pbr_cook_torrance_%sweighted_mse_stack_step" % family
        assert F._STEP_KINDS[F._step_kind(fit_kind, w)][0] == "pbr_cook_torrance_%sweighted_mse_stack_fit_step" % family
        # weights that require grad: the composition
        learned = w.clone().requires_grad_(True)
        assert route(grad_maps, (v, lights, inten), targets, kw, True, learned) is None
        assert route(grad_maps, fitted, targets, kw, True, learned) is None
        with torch.no_grad():
            assert route(grad_maps, fitted, targets, kw, True, w) is None
        # weights=None: exactly today's answers, positionally and by keyword
        for params, served in (((v, lights, inten), "step"), (fitted, "fit")):
            assert route(grad_maps, params, targets, kw, True) == route(grad_maps, params, targets, kw, on_device=True) == served
            assert route(grad_maps, params, targets, kw, True, None) == served and route(grad_maps, params, targets, kw, weights=None, on_device=True) == served
            assert route(grad_maps, params, targets, kw, False) is None
        assert route(maps, (v, lights, inten), targets, kw, True) is None
    # the view types still exclude each other with weights
    assert F._stack_route(grad_maps, (view, lights, inten), targets, dict(light_type="point", view_type="point"), True, w) is None
    assert F._camera_stack_route(grad_maps, (view, lights, inten), targets, dict(light_type="point"), True, w) is None


# ------------------------------------------------------------------ the one combination of case and camera the sibling files do not cover
def test_sixteen_shots_from_one_position_sit_off_the_kinks():
    """tests/test_gpu_weighted_stack.py also runs test_view_stack_host.sixteen_shots under the FIXED camera (all sixteen shots from the
    case's C), which neither sibling host file looks at.  The conditions of test_the_per_shot_images_sit_off_the_kinks that decide a branch,
    in float64: every linear image >= 0.45 below the upper clamp, >= 3.5e-6 from the sRGB knee, every raw N.V, N.L and N.H >= 1e-4 from zero."""
    import sys
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import camera_oracle as CO
    import torch_oracle as T
    from test_view_stack_host import shot_oracle, sixteen_shots
    c = sixteen_shots()
    cams = c["C"].reshape(1, 3).expand(16, 3).double()
    maps = [None if t is None else t.float().double() for t in c["maps"]]
    H, W = maps[0].shape[-2:]
    linear = shot_oracle(c, torch.float64, cameras=cams, return_srgb=False)
    assert float(linear.max()) <= 1 - 0.45, float(linear.max())
    if c["srgb"]:
        knee = float((shot_oracle(c, torch.float64, cameras=cams) - 0.0404482).abs().min())
        assert knee >= 3.5e-6, knee
    vmap = torch.nn.functional.normalize(CO.view_offsets(cams[0], H, W, c["light_size"]), dim=0)
    n = torch.nn.functional.normalize(maps[1], dim=0)
    for l in range(16):
        lmap, _ = T._light_geometry(c["light_type"], c["lights_t"][l].double(), c["light_size"], H, W, torch.float64, 0, H)
        half = torch.nn.functional.normalize(vmap + lmap, dim=0)
        for what, other in (("N.V", vmap), ("N.L", lmap), ("N.H", half)):
            dot = float((n * other).sum(dim=0).abs().min())
            assert dot >= 1e-4, (l, what, dot)
