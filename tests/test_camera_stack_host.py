"""Light stacks under the perspective camera, host side (no device): pbr_cook_torrance_camera_stack, pbr_cook_torrance_camera_mse_stack_step,
pbr_camera_mse_stack_fit_workspace_bytes and pbr_cook_torrance_camera_mse_stack_fit_step are declared, exported and bound without touching
the ABI version or the descriptor; they return the documented codes before any launch; the fit step's size query is the orthographic fit
layout; and functional._camera_stack_route routes what the one-pass forms serve, while functional._stack_route still answers None for
view_type="point"."""
import ctypes
import re

import pytest
import torch

import abi_header
from pypbr_amd import _native as N
from pypbr_amd import functional as F
from test_light_stack_host import LIGHTS3, _desc



def _at(buf, on):
    return ctypes.addressof(buf) if on else None


def _stack(d):
    return N.lib().pbr_cook_torrance_camera_stack(ctypes.byref(d), None)


def _step(d, targets=1, loss=1, workspace=1):
    """The entry points through ctypes with dummy non-NULL addresses: every case here must return before anything is launched or read."""
    buf = (ctypes.c_float * 64)()
    return N.lib().pbr_cook_torrance_camera_mse_stack_step(ctypes.byref(d), _at(buf, targets), None, None, None, None, None, _at(buf, loss),
                                                           _at(buf, workspace), None)


def _fit(d, g_params=1, targets=1, loss=1, workspace=1):
    buf = (ctypes.c_float * 64)()
    return N.lib().pbr_cook_torrance_camera_mse_stack_fit_step(ctypes.byref(d), _at(buf, targets), None, None, None, None, None,
                                                               _at(buf, g_params), _at(buf, loss), _at(buf, workspace), None)


def _size(d):
    return N.lib().pbr_camera_mse_stack_fit_workspace_bytes(ctypes.byref(d))


def test_abi_and_descriptor_are_unchanged():
    lib = N.lib()
    assert N.ABI_VERSION == 9 and lib.pbr_abi_version() == 9
    assert lib.pbr_render_desc_size() == ctypes.sizeof(N.RenderDesc) == 632
    assert "#define PBR_HIP_ABI_VERSION 9" in re.sub(r"[ \t]+", " ", abi_header.TEXT)


def test_launch_counters_have_the_camera_keys():
    assert {"camera_stack", "camera_mse_stack_step", "camera_mse_stack_fit_step"} <= set(F.STACK_LAUNCHES)
    assert {"cook_torrance_stack", "mse_stack_step", "mse_stack_fit_step"} <= set(F.STACK_LAUNCHES)
    # the steps' keys are what _launch_loss_step forms from the entry points' names
    for kind, key in (("camera_stack", "camera_mse_stack_step"), ("camera_fit", "camera_mse_stack_fit_step")):
        entry, query = F._STEP_KINDS[kind]
        assert entry[len("pbr_cook_torrance_"):] == key and entry in N.EXPORTS and query in N.EXPORTS


def test_entry_points_return_their_codes_before_any_launch():
    d = _desc(tile=(2, 2))                                   # tiled maps
    assert _stack(d) == N.ERR_UNSUPPORTED and _step(d) == N.ERR_UNSUPPORTED and _fit(d) == N.ERR_UNSUPPORTED and _size(d) == 0
    d = _desc()
    d.map_height, d.map_width = d.height_total, d.width      # map_height / map_width set at all: the camera takes plain descriptors only
    assert _stack(d) == N.ERR_UNSUPPORTED and _step(d) == N.ERR_UNSUPPORTED and _fit(d) == N.ERR_UNSUPPORTED and _size(d) == 0
    d = _desc()
    d.out_dtype = N.F16                                      # an fp16 result
    assert _stack(d) == N.ERR_DTYPE and _step(d) == N.ERR_DTYPE and _fit(d) == N.ERR_DTYPE and _size(d) == 0
    for field, value in (("out_channel_stride", 8 * 16 + 4), ("out_batch_stride", 4 * 8 * 16)):      # the stack is contiguous
        d = _desc()
        setattr(d, field, value)
        assert _stack(d) == N.ERR_UNSUPPORTED, field
    for light_type in (N.LIGHT_POINT, N.LIGHT_DIRECTIONAL):  # a NaN grid makes every view vector NaN, whatever the light type
        d = _desc()
        d.light_type, d.light_size = light_type, float("nan")
        assert _step(d) == N.ERR_UNSUPPORTED and _fit(d) == N.ERR_UNSUPPORTED and _size(d) == 0
    d = _desc()
    assert _step(d, targets=0) == N.ERR_NULL_MAP and _step(d, loss=0) == N.ERR_NULL_MAP and _step(d, workspace=0) == N.ERR_NULL_MAP
    assert _fit(d, g_params=0) == N.ERR_NULL_MAP and _fit(d, targets=0) == N.ERR_NULL_MAP
    assert _fit(d, loss=0) == N.ERR_NULL_MAP and _fit(d, workspace=0) == N.ERR_NULL_MAP
    # the existing codes for NULL maps and bad shapes
    d = _desc()
    d.albedo.data = None
    assert _stack(d) == N.ERR_NULL_MAP and _step(d) == N.ERR_NULL_MAP and _fit(d) == N.ERR_NULL_MAP and _size(d) == 0
    d = _desc()
    d.out = None
    assert _stack(d) == N.ERR_NULL_MAP
    for field, value in (("width", 0), ("n_lights", 17), ("y_offset", -1), ("abi_version", 8)):
        d = _desc()
        setattr(d, field, value)
        assert _stack(d) == N.ERR_SHAPE and _step(d) == N.ERR_SHAPE and _fit(d) == N.ERR_SHAPE and _size(d) == 0, field
    d = _desc()
    d.light_type = 7
    assert _stack(d) == N.ERR_LIGHT_TYPE and _step(d) == N.ERR_LIGHT_TYPE
    d = _desc()
    d.workflow = 5
    assert _stack(d) == N.ERR_WORKFLOW and _fit(d) == N.ERR_WORKFLOW


@pytest.mark.parametrize("hw", [(7, 12), (5, 9)])
@pytest.mark.parametrize("L", [1, 3])
def test_fit_workspace_is_the_orthographic_fit_layout(L, hw):
    """The loss partials and their stage sums, one row of 3 + 6 L floats per workgroup of the one-pixel decomposition, their stage sums:
    what pbr_mse_stack_fit_workspace_bytes promises the orthographic fit step -- and nothing for descriptors the camera does not serve."""
    lib = N.lib()
    d = _desc(lights=LIGHTS3[:L], B=2, H=hw[0], W=hw[1])
    assert _size(d) == lib.pbr_mse_stack_fit_workspace_bytes(ctypes.byref(d)) > lib.pbr_mse_step_workspace_bytes(ctypes.byref(d)) + 256 * (3 + 6 * L) * 8
    d = _desc(lights=LIGHTS3[:L], B=2, H=hw[0], W=hw[1], tile=(2, 2))
    assert _size(d) == 0
    d = _desc(lights=LIGHTS3[:L], B=2, H=hw[0], W=hw[1])
    d.out_dtype = N.F16
    assert _size(d) == 0


STACK_CASES = ["A_specular_directional_3", "A_converted_point_3", "A_metallic_point_1", "B_metallic_directional_3", "B_specular_point_1",
               "C_converted_point_3_f16", "C_specular_directional_3_f16"]


@pytest.mark.parametrize("name", STACK_CASES)
def test_the_per_light_images_sit_off_the_kinks(name):
    """What lets tests/test_gpu_camera_stack.py compare every pixel's gradient: in float64 no value of any per-light image of its cases lies
    within 0.45 of the upper clamp or within 3.5e-6 of the sRGB knee (0.0404482 encoded; fp32 error there is ~1e-8), and at most 27 % of an
    image sits on the lower clamp.  (Worst seen: 0.74, 3.52e-6, 26.6 %.)"""
    from test_camera_host import CASES, fixture_case, oracle
    c = fixture_case({k["name"]: k for k in CASES}[name])
    for l in range(c["L"]):
        one = dict(lights=c["lights_t"][l:l + 1], intens=c["intens_t"][l:l + 1])
        linear = oracle(c, torch.float64, return_srgb=False, **one)
        assert float(linear.max()) <= 1 - 0.45, (name, l, float(linear.max()))
        assert float((linear <= 0).double().mean()) <= 0.27, (name, l)
        if c["srgb"]:
            knee = float((oracle(c, torch.float64, **one) - 0.0404482).abs().min())
            assert knee > 3.5e-6, (name, l, knee)


def test_routing():
    """functional._camera_stack_route on CPU tensors, the device requirement factored out; functional._stack_route keeps its answer."""
    a, n, r, m = torch.rand(3, 6, 8), torch.rand(3, 6, 8), torch.rand(1, 6, 8), torch.rand(1, 6, 8)
    maps = (a, n, r, m, None)
    grad_maps = (a.clone().requires_grad_(True), n, r, m, None)
    camera, lights, inten = torch.tensor([0.0, 0.0, 0.6]), torch.tensor(LIGHTS3), torch.tensor([1.0, 1.0, 1.0])
    targets = torch.rand(3, 3, 6, 8)
    kw = dict(light_type="point", view_type="point")
    route = lambda maps, params, targets=targets, kw=kw, on=True: F._camera_stack_route(maps, params, targets, kw, on_device=on)
    assert route(maps, (camera, lights, inten)) is None                                        # nothing requires grad
    assert route(grad_maps, (camera, lights, inten)) == "step"
    assert route(grad_maps, (camera, lights, inten), kw=dict(kw, tile=1, y_offset=0)) == "step"
    for which in range(3):                                                                     # the position, a light, an intensity: each alone
        params = [camera, lights, inten]
        params[which] = params[which].clone().requires_grad_(True)
        assert route(maps, tuple(params)) == "fit"                                             # only the parameters are fitted
        assert route(grad_maps, tuple(params)) == "fit"                                        # together with the maps
    fitted = (camera.clone().requires_grad_(True), lights, inten)
    for params, served in (((camera, lights, inten), "step"), (fitted, "fit")):
        assert route(grad_maps, params) == served
        assert route(grad_maps, params, targets=targets.clone().requires_grad_(True)) is None  # targets that require grad
        assert route(grad_maps, params, on=False) is None                                      # no ROCm device
        assert route(grad_maps, params, kw=dict(kw, view_type="directional")) is None          # the orthographic view is _stack_route's
        assert route(grad_maps, params, kw=dict(light_type="point")) is None                   # ... and it is the default
        assert route(grad_maps, params, kw=dict(kw, height_total=12)) is None                  # a row band
        with torch.no_grad():
            assert route(grad_maps, params) is None
        batched = (a.expand(2, 3, 6, 8).clone().requires_grad_(True), n, r.expand(2, 1, 6, 8), m.expand(2, 1, 6, 8), None)   # the normal is shared
        assert route(batched, params, targets=torch.rand(2, 3, 3, 6, 8)) is None
        own = (batched[0], n.expand(2, 3, 6, 8), batched[2], batched[3], None)
        assert route(own, params, targets=torch.rand(2, 3, 3, 6, 8)) == served
        with pytest.raises(NotImplementedError, match="tile"):                                 # tiled maps: _view_type says so before any routing
            route(grad_maps, params, kw=dict(kw, tile=2))
        # the orthographic route still leaves the camera alone, and still serves the orthographic view
        assert F._stack_route(grad_maps, params, targets, kw, on_device=True) is None
        assert F._stack_route(grad_maps, params, targets, dict(light_type="point"), on_device=True) == served
    assert route(grad_maps, (camera.tolist(), lights.clone().requires_grad_(True), inten.tolist())) == "fit"      # plain lists beside a fitted light
    # the functions the routes name carry the class names the GPU tests look for
    assert F._CameraStackStepFn.__name__ == "_CameraStackStepFn" and F._CameraStackFitFn.__name__ == "_CameraStackFitFn"
    assert len({F._CameraStackStepFn, F._CameraStackFitFn, F._MseStackStepFn, F._MseStackFitFn}) == 4
