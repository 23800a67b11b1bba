"""Light stacks with one camera position per shot, host side (no device): pbr_cook_torrance_view_stack, pbr_cook_torrance_view_mse_stack_step,
pbr_view_mse_stack_fit_workspace_bytes and pbr_cook_torrance_view_mse_stack_fit_step are declared, exported and bound without touching the ABI
version or the descriptor; they return the documented codes before any launch (both or neither camera pointer included); the fit step's size
query is the camera fit layout with rows of 9 L floats; the Python layer validates `view_dir` by element count; functional._view_stack_route
routes what the one-pass forms serve while _camera_stack_route and _stack_route answer as before; the per-shot oracle with equal cameras is the
fixture's single-camera evaluation; and the cameras tests/test_gpu_view_stack.py uses keep every per-shot image off the kinks."""
import ctypes
import os
import re
import sys

import pytest
import torch

import abi_header
from pypbr_amd import _native as N
from pypbr_amd import functional as F
from test_camera_host import CASES, fixture_case, oracle
from test_light_stack_host import LIGHTS3, _desc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
import camera_oracle as CO  # noqa: E402
import torch_oracle as T  # noqa: E402

STACK_CASES = ["A_specular_directional_3", "A_converted_point_3", "A_metallic_point_1", "B_metallic_directional_3", "B_specular_point_1",
               "C_converted_point_3_f16", "C_specular_directional_3_f16"]
DELTAS = torch.tensor([[0.0, 0.0, 0.0], [0.15, -0.10, 0.05], [-0.20, 0.12, -0.04]])      # camera l of a case is C + DELTAS[l]
BY_NAME = {k["name"]: k for k in CASES}


def cameras_of(c):
    """[L,3]: the case's camera moved by DELTAS[l] for shot l."""
    return c["C"].reshape(1, 3) + DELTAS[:c["L"]]


def sixteen_shots():
    """The 5 x 9 fixture case (one-pixel lanes, specular workflow, point lights) under SIXTEEN shots: rows of 144 parameter sums.  Lights and
    cameras are drawn once from a fixed seed, the flash a few centimetres from the lens; intensities differ per shot and per channel."""
    c = fixture_case(BY_NAME["B_specular_point_1"])
    g = torch.Generator().manual_seed(1605)
    cams = c["C"].reshape(1, 3) + (torch.rand(16, 3, generator=g) - 0.5) * torch.tensor([0.2, 0.2, 0.2])
    lights = cams + (torch.rand(16, 3, generator=g) - 0.5) * 0.2
    intens = c["intens_t"].reshape(-1, 3)[:1] * (0.3 + 0.4 * torch.rand(16, 3, generator=g))
    return dict(c, name="B_specular_point_16", L=16, lights_t=lights, intens_t=intens, cameras=cams)


def shot_oracle(c, dtype, maps=None, cameras=None, lights=None, intens=None, **over):
    """[L,3,H,W] / [B,L,3,H,W]: image l is tools/camera_oracle.py called with camera l and light l alone."""
    cameras = cameras_of(c) if cameras is None else cameras
    lights = c["lights_t"] if lights is None else lights
    intens = c["intens_t"] if intens is None else intens
    rows = intens.reshape(-1, 3)
    images = [oracle(c, dtype, maps=maps, camera=cameras[l], lights=lights.reshape(-1, 3)[l:l + 1],
                     intens=rows[l:l + 1] if rows.shape[0] > 1 else rows, **over) for l in range(c["L"])]
    return torch.stack(images, dim=-4)


def _at(buf, on):
    return ctypes.addressof(buf) if on else None


def _cams(host, device):
    """(cameras_host, cameras_device) for the C ABI: a float[16][3] block and a dummy non-NULL address."""
    block = (ctypes.c_float * 48)(*([0.0, 0.0, 1.0] * 16))
    return (block if host else None), (ctypes.addressof(block) if device else None), block


def _stack(d, host=1, device=0):
    h, dv, keep = _cams(host, device)
    return N.lib().pbr_cook_torrance_view_stack(ctypes.byref(d), h, dv, None)


def _step(d, targets=1, loss=1, workspace=1, host=1, device=0):
    """The entry points through ctypes with dummy non-NULL addresses: every case here must return before anything is launched or read."""
    buf = (ctypes.c_float * 64)()
    h, dv, keep = _cams(host, device)
    return N.lib().pbr_cook_torrance_view_mse_stack_step(ctypes.byref(d), h, dv, _at(buf, targets), None, None, None, None, None, _at(buf, loss),
                                                         _at(buf, workspace), None)


def _fit(d, g_params=1, targets=1, loss=1, workspace=1, host=1, device=0):
    buf = (ctypes.c_float * 64)()
    h, dv, keep = _cams(host, device)
    return N.lib().pbr_cook_torrance_view_mse_stack_fit_step(ctypes.byref(d), h, dv, _at(buf, targets), None, None, None, None, None,
                                                             _at(buf, g_params), _at(buf, loss), _at(buf, workspace), None)


def _size(d):
    return N.lib().pbr_view_mse_stack_fit_workspace_bytes(ctypes.byref(d))


def test_abi_and_descriptor_are_unchanged():
    lib = N.lib()
    assert N.ABI_VERSION == 9 and lib.pbr_abi_version() == 9
    assert lib.pbr_render_desc_size() == ctypes.sizeof(N.RenderDesc) == 632
    assert "#define PBR_HIP_ABI_VERSION 9" in re.sub(r"[ \t]+", " ", abi_header.TEXT)


def test_launch_counters_and_step_kinds():
    assert {"view_stack", "view_mse_stack_step", "view_mse_stack_fit_step"} <= set(F.STACK_LAUNCHES)
    assert {"camera_stack", "camera_mse_stack_step", "camera_mse_stack_fit_step", "cook_torrance_stack", "mse_stack_step",
            "mse_stack_fit_step"} <= set(F.STACK_LAUNCHES)
    for kind, key in (("view_stack", "view_mse_stack_step"), ("view_fit", "view_mse_stack_fit_step")):
        entry, query = F._STEP_KINDS[kind]
        assert entry[len("pbr_cook_torrance_"):] == key and entry in N.EXPORTS and query in N.EXPORTS
    assert "view_fit" in F._FIT_KINDS and "view_stack" not in F._FIT_KINDS


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
    # exactly one source of positions
    for host, device in ((0, 0), (1, 1)):
        assert _stack(d, host=host, device=device) == N.ERR_NULL_MAP
        assert _step(d, host=host, device=device) == N.ERR_NULL_MAP
        assert _fit(d, host=host, device=device) == N.ERR_NULL_MAP
    # ... and the gate's own codes whichever source is named (a device pointer is not read before the launch either)
    d = _desc(tile=(2, 2))
    assert _stack(d, host=0, device=1) == N.ERR_UNSUPPORTED and _step(d, host=0, device=1) == N.ERR_UNSUPPORTED
    assert _fit(d, host=0, device=1) == N.ERR_UNSUPPORTED
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
@pytest.mark.parametrize("L", [1, 3, 16])
def test_fit_workspace_is_the_camera_fit_layout_with_rows_of_9L(L, hw):
    """The loss partials and their stage sums, one row of 9 L floats per workgroup of the one-pixel decomposition (8-byte aligned), 256 rows
    of fp64 stage sums -- and nothing for descriptors the camera does not serve."""
    lib = N.lib()
    lights = (LIGHTS3 * 6)[:L]
    d = _desc(lights=lights, B=2, H=hw[0], W=hw[1])
    loss_part = lib.pbr_mse_step_workspace_bytes(ctypes.byref(d))
    lg = 0
    while (1 << lg) < hw[1] and lg < 6:
        lg += 1
    bx, by = 1 << lg, 64 >> lg
    most = -(-hw[1] // bx) * -(-(2 * hw[0]) // by)                                    # one-pixel lanes, 64-lane workgroups: the most any launch has
    camera_rows = (most * (3 + 6 * L) * 4 + 7) & ~7                                   # the camera fit layout, the same count of rows
    assert lib.pbr_camera_mse_stack_fit_workspace_bytes(ctypes.byref(d)) == loss_part + camera_rows + 256 * (3 + 6 * L) * 8
    rows = (most * 9 * L * 4 + 7) & ~7
    assert _size(d) == loss_part + rows + 256 * 9 * L * 8 > 0
    d = _desc(lights=lights, B=2, H=hw[0], W=hw[1], tile=(2, 2))
    assert _size(d) == 0
    d = _desc(lights=lights, B=2, H=hw[0], W=hw[1])
    d.out_dtype = N.F16
    assert _size(d) == 0


def test_view_dir_shapes_are_validated_by_element_count():
    assert F._stack_views([0.0, 0.0, 1.0], 3) == 1 and F._stack_views(torch.zeros(1, 3), 3) == 1        # 3 values: one view for all shots
    assert F._stack_views(torch.zeros(3, 3), 3) == 3 and F._stack_views(torch.zeros(9), 3) == 3         # 3 L values: one per shot
    assert F._stack_views(torch.zeros(1, 3), 1) == 1 and F._stack_views(torch.zeros(3), 1) == 1         # L = 1: the same thing
    for bad in (torch.zeros(2, 3), torch.zeros(4), torch.zeros(4, 3), torch.zeros(0), [0.0, 1.0]):
        with pytest.raises(ValueError, match=r"\[3\].*\[L,3\]"):
            F._stack_views(bad, 3)
    # the public calls say so before any device work: CPU maps would otherwise raise RuntimeError (no CPU path)
    a, n, r, m = torch.rand(3, 6, 8), torch.rand(3, 6, 8), torch.rand(1, 6, 8), torch.rand(1, 6, 8)
    kw = dict(light=torch.tensor(LIGHTS3), light_intensity=[1.0, 1.0, 1.0], light_type="point", view_type="point")
    for bad in (torch.zeros(2, 3), torch.zeros(4)):
        with pytest.raises(ValueError, match=r"\[3\].*\[L,3\]"):
            F.cook_torrance_stack(a, n, r, m, view_dir=bad, **kw)
        with pytest.raises(ValueError, match=r"\[3\].*\[L,3\]"):
            F.rendering_loss_mse_stack(a, n, r, m, targets=torch.rand(3, 3, 6, 8), view_dir=bad, **kw)
        from pypbr_amd.losses import MultiLightRenderingLoss
        with pytest.raises(ValueError, match=r"\[3\].*\[L,3\]"):
            MultiLightRenderingLoss("point", bad, torch.tensor(LIGHTS3), torch.tensor([1.0, 1.0, 1.0]), view_type="point")
    # host positions for the launch: L rows of three, as a float block; never a device tensor
    host, dev = F._camera_rows(torch.tensor(LIGHTS3), 3, torch.device("cpu"))
    assert dev is None and len(host) == 9 and [round(x, 6) for x in host] == [round(x, 6) for row in LIGHTS3 for x in row]
    with pytest.raises(ValueError):
        F._camera_rows(torch.zeros(2, 3), 3, torch.device("cpu"))


def test_routing():
    """functional._view_stack_route on CPU tensors, the device requirement factored out; _camera_stack_route and _stack_route answer as
    before for a single position."""
    a, n, r, m = torch.rand(3, 6, 8), torch.rand(3, 6, 8), torch.rand(1, 6, 8), torch.rand(1, 6, 8)
    maps = (a, n, r, m, None)
    grad_maps = (a.clone().requires_grad_(True), n, r, m, None)
    cameras, lights, inten = torch.tensor([[0.0, 0.0, 0.6], [0.1, 0.0, 0.7], [-0.1, 0.1, 0.5]]), torch.tensor(LIGHTS3), torch.tensor([1.0, 1.0, 1.0])
    targets = torch.rand(3, 3, 6, 8)
    kw = dict(light_type="point", view_type="point")
    route = lambda maps, params, targets=targets, kw=kw, on=True: F._view_stack_route(maps, params, targets, kw, on_device=on)
    assert route(maps, (cameras, lights, inten)) is None                                       # nothing requires grad
    assert route(grad_maps, (cameras, lights, inten)) == "step"
    assert route(grad_maps, (cameras, lights, inten), kw=dict(kw, tile=1, y_offset=0)) == "step"
    for which in range(3):                                                                     # the positions, a light, an intensity: each alone
        params = [cameras, lights, inten]
        params[which] = params[which].clone().requires_grad_(True)
        assert route(maps, tuple(params)) == "fit"
        assert route(grad_maps, tuple(params)) == "fit"
    fitted = (cameras.clone().requires_grad_(True), lights, inten)
    for params, served in (((cameras, lights, inten), "step"), (fitted, "fit")):
        assert route(grad_maps, params, targets=targets.clone().requires_grad_(True)) is None  # targets that require grad
        assert route(grad_maps, params, on=False) is None                                      # no ROCm device
        assert route(grad_maps, params, kw=dict(kw, view_type="directional")) is None          # one orthographic direction per shot: the composition
        assert route(grad_maps, params, kw=dict(light_type="point")) is None
        assert route(grad_maps, params, kw=dict(kw, height_total=12)) is None                  # a row band
        with torch.no_grad():
            assert route(grad_maps, params) is None
        batched = (a.expand(2, 3, 6, 8).clone().requires_grad_(True), n, r.expand(2, 1, 6, 8), m.expand(2, 1, 6, 8), None)   # the normal is shared
        assert route(batched, params, targets=torch.rand(2, 3, 3, 6, 8)) is None
        own = (batched[0], n.expand(2, 3, 6, 8), batched[2], batched[3], None)
        assert route(own, params, targets=torch.rand(2, 3, 3, 6, 8)) == served
        with pytest.raises(NotImplementedError, match="tile"):
            route(grad_maps, params, kw=dict(kw, tile=2))
    # a single position: the routes that existed answer as they did
    camera = torch.tensor([0.0, 0.0, 0.6])
    for params, served in (((camera, lights, inten), "step"), ((camera.clone().requires_grad_(True), lights, inten), "fit")):
        assert F._camera_stack_route(grad_maps, params, targets, kw, on_device=True) == served
        assert F._camera_stack_route(grad_maps, params, targets, dict(light_type="point"), on_device=True) is None
        assert F._stack_route(grad_maps, params, targets, kw, on_device=True) is None
        assert F._stack_route(grad_maps, params, targets, dict(light_type="point"), on_device=True) == served
    assert F._ViewStackStepFn.__name__ == "_ViewStackStepFn" and F._ViewStackFitFn.__name__ == "_ViewStackFitFn"
    assert len({F._ViewStackStepFn, F._ViewStackFitFn, F._CameraStackStepFn, F._CameraStackFitFn, F._MseStackStepFn, F._MseStackFitFn}) == 6


@pytest.mark.parametrize("name", STACK_CASES)
def test_equal_cameras_are_the_single_camera_oracle(name):
    """With all L cameras equal to C, image l of the per-shot oracle is the fixture's single-camera evaluation for light l alone, bit for bit
    (it is the same call); for one light that is the golden image itself, which upstream evaluated pixel by pixel."""
    c = fixture_case(BY_NAME[name])
    same = c["C"].reshape(1, 3).expand(c["L"], 3)
    for dtype in (torch.float32, torch.float64):
        stack = shot_oracle(c, dtype, cameras=same)
        for l in range(c["L"]):
            one = oracle(c, dtype, lights=c["lights_t"][l:l + 1], intens=c["intens_t"][l:l + 1])
            assert torch.equal(stack.select(-4, l), one), (name, l)
        if c["L"] == 1:
            ref = c["ref32"] if dtype == torch.float32 else c["ref64"]
            assert float((stack.select(-4, 0).double() - ref.double()).abs().max()) <= (1e-5 if dtype == torch.float32 else 1e-12), name


@pytest.mark.parametrize("name", STACK_CASES + ["B_specular_point_16"])
def test_the_per_shot_images_sit_off_the_kinks(name):
    """What lets tests/test_gpu_view_stack.py compare every pixel's gradient, in float64 for cameras C + DELTAS[l]: every per-shot linear image
    stays >= 0.45 below the upper clamp, has <= 27 % of its values on the lower clamp, is >= 3.5e-6 from the sRGB knee (0.0404482 encoded),
    and every raw N.V_l, N.L_l and N.H_l is >= 1e-4 from zero.  (Worst seen: maximum 0.256, 26.6 %, 2.4e-5, 2.2e-4.)  The sixteen shots of
    `sixteen_shots` are held to the three conditions that decide a branch -- upper clamp, knee, dots (worst seen: maximum 0.347, 4.3e-5,
    8.9e-4) -- and to 40 % on the lower clamp: with the flash beside the lens a third of this material faces away from every shot (33.3 %),
    and how much of an image is dark bears on how many pixels carry a gradient, not on which branch float32 takes."""
    c = sixteen_shots() if name == "B_specular_point_16" else fixture_case(BY_NAME[name])
    cams = c.get("cameras", cameras_of(c)).double()
    maps = [None if t is None else t.float().double() for t in c["maps"]]
    batched = maps[0].dim() == 4
    H, W = maps[0].shape[-2:]
    for l in range(c["L"]):
        one = dict(cameras=cams, lights=c["lights_t"], intens=c["intens_t"])
        linear = shot_oracle(c, torch.float64, return_srgb=False, **one).select(-4, l)
        assert float(linear.max()) <= 1 - 0.45, (name, l, float(linear.max()))
        assert float((linear <= 0).double().mean()) <= (0.40 if c["L"] == 16 else 0.27), (name, l)
        if c["srgb"]:
            knee = float((shot_oracle(c, torch.float64, **one).select(-4, l) - 0.0404482).abs().min())
            assert knee >= 3.5e-6, (name, l, knee)
        vmap = torch.nn.functional.normalize(CO.view_offsets(cams[l], H, W, c["light_size"]), dim=0)
        lmap, _ = T._light_geometry(c["light_type"], c["lights_t"][l].double(), c["light_size"], H, W, torch.float64, 0, H)
        half = torch.nn.functional.normalize(vmap + lmap, dim=0)
        normals = [maps[1][b] for b in range(maps[1].shape[0])] if batched and maps[1] is not None else [maps[1]]
        for normal in normals:
            n = torch.tensor([0.0, 0.0, 1.0], dtype=torch.float64).view(3, 1, 1).expand(3, H, W) if normal is None else torch.nn.functional.normalize(normal, dim=0)
            for what, other in (("N.V", vmap), ("N.L", lmap), ("N.H", half)):
                dot = float((n * other).sum(dim=0).abs().min())
                assert dot >= 1e-4, (name, l, what, dot)
