"""The perspective camera, host side (no device): pbr_cook_torrance_camera, pbr_camera_backward_workspace_bytes and
pbr_cook_torrance_camera_backward are declared, exported and bound without touching the ABI version or the descriptor; they return the
documented codes before any launch; the Python layer rejects what the camera does not serve before any device work; and the fixture
(tests/golden/camera.npz, upstream evaluated pixel by pixel with view_dir = C - P) agrees with tools/camera_oracle.py, the vectorised
statement the GPU tests differentiate."""
import ctypes
import json
import os
import re
import sys

import numpy as np
import pytest
import torch

import abi_header
import torch_oracle as O
from pypbr_amd import _native as N
from pypbr_amd import functional as F
from test_light_stack_host import LIGHTS3, _desc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
import camera_oracle as CO  # noqa: E402

FIXTURE = dict(np.load(os.path.join(ROOT, "tests", "golden", "camera.npz")))
CASES = json.loads(str(FIXTURE["cases"]))
IDS = [c["name"] for c in CASES]


def fixture_case(case):
    """name -> torch tensors of one case (maps as stored: float16 for the fp16 cases), plus the case's flags."""
    get = lambda k: torch.from_numpy(FIXTURE["%s/%s" % (case["name"], k)]) if "%s/%s" % (case["name"], k) in FIXTURE else None
    return dict(case, maps=[get(k) for k in ("albedo", "normal", "roughness", "metallic", "specular")], C=get("camera"), lights_t=get("lights"),
                intens_t=get("intensities"), ref32=get("ref32"), ref64=get("ref64"))


def oracle(c, dtype, maps=None, camera=None, lights=None, intens=None, view_map=None, **over):
    """tools/camera_oracle.py on a fixture case (every material of a batch), with what a test replaces."""
    maps = [None if t is None else (t.float() if t.dtype == torch.float16 else t) for t in (c["maps"] if maps is None else maps)]
    batched = maps[0].dim() == 4
    kw = dict(camera=c["C"] if camera is None else camera, lights=c["lights_t"] if lights is None else lights,
              intensities=c["intens_t"] if intens is None else intens, light_type=c["light_type"], light_size=c["light_size"],
              albedo_is_srgb=c["srgb"], specular_is_srgb=c["srgb"], return_srgb=c["srgb"], converted=c["workflow"] == "converted",
              view_map=view_map, dtype=dtype)
    if c["workflow"] == "converted":
        kw["specular_is_srgb"] = True                        # the converted material's flag upstream, whatever the albedo's
    kw.update(over)
    outs = [CO.cook_torrance_camera(*[None if t is None else (t[b] if batched else t) for t in maps], **kw) for b in range(maps[0].shape[0] if batched else 1)]
    return torch.stack(outs) if batched else outs[0]


def _backward(d, grad_out=1, g_params=0, workspace=0):
    """The entry point through ctypes with dummy non-NULL addresses: every case here must return before anything is launched or read."""
    buf = (ctypes.c_float * 64)()
    at = lambda on: ctypes.addressof(buf) if on else None
    return N.lib().pbr_cook_torrance_camera_backward(ctypes.byref(d), at(grad_out), None, None, None, None, None, at(g_params), at(workspace), None)


def test_abi_and_descriptor_are_unchanged():
    lib = N.lib()
    assert N.ABI_VERSION == 9 and lib.pbr_abi_version() == 9
    assert lib.pbr_render_desc_size() == ctypes.sizeof(N.RenderDesc) == 632
    assert "#define PBR_HIP_ABI_VERSION 9" in re.sub(r"[ \t]+", " ", abi_header.TEXT)


def test_entry_points_return_their_codes_before_any_launch():
    lib = N.lib()
    camera = lambda d: lib.pbr_cook_torrance_camera(ctypes.byref(d), None)
    size = lambda d: lib.pbr_camera_backward_workspace_bytes(ctypes.byref(d))
    d = _desc(tile=(2, 2))                                   # tiled maps
    assert camera(d) == N.ERR_UNSUPPORTED and _backward(d) == N.ERR_UNSUPPORTED and size(d) == 0
    d = _desc()
    d.map_height, d.map_width = d.height_total, d.width      # map_height / map_width set at all: the camera takes plain descriptors only
    assert camera(d) == N.ERR_UNSUPPORTED and _backward(d) == N.ERR_UNSUPPORTED
    d = _desc()
    d.out_dtype = N.F16
    assert camera(d) == N.ERR_DTYPE and _backward(d) == N.ERR_DTYPE and size(d) == 0
    d = _desc()
    d.light_size = float("nan")
    assert _backward(d) == N.ERR_UNSUPPORTED
    d = _desc()
    assert _backward(d, grad_out=0) == N.ERR_NULL_MAP
    assert _backward(d, g_params=1, workspace=0) == N.ERR_NULL_MAP
    # the existing codes for NULL maps and bad shapes
    d = _desc()
    d.albedo.data = None
    assert camera(d) == N.ERR_NULL_MAP and _backward(d) == N.ERR_NULL_MAP
    d = _desc()
    d.out = None
    assert camera(d) == N.ERR_NULL_MAP
    for field, value in (("width", 0), ("n_lights", 17), ("y_offset", -1), ("abi_version", 8)):
        d = _desc()
        setattr(d, field, value)
        assert camera(d) == N.ERR_SHAPE and _backward(d) == N.ERR_SHAPE and size(d) == 0, field
    d = _desc()
    d.height_total = d.height - 1                            # a band taller than its map
    assert camera(d) == N.ERR_SHAPE
    d = _desc()
    d.light_type = 7
    assert camera(d) == N.ERR_LIGHT_TYPE
    d = _desc()
    d.workflow = 5
    assert camera(d) == N.ERR_WORKFLOW


@pytest.mark.parametrize("hw", [(7, 12), (5, 9)])
@pytest.mark.parametrize("L", [1, 3])
def test_workspace_is_the_documented_layout(L, hw):
    """One row of 3 + 6 L floats per workgroup of the one-pixel decomposition (8-byte aligned), then 256 rows of doubles: what
    pbr_param_grad_workspace_bytes promises the orthographic backward."""
    lib = N.lib()
    d = _desc(lights=LIGHTS3[:L], B=2, H=hw[0], W=hw[1])
    assert lib.pbr_camera_backward_workspace_bytes(ctypes.byref(d)) == lib.pbr_param_grad_workspace_bytes(ctypes.byref(d)) > 256 * (3 + 6 * L) * 8


def test_python_validation_needs_no_device():
    a, n, r, m = torch.rand(3, 6, 8), torch.rand(3, 6, 8), torch.rand(1, 6, 8), torch.rand(1, 6, 8)
    kw = dict(view_dir=[0.0, 0.0, 0.6], light=[0.1, 0.1, 1.0], light_intensity=[1.0, 1.0, 1.0])
    for call in (F.cook_torrance, F.plan_cook_torrance):
        with pytest.raises(ValueError, match="view_type"):
            call(a, n, r, m, view_type="perspective", **kw)
        with pytest.raises(NotImplementedError, match="tile"):
            call(a, n, r, m, view_type="point", tile=2, **kw)
        with pytest.raises(NotImplementedError, match="blend"):
            call(a, n, r, m, view_type="point", blend=(a, n, r, m, None, r), **kw)
        with pytest.raises(NotImplementedError, match="float32"):
            call(a, n, r, m, view_type="point", out_dtype=torch.float16, **kw)
    with pytest.raises(ValueError, match="view_type"):
        F.rendering_loss_mse(a, n, r, m, target=torch.rand(3, 6, 8), view_type="fisheye", **kw)
    with pytest.raises(ValueError, match="view_type"):
        F.cook_torrance_stack(a, n, r, m, view_type="fisheye", **kw)
    with pytest.raises(ValueError, match="view_type"):
        F.rendering_loss_mse_stack(a, n, r, m, targets=torch.rand(1, 3, 6, 8), view_type="fisheye", **kw)
    from pypbr_amd.losses import MultiLightRenderingLoss, RenderingLoss
    from pypbr_amd.models import CookTorranceBRDF
    with pytest.raises(ValueError, match="view_type"):
        CookTorranceBRDF(view_type="fisheye")
    assert CookTorranceBRDF().view_type == "directional" and CookTorranceBRDF("point", None, view_type="POINT").view_type == "point"
    assert RenderingLoss(view_type="point").brdf.view_type == "point" and MultiLightRenderingLoss(view_type="point").brdf.view_type == "point"
    # a camera has no one-pass loss step: the routing says so without a device
    grad = (a.clone().requires_grad_(True), n, r, m, None)
    params = (torch.tensor(kw["view_dir"]), torch.tensor([kw["light"]]), torch.tensor(kw["light_intensity"]))
    assert F._stack_route(grad, params, torch.rand(1, 3, 6, 8), dict(light_type="point"), on_device=True) == "step"
    assert F._stack_route(grad, params, torch.rand(1, 3, 6, 8), dict(light_type="point", view_type="point"), on_device=True) is None


@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_the_oracle_is_the_fixture(case):
    """The vectorised statement against upstream pixel by pixel: float64 within 1e-12 of ref64 (measured: 1.2e-16), float32 within 1e-6 of
    ref32 (measured: 6e-8; the margin is for another torch build's normalize)."""
    c = fixture_case(case)
    e64 = float((oracle(c, torch.float64) - c["ref64"]).abs().max())
    e32 = float((oracle(c, torch.float32) - c["ref32"]).abs().max())
    print("%s: |oracle64 - ref64| = %.2e   |oracle32 - ref32| = %.2e" % (case["name"], e64, e32))
    assert c["ref64"].dtype == torch.float64 and c["ref32"].dtype == torch.float32
    assert e64 <= 1e-12 and e32 <= 1e-6


def test_the_fixture_covers_what_it_says():
    got = [fixture_case(c) for c in CASES]
    assert {tuple(c["shape"]) for c in got} == {(7, 12), (5, 9), (2, 6, 16)}
    assert {c["workflow"] for c in got} == {"metallic", "specular", "converted"}
    assert {c["light_type"] for c in got} == {"point", "directional"} and {c["L"] for c in got} == {1, 3}
    assert {c["srgb"] for c in got} == {True, False} and {c["light_size"] for c in got} == {1.0, 2.0}
    assert any(c["maps"][1] is None for c in got) and any(c.get("f16") for c in got)
    assert sorted({tuple(round(float(v), 3) for v in c["C"]) for c in got if not c.get("forward_only")}) == [(0.0, 0.0, 0.6), (0.1, -0.2, 1.5)]
    edge = [c for c in got if c.get("forward_only")]
    assert len(edge) == 1 and tuple(edge[0]["shape"]) == (5, 9) and not edge[0]["C"].any() and torch.isfinite(edge[0]["ref32"]).all()
    for c in got:
        assert all(t is None or t.dtype == (torch.float16 if c.get("f16") else torch.float32) for t in c["maps"])
        assert float(c["maps"][2].min()) >= 0.2 and float(c["maps"][2].max()) <= 1.0
        recorded = json.load(open(os.path.join(ROOT, "tests", "golden", "parity_thresholds.json")))["sets"]
        assert float(c["maps"][2].min()) > max(recorded.values()) + 0.01                       # criterion (i) applies to every value
        if c.get("forward_only"):
            continue
        assert float((c["ref64"] <= 0).double().mean()) <= 0.5 and float((c["ref64"] >= 1).double().mean()) <= 0.5
        if c["maps"][1] is None:
            continue
        normals = c["maps"][1].float().double()
        for nm in (normals if normals.dim() == 4 else normals[None]):
            H, W = nm.shape[-2:]
            v = torch.nn.functional.normalize(CO.view_offsets(c["C"].double(), H, W, c["light_size"]), dim=0)
            ndv = (torch.nn.functional.normalize(nm, dim=0) * v).sum(0)
            assert (ndv < 0).any() and (ndv > 0).any() and (nm[2] > 0).all(), c["name"]         # the sign changes for the camera only


@pytest.mark.parametrize("case", [c for c in CASES if c["L"] == 1 and not c.get("f16")], ids=[c["name"] for c in CASES if c["L"] == 1 and not c.get("f16")])
def test_one_view_for_every_pixel_is_the_orthographic_oracle(case):
    """With every pixel's view forced to one vector the statement IS torch_oracle.cook_torrance: bit for bit in float64."""
    c = fixture_case(case)
    view = torch.tensor([0.2, -0.1, 1.0], dtype=torch.float64)
    a, n, r, m, s = (None if t is None else t.double() for t in c["maps"])
    H, W = a.shape[-2:]
    forced = torch.nn.functional.normalize(view, dim=0).view(3, 1, 1).expand(3, H, W)
    got = oracle(c, torch.float64, view_map=forced)
    kw = dict(view=view, light=c["lights_t"][0].double(), intensity=c["intens_t"][0].double(), light_type=c["light_type"], light_size=c["light_size"],
              return_srgb=c["srgb"])
    if c["workflow"] == "converted":
        want = O.cook_torrance_converted(a, n, r, m, albedo_is_srgb=c["srgb"], **kw)
    else:
        want = O.cook_torrance(a, n, r, m, s, albedo_is_srgb=c["srgb"], specular_is_srgb=c["srgb"], **kw)
    assert torch.equal(got, want)
