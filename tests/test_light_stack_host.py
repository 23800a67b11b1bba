"""Light stacks, host side (no device): the two entry points are declared, exported and bound; their descriptor checks return the documented
codes before any launch; the Python layer rejects a stack it cannot describe before any device work."""
import ctypes
import re

import pytest
import torch

import abi_header
from pypbr_amd import _native as N
from pypbr_amd import functional as F

LIGHTS3 = [[0.1, 0.1, 1.0], [-0.4, 0.2, 0.7], [0.3, -0.3, 0.9]]


def _desc(lights=LIGHTS3, tile=(1, 1), B=2, H=8, W=16):
    a, n, r, m = torch.rand(B, 3, H, W), torch.rand(B, 3, H, W), torch.rand(B, 1, H, W), torch.rand(B, 1, H, W)
    o = torch.empty(B, 3, tile[0] * H, tile[1] * W)
    d = F.build_descriptor(a, n, r, m, None, o, view_dir=[0, 0, 1], light=lights, light_intensity=[1, 1, 1], light_type="point", light_size=None,
                           albedo_is_srgb=True, specular_is_srgb=True, return_srgb=True, convert_to_diffuse_specular=False, y_offset=0,
                           height_total=None, tile=tile)
    d._keep = (a, n, r, m, o)
    return d


def _step(d, targets=1, loss=1, workspace=1):
    """The step through ctypes with dummy non-NULL addresses: every case here must return before anything is launched or read."""
    buf = (ctypes.c_float * 64)()
    at = lambda on: ctypes.addressof(buf) if on else None
    return N.lib().pbr_cook_torrance_mse_stack_step(ctypes.byref(d), at(targets), None, None, None, None, None, at(loss), at(workspace), None)


def test_names_declared_exported_and_bound():
    lib = N.lib()
    assert N.ABI_VERSION == 9 and lib.pbr_abi_version() == 9
    assert "#define PBR_HIP_ABI_VERSION 9" in re.sub(r"[ \t]+", " ", abi_header.TEXT)


def test_step_rejects_null_pointers_too_many_lights_and_tiled_maps():
    lib = N.lib()
    d = _desc()
    assert _step(d, targets=0) == N.ERR_NULL_MAP
    assert _step(d, loss=0) == N.ERR_NULL_MAP
    assert _step(d, workspace=0) == N.ERR_NULL_MAP
    d = _desc()
    d.n_lights = 17
    assert _step(d) == N.ERR_SHAPE
    assert lib.pbr_cook_torrance_stack(ctypes.byref(d), None) == N.ERR_SHAPE
    d = _desc(tile=(2, 2))
    assert d.map_height == 8 and d.height == 16
    assert _step(d) == N.ERR_UNSUPPORTED
    assert lib.pbr_mse_step_workspace_bytes(ctypes.byref(d)) == 0
    assert lib.pbr_cook_torrance_stack(ctypes.byref(d), None) == N.ERR_UNSUPPORTED


def test_forward_stack_rejects_what_it_does_not_serve():
    lib = N.lib()
    d = _desc()
    d.out_dtype = N.F16
    assert lib.pbr_cook_torrance_stack(ctypes.byref(d), None) == N.ERR_DTYPE
    assert _step(d) == N.ERR_DTYPE
    d = _desc()
    d.out_channel_stride = 8 * 16 + 4
    assert lib.pbr_cook_torrance_stack(ctypes.byref(d), None) == N.ERR_UNSUPPORTED
    d = _desc()
    d.out_batch_stride = 4 * 8 * 16
    assert lib.pbr_cook_torrance_stack(ctypes.byref(d), None) == N.ERR_UNSUPPORTED
    d = _desc()
    d.out = None
    assert lib.pbr_cook_torrance_stack(ctypes.byref(d), None) == N.ERR_NULL_MAP


def test_python_validation_raises_before_any_device_work():
    """CPU tensors throughout: a check that ran after the first device access would raise RuntimeError ("no CPU path"), not ValueError."""
    from pypbr_amd.losses import MultiLightRenderingLoss
    a, n, r, m = torch.rand(3, 6, 8), torch.rand(3, 6, 8), torch.rand(1, 6, 8), torch.rand(1, 6, 8)
    kw = dict(view_dir=[0, 0, 1], light_type="point")
    many = [[0.1 * i, 0.0, 1.0] for i in range(17)]
    with pytest.raises(ValueError, match="between 1 and 16 lights"):
        F.cook_torrance_stack(a, n, r, m, light=many, light_intensity=[1, 1, 1], **kw)
    with pytest.raises(ValueError, match="between 1 and 16 lights"):
        F.rendering_loss_mse_stack(a, n, r, m, targets=torch.rand(17, 3, 6, 8), light=many, light_intensity=[1, 1, 1], **kw)
    with pytest.raises(ValueError, match="between 1 and 16 lights"):
        MultiLightRenderingLoss("point", torch.tensor([0.0, 0.0, 1.0]), torch.tensor(many), torch.tensor([1.0, 1.0, 1.0]))
    for rows in (2, 4):
        with pytest.raises(ValueError, match="1 row or one per light"):
            F.cook_torrance_stack(a, n, r, m, light=LIGHTS3, light_intensity=[[1, 1, 1]] * rows, **kw)
        with pytest.raises(ValueError, match="1 row or one per light"):
            F.rendering_loss_mse_stack(a, n, r, m, targets=torch.rand(3, 3, 6, 8), light=LIGHTS3, light_intensity=[[1, 1, 1]] * rows, **kw)
        with pytest.raises(ValueError, match="1 row or one per light"):
            MultiLightRenderingLoss("point", torch.tensor([0.0, 0.0, 1.0]), torch.tensor(LIGHTS3), torch.ones(rows, 3))
    for shape in ((3, 6, 8), (2, 3, 6, 8), (3, 3, 6, 9), (1, 3, 3, 6, 8), (3, 1, 6, 8)):
        with pytest.raises(ValueError, match="targets must be the stack"):
            F.rendering_loss_mse_stack(a, n, r, m, targets=torch.rand(*shape), light=LIGHTS3, light_intensity=[1, 1, 1], **kw)
    with pytest.raises(ValueError, match="targets must be the stack"):       # batched maps want [B,L,3,H,W]
        F.rendering_loss_mse_stack(a[None], n[None], r[None], m[None], targets=torch.rand(3, 3, 6, 8), light=LIGHTS3, light_intensity=[1, 1, 1], **kw)
    # what IS a stack passes the validation and reaches the device layer, which has no CPU path
    with pytest.raises(RuntimeError, match="no CPU"):
        F.rendering_loss_mse_stack(a, n, r, m, targets=torch.rand(3, 3, 6, 8), light=LIGHTS3, light_intensity=[[1, 1, 1]] * 3, **kw)
    loss = MultiLightRenderingLoss("directional", torch.tensor([0.0, 0.0, 1.0]), torch.tensor(LIGHTS3), torch.tensor([[1.0, 1.0, 1.0]]))
    assert loss.n_lights == 3 and loss.brdf.light_type == "directional"
