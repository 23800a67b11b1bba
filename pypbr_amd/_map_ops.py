"""Stand-alone map operations with their backward kernels: the colour transfers (pypbr/utils/functions.py:31-66), the
metallic <-> specular conversions (materials/metallic.py:98-108, materials/diffuse.py:128-147) and decode_normal (materials/base.py:191-242):
csrc/map_ops.hip; MaterialBase.resize for one map (base.py:490-504): csrc/resize.hip, its gradient csrc/resize_backward.hip."""
from typing import Optional

import torch

from . import _native as N
from ._dispatch import _DTYPES, _device_tensor, _grad_like, _needs_grad, launch, ptr


def _colour_raw(t: torch.Tensor, to_linear: bool) -> torch.Tensor:
    out = torch.empty_like(t)
    fn = N.lib().pbr_srgb_to_linear if to_linear else N.lib().pbr_linear_to_srgb
    launch(t.device, fn, t.data_ptr(), out.data_ptr(), t.numel(), _DTYPES[t.dtype])
    return out


class _ColourFn(torch.autograd.Function):
    """srgb_to_linear / linear_to_srgb with their backward kernels (pbr_*_backward): the reference's colour transfers are plain
    torch ops (functions.py:31-66), so a rendering loss differentiates through material.to_linear() / linear_albedo."""

    @staticmethod
    def forward(ctx, texture, to_linear):
        t = _device_tensor(texture.detach(), "srgb_to_linear" if to_linear else "linear_to_srgb")
        ctx.save_for_backward(t)
        ctx.to_linear = to_linear
        return _colour_raw(t, to_linear)

    @staticmethod
    def backward(ctx, grad_out):
        (t,) = ctx.saved_tensors
        g = _grad_like(grad_out, t)
        gin = torch.empty_like(t)
        fn = N.lib().pbr_srgb_to_linear_backward if ctx.to_linear else N.lib().pbr_linear_to_srgb_backward
        launch(t.device, fn, t.data_ptr(), g.data_ptr(), gin.data_ptr(), t.numel(), _DTYPES[t.dtype])
        return gin, None


def srgb_to_linear(texture: torch.Tensor) -> torch.Tensor:
    """utils.srgb_to_linear (pypbr/utils/functions.py:31-47) on the device; differentiable (its own backward kernel)."""
    if _needs_grad(texture):
        return _ColourFn.apply(texture, True)
    return _colour_raw(_device_tensor(texture, "srgb_to_linear"), True)


def linear_to_srgb(texture: torch.Tensor) -> torch.Tensor:
    """utils.linear_to_srgb (pypbr/utils/functions.py:50-66) on the device; differentiable (its own backward kernel)."""
    if _needs_grad(texture):
        return _ColourFn.apply(texture, False)
    return _colour_raw(_device_tensor(texture, "linear_to_srgb"), False)


def _m2ds_raw(a, m, albedo_is_srgb):
    diffuse, spec = torch.empty_like(a), torch.empty_like(a)
    P = a.shape[-1] * a.shape[-2]
    launch(a.device, N.lib().pbr_metallic_to_specular, a.data_ptr(), m.data_ptr(), diffuse.data_ptr(), spec.data_ptr(),
           a.numel() // (3 * P), P, int(albedo_is_srgb), _DTYPES[a.dtype])
    return diffuse, spec


class _MetallicToSpecularFn(torch.autograd.Function):
    """to_diffuse_specular_material's arithmetic (metallic.py:98-108) with its backward kernel."""

    @staticmethod
    def forward(ctx, albedo, metallic, albedo_is_srgb):
        a, m = albedo.detach(), metallic.detach()
        ctx.save_for_backward(a, m)
        ctx.srgb = bool(albedo_is_srgb)
        return _m2ds_raw(a, m, albedo_is_srgb)

    @staticmethod
    def backward(ctx, g_diffuse, g_specular):
        a, m = ctx.saved_tensors
        gd = None if g_diffuse is None else _grad_like(g_diffuse, a)
        gs = None if g_specular is None else _grad_like(g_specular, a)
        ga = torch.empty_like(a) if ctx.needs_input_grad[0] else None
        gm = torch.empty_like(m) if ctx.needs_input_grad[1] else None
        P = a.shape[-1] * a.shape[-2]
        launch(a.device, N.lib().pbr_metallic_to_specular_backward, a.data_ptr(), m.data_ptr(), ptr(gd), ptr(gs), ptr(ga), ptr(gm),
               a.numel() // (3 * P), P, int(ctx.srgb), _DTYPES[a.dtype])
        return ga, gm, None


def metallic_to_diffuse_specular(albedo: torch.Tensor, metallic: torch.Tensor, albedo_is_srgb: bool = False):
    """Arithmetic of to_diffuse_specular_material (metallic.py:98-108).  albedo [..,3,H,W],
    metallic [..,1,H,W] -> (diffuse, specular) both [..,3,H,W] in linear space.  Differentiable w.r.t. both maps."""
    a = _device_tensor(albedo, "metallic_to_diffuse_specular")
    m = _device_tensor(metallic, "metallic_to_diffuse_specular")
    if a.shape[-3] != 3 or m.shape[-3] != 1 or a.shape[-2:] != m.shape[-2:] or a.shape[:-3] != m.shape[:-3]:
        raise ValueError("albedo [..,3,H,W] / metallic [..,1,H,W] expected, got %s / %s" % (tuple(a.shape), tuple(m.shape)))
    if m.dtype != a.dtype:
        m = m.to(a.dtype)
    if _needs_grad(a, m):
        return _MetallicToSpecularFn.apply(a, m, bool(albedo_is_srgb))
    return _m2ds_raw(a, m, albedo_is_srgb)


def _ds2bm_raw(d, s, albedo_is_srgb):
    base, met = torch.empty_like(d), torch.empty_like(d)
    launch(d.device, N.lib().pbr_specular_to_metallic, d.data_ptr(), s.data_ptr(), base.data_ptr(), met.data_ptr(),
           d.numel(), int(albedo_is_srgb), _DTYPES[d.dtype])
    return base, met


class _SpecularToMetallicFn(torch.autograd.Function):
    """to_basecolor_metallic_material's arithmetic (diffuse.py:128-147) with its backward kernel (torch's sub-gradients through
    clamp / where; the thresholded selects are re-taken with the forward's own arithmetic)."""

    @staticmethod
    def forward(ctx, diffuse, specular, albedo_is_srgb):
        d, s = diffuse.detach(), specular.detach()
        ctx.save_for_backward(d, s)
        ctx.srgb = bool(albedo_is_srgb)
        return _ds2bm_raw(d, s, albedo_is_srgb)

    @staticmethod
    def backward(ctx, g_basecolor, g_metallic):
        d, s = ctx.saved_tensors
        gb = None if g_basecolor is None else _grad_like(g_basecolor, d)
        gm = None if g_metallic is None else _grad_like(g_metallic, d)
        gd = torch.empty_like(d) if ctx.needs_input_grad[0] else None
        gs = torch.empty_like(s) if ctx.needs_input_grad[1] else None
        launch(d.device, N.lib().pbr_specular_to_metallic_backward, d.data_ptr(), s.data_ptr(), ptr(gb), ptr(gm), ptr(gd), ptr(gs), d.numel(),
               int(ctx.srgb), _DTYPES[d.dtype])
        return gd, gs, None


def diffuse_specular_to_basecolor_metallic(diffuse: torch.Tensor, specular: torch.Tensor, albedo_is_srgb: bool = False):
    """Arithmetic of to_basecolor_metallic_material (diffuse.py:128-147): RAW specular in,
    (basecolor, 3-channel metallic) out.  Differentiable w.r.t. both maps."""
    d = _device_tensor(diffuse, "diffuse_specular_to_basecolor_metallic")
    s = _device_tensor(specular, "diffuse_specular_to_basecolor_metallic")
    if d.shape != s.shape:
        raise ValueError("diffuse %s and specular %s must have the same shape" % (tuple(d.shape), tuple(s.shape)))
    if s.dtype != d.dtype:
        s = s.to(d.dtype)
    if _needs_grad(d, s):
        return _SpecularToMetallicFn.apply(d, s, bool(albedo_is_srgb))
    return _ds2bm_raw(d, s, albedo_is_srgb)


def _resize_raw(t: torch.Tensor, ho: int, wo: int, antialias: bool) -> torch.Tensor:
    h, w = t.shape[-2:]
    planes = t.numel() // (h * w)
    out = torch.empty(t.shape[:-2] + (ho, wo), dtype=t.dtype, device=t.device)
    lib = N.lib()
    ws = torch.empty(lib.pbr_resize_workspace_bytes(planes, h, wo) // 4, dtype=torch.float32, device=t.device)
    launch(t.device, lib.pbr_resize_bilinear, t.data_ptr(), out.data_ptr(), planes, h, w, ho, wo, int(bool(antialias)), ws.data_ptr())
    return out


class _ResizeFn(torch.autograd.Function):
    """MaterialBase.resize for one map with its backward kernel (the transposed tap matrices: pbr_resize_bilinear_backward)."""

    @staticmethod
    def forward(ctx, texture, ho, wo, antialias):
        t = texture.detach().contiguous()
        ctx.geom = (tuple(t.shape), ho, wo, bool(antialias))
        return _resize_raw(t, ho, wo, antialias)

    @staticmethod
    def backward(ctx, grad_out):
        shape, ho, wo, antialias = ctx.geom
        h, w = shape[-2:]
        g = grad_out.to(torch.float32).contiguous()
        planes = g.numel() // (ho * wo)
        gin = torch.empty(shape, dtype=torch.float32, device=g.device)
        lib = N.lib()
        ws = torch.empty(max(1, lib.pbr_resize_backward_workspace_bytes(planes, h, w, ho, wo) // 4), dtype=torch.float32, device=g.device)
        launch(g.device, lib.pbr_resize_bilinear_backward, g.data_ptr(), gin.data_ptr(), planes, h, w, ho, wo, int(antialias), ws.data_ptr())
        return gin, None, None, None


def resize(texture: torch.Tensor, size, antialias: bool = True) -> torch.Tensor:
    """MaterialBase.resize for one map (base.py:490-504 -> torchvision resize of a float tensor):
    bilinear, align_corners=False, optional antialiasing.  `size` = (h, w), or an int that fixes the
    SMALLER edge and keeps the aspect ratio (torchvision semantics).  [..., H, W] float32 on device.
    Differentiable (its own backward kernel), as F.interpolate is upstream."""
    if not texture.is_cuda:
        raise RuntimeError("resize needs a tensor on a ROCm device; there is no CPU path")
    if texture.dtype != torch.float32:
        raise TypeError("resize supports float32 maps, got %s" % texture.dtype)
    h, w = texture.shape[-2:]
    if isinstance(size, (list, tuple)) and len(size) == 1:
        size = size[0]
    if isinstance(size, int):
        short, long = (w, h) if w <= h else (h, w)
        new_short, new_long = size, int(size * long / short)
        size = (new_long, new_short) if w <= h else (new_short, new_long)
    ho, wo = int(size[0]), int(size[1])
    if _needs_grad(texture):
        return _ResizeFn.apply(texture, ho, wo, bool(antialias))
    return _resize_raw(texture.contiguous(), ho, wo, antialias)


def _decode_normal_raw(t: torch.Tensor, out: Optional[torch.Tensor] = None):
    C, H, W = t.shape
    if out is None:
        out = torch.empty((3, H, W), dtype=t.dtype, device=t.device)
    flag = torch.empty(1, dtype=torch.int32, device=t.device)
    launch(t.device, N.lib().pbr_decode_normal, t.data_ptr(), out.data_ptr(), C, H * W, _DTYPES[t.dtype], flag.data_ptr())
    return out, flag


class _DecodeNormalFn(torch.autograd.Function):
    """A predicted normal map assigned to a material in a rendering loss (06_advanced.rst:73-107) must keep its
    gradient: forward = pbr_decode_normal, backward = pbr_decode_normal_backward (float32)."""

    @staticmethod
    def forward(ctx, normal_map):
        t = normal_map.detach().contiguous()
        out, flag = _decode_normal_raw(t)
        ctx.save_for_backward(normal_map)
        ctx.flag = flag
        return out

    @staticmethod
    def backward(ctx, grad_out):
        (normal_map,) = ctx.saved_tensors
        t, g = normal_map.detach().contiguous(), grad_out.to(torch.float32).contiguous()
        gin = torch.empty_like(t)
        launch(t.device, N.lib().pbr_decode_normal_backward, t.data_ptr(), g.data_ptr(), gin.data_ptr(), t.shape[0],
               t.shape[1] * t.shape[2], ctx.flag.data_ptr())
        return gin


def decode_normal(normal_map: torch.Tensor) -> torch.Tensor:
    """MaterialBase._process_normal_map (base.py:191-242) on the device: (2|3,H,W) -> (3,H,W).  Differentiable for
    float32 maps (its own backward kernel)."""
    if normal_map.dim() != 3 or normal_map.shape[0] not in (2, 3):
        raise ValueError("Normal map must have 2 or 3 channels.")
    if normal_map.requires_grad and torch.is_grad_enabled():
        if not normal_map.is_cuda or normal_map.dtype != torch.float32:
            raise NotImplementedError("gradients through decode_normal need a float32 map on a ROCm device")
        return _DecodeNormalFn.apply(normal_map)
    return _decode_normal_raw(_device_tensor(normal_map, "decode_normal"))[0]
