"""Normal-map operations (pypbr/utils/functions.py:69-177, materials/base.py:673-729): csrc/normal_ops.hip."""
from typing import Optional

import torch

from . import _native as N
from ._dispatch import _DTYPES, _needs_grad, _rows_dense, launch
from ._upload import _staged


def _directx(convention) -> bool:
    """NormalConvention.OPENGL / DIRECTX (or their values "opengl" / "directx") -> the kernel's flag; anything else is upstream's
    ValueError (functions.py:164-171)."""
    value = getattr(convention, "value", convention)
    if value == "opengl":
        return False
    if value == "directx":
        return True
    raise ValueError("Unsupported normal convention.")


def _nfh_raw(h: torch.Tensor, scale: float, directx: bool) -> torch.Tensor:
    """h [B,1,H,W] (rows dense) -> normals [B,3,H,W]."""
    h = _rows_dense(h)
    B, _, H, W = h.shape
    out = torch.empty((B, 3, H, W), dtype=h.dtype, device=h.device)
    launch(h.device, N.lib().pbr_normal_from_height, h.data_ptr(), h.stride(0), out.data_ptr(), out.stride(0), out.stride(1), B, H, W,
           float(scale), int(directx), _DTYPES[h.dtype])
    return out


class _NormalFromHeightFn(torch.autograd.Function):
    """compute_normal_from_height with its backward kernel (the transposed stencil of F.normalize's adjoint)."""

    @staticmethod
    def forward(ctx, height, scale, directx):
        h = _rows_dense(height.detach())
        ctx.save_for_backward(h)
        ctx.args = (float(scale), bool(directx))
        return _nfh_raw(h, scale, directx)

    @staticmethod
    def backward(ctx, grad_out):
        (h,) = ctx.saved_tensors
        scale, directx = ctx.args
        g = _rows_dense(grad_out.to(torch.float32))
        B, _, H, W = h.shape
        gh = torch.empty((B, 1, H, W), dtype=torch.float32, device=h.device)
        launch(h.device, N.lib().pbr_normal_from_height_backward, h.data_ptr(), h.stride(0), g.data_ptr(), g.stride(0), g.stride(1), gh.data_ptr(),
               gh.stride(0), B, H, W, scale, int(directx))
        return gh, None, None


def normal_from_height(height: torch.Tensor, scale: float = 1.0, convention="opengl") -> torch.Tensor:
    """utils.compute_normal_from_height (functions.py:123-177) on the device: (H,W) | (1,H,W) -> (3,H,W), (B,1,H,W) -> (B,3,H,W);
    zero padding at every image's border.  float32 / float16 storage; differentiable for float32 (its own backward kernel); CPU
    tensors are staged through the device.  A height with more than one channel is refused (upstream would return 3C channels)."""
    if height is None:
        raise ValueError("Height map is required to compute normals.")
    directx = _directx(convention)
    if height.dim() == 2:
        h4 = height[None, None]
    elif height.dim() == 3:
        if height.shape[0] != 1:
            raise ValueError("Height map must have 1 channel, got %d" % height.shape[0])
        h4 = height[None]
    elif height.dim() == 4:
        if height.shape[1] != 1:
            raise ValueError("Height map must have 1 channel, got %d" % height.shape[1])
        h4 = height
    else:
        raise ValueError("Height map must be (H,W), (1,H,W) or (B,1,H,W), got %s" % (tuple(height.shape),))
    if height.dtype not in _DTYPES:
        raise TypeError("normal_from_height supports float32/float16, got %s" % height.dtype)
    grad = _needs_grad(height)
    if grad and height.dtype != torch.float32:
        raise NotImplementedError("gradients through normal_from_height need a float32 height map")
    if grad:
        out = _staged(h4, lambda t: _NormalFromHeightFn.apply(t, scale, directx))
    else:
        out = _staged(h4, lambda t: _nfh_raw(t, scale, directx))
    return out if height.dim() == 4 else out[0]


def _matrix(matrix):
    m = [[float(v) for v in row] for row in (matrix.tolist() if isinstance(matrix, torch.Tensor) else matrix)]
    if len(m) != 2 or any(len(row) != 2 for row in m):
        raise ValueError("the transform is a 2x2 matrix")
    return m[0][0], m[0][1], m[1][0], m[1][1]


def _transform_raw(n: torch.Tensor, m, renormalize: bool, out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """n [B,3,H,W] (rows dense) -> out (a new tensor, or `out`, which may be n itself)."""
    B, _, H, W = n.shape
    if out is None:
        out = torch.empty((B, 3, H, W), dtype=n.dtype, device=n.device)
    launch(n.device, N.lib().pbr_normal_transform, n.data_ptr(), n.stride(0), n.stride(1), out.data_ptr(), out.stride(0), out.stride(1), B, H * W,
           *m, int(renormalize), _DTYPES[n.dtype])
    return out


class _TransformNormalsFn(torch.autograd.Function):
    """rotate_normals / adjust_normal_strength / invert_normal with their backward kernel."""

    @staticmethod
    def forward(ctx, normal, m, renormalize):
        n = _rows_dense(normal.detach())
        ctx.save_for_backward(n)
        ctx.args = (m, bool(renormalize))
        return _transform_raw(n, m, renormalize)

    @staticmethod
    def backward(ctx, grad_out):
        (n,) = ctx.saved_tensors
        m, renormalize = ctx.args
        g = _rows_dense(grad_out.to(torch.float32))
        B, _, H, W = n.shape
        gi = torch.empty((B, 3, H, W), dtype=torch.float32, device=n.device)
        launch(n.device, N.lib().pbr_normal_transform_backward, n.data_ptr(), n.stride(0), n.stride(1), g.data_ptr(), g.stride(0), g.stride(1),
               gi.data_ptr(), gi.stride(0), gi.stride(1), B, H * W, *m, int(renormalize))
        return gi, None, None


def transform_normals(normal: torch.Tensor, matrix, renormalize: bool, out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """(x, y) <- matrix (x, y) per pixel, z kept, then F.normalize when `renormalize` -- the one transform behind rotate_normals
    (functions.py:69-108: a rotation, renormalised), adjust_normal_strength (base.py:689-706: f I, renormalised) and invert_normal
    (functions.py:111-120: diag(1, -1), not renormalised).  (3,H,W) | (B,3,H,W), float32 / float16 storage; differentiable for
    float32.  `out` (a device tensor of the same shape and dtype, `normal` itself allowed) receives the result without autograd."""
    if normal.dim() not in (3, 4) or normal.shape[-3] != 3:
        raise ValueError("Normal map must have 3 channels, got shape %s" % (tuple(normal.shape),))
    if normal.dtype not in _DTYPES:
        raise TypeError("transform_normals supports float32/float16, got %s" % normal.dtype)
    m = _matrix(matrix)
    n4 = normal if normal.dim() == 4 else normal[None]
    grad = _needs_grad(normal)
    if grad and normal.dtype != torch.float32:
        raise NotImplementedError("gradients through transform_normals need a float32 normal map")
    if out is not None:
        if grad:
            raise NotImplementedError("out= takes no gradient")
        if not (out.is_cuda and normal.is_cuda and out.shape == normal.shape and out.dtype == normal.dtype):
            raise ValueError("out= must be a device tensor of the normal map's shape and dtype")
        o4 = out if out.dim() == 4 else out[None]
        if _rows_dense(o4) is not o4 or _rows_dense(n4) is not n4:
            raise ValueError("out= needs dense rows")
        _transform_raw(n4, m, renormalize, out=o4)
        torch.autograd.graph.increment_version(out)    # the kernel wrote through a raw pointer: autograd and the caches must see an edit
        return out
    if grad:
        res = _staged(n4, lambda t: _TransformNormalsFn.apply(t, m, renormalize))
    else:
        res = _staged(n4, lambda t: _transform_raw(_rows_dense(t), m, renormalize))
    return res if normal.dim() == 4 else res[0]
