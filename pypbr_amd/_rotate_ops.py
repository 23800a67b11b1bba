"""Rotation (pypbr/materials/base.py:539-603, utils/functions.py:69-108): csrc/rotation.hip.

Upstream pads a map, rotates it with torchvision's nearest-neighbour rotate(expand=True), centre-crops it and rotates the normal vectors.
The chain is one closed-form index function per output pixel: rotate_plan computes its constants on the host,
rotate_maps runs it over all planes of a block in one launch, the normal triple's transform included.  (pypbr_amd/rotation.py is the
material-level API on top of this.)"""
import collections
import ctypes
import math
from typing import Optional

import torch

from . import _native as N
from ._caches import ValueMemo
from ._dispatch import _DTYPES, LAUNCHES, _needs_grad, _rows_dense, launch, ptr
from ._upload import _staged

LAUNCHES.update({"rotate_planes": 0, "rotate_planes_backward": 0})


PADDING_MODES = ("constant", "circular")
RotatePlan = collections.namedtuple("RotatePlan", "h w H W pad Hp Wp oh ow top left circular x0 y0 t00 t10 t01 t11 cos_r sin_r normal_matrix")
_ROTATE_PLANS = ValueMemo()


def _make_rotate_plan(h: int, w: int, angle: float, expand: bool, padding_mode: str) -> RotatePlan:
    a = math.radians(angle)
    H, W = h, w
    if expand:                                            # base.py:570-580, its quirk included: 180 degrees of 64 x 64 expand to 65 x 65
        W = math.ceil(abs(w * math.cos(a)) + abs(h * math.sin(a)))
        H = math.ceil(abs(w * math.sin(a)) + abs(h * math.cos(a)))
    pad = math.ceil(math.sqrt(H ** 2 + W ** 2)) - H       # base.py:583-584: the height decides both axes
    circular = padding_mode == "circular"
    if circular and (pad > h or pad > w):
        raise ValueError("circular padding of %d pixels does not fit a %dx%d map (upstream's F.pad refuses to wrap more than once)" % (pad, h, w))
    if pad < 0 or H < 1 or W < 1:
        raise ValueError("rotating a %dx%d map by %r degrees%s leaves a %dx%d target with padding %d" % (h, w, angle, " (expand)" if expand else "", H, W, pad))
    Hp, Wp = h + 2 * pad, w + 2 * pad
    r = math.radians(-angle)                              # torchvision's rotate: the inverse matrix of -angle about centre 0
    theta = torch.tensor([math.cos(r), math.sin(r), 0.0, -math.sin(r), math.cos(r), 0.0], dtype=torch.float32).view(2, 3)
    # torchvision's _compute_affine_output_size in its fp32 tensor arithmetic (torch's own rounding: CPU tensors)
    pts = torch.tensor([[-0.5 * Wp, -0.5 * Hp, 1.0], [-0.5 * Wp, 0.5 * Hp, 1.0], [0.5 * Wp, 0.5 * Hp, 1.0], [0.5 * Wp, -0.5 * Hp, 1.0]])
    corners = torch.matmul(pts, theta.T)
    half = torch.tensor((Wp * 0.5, Hp * 0.5))
    lo, hi = corners.min(dim=0)[0] + half, corners.max(dim=0)[0] + half
    tol = 1e-4
    size = torch.ceil((hi / tol).trunc_() * tol) - torch.floor((lo / tol).trunc_() * tol)
    ow, oh = int(size[0]), int(size[1])
    top, left = int(round((oh - H) / 2.0)), int(round((ow - W) / 2.0))      # torchvision's center_crop: Python's round, halves to even
    rt = theta.transpose(0, 1) / torch.tensor([0.5 * Wp, 0.5 * Hp], dtype=torch.float32)
    c, s_ = math.cos(a), math.sin(a)                       # rotate_normals, functions.py:81-88: R(angle)
    return RotatePlan(h, w, H, W, pad, Hp, Wp, oh, ow, top, left, circular, left - ow * 0.5 + 0.5, top - oh * 0.5 + 0.5,
                      float(rt[0, 0]), float(rt[1, 0]), float(rt[0, 1]), float(rt[1, 1]), float(theta[0, 0]), float(theta[0, 1]),
                      (c, -s_, s_, c))


def rotate_plan(h: int, w: int, angle: float, expand: bool = False, padding_mode: str = "constant") -> RotatePlan:
    """The host-side constants of MaterialBase.rotate (base.py:539-603) on an h x w map: the target size (H, W), the padding, the padded
    size, torchvision's expanded size (oh, ow), the centre crop's (top, left), the fp32 matrix entries of the index function and the 2x2
    matrix of rotate_normals.  Pure host arithmetic, kept per (h, w, angle, expand, padding_mode); ValueError for a padding mode other
    than "constant" / "circular" and for a circular padding that would wrap more than once -- before any device work."""
    if padding_mode not in PADDING_MODES:
        raise ValueError("Invalid padding mode %r. Must be 'constant' or 'circular'." % (padding_mode,))
    h, w, angle, expand = int(h), int(w), float(angle), bool(expand)
    if h < 1 or w < 1:
        raise ValueError("rotate needs a non-empty map, got %dx%d" % (h, w))
    return _ROTATE_PLANS.get((h, w, angle, expand, padding_mode), lambda: _make_rotate_plan(h, w, angle, expand, padding_mode))


def rotate_indices(plan: RotatePlan) -> torch.Tensor:
    """The index function of a plan written out on the host, as csrc/rotation.hip evaluates it (fp32, every step rounded on its own):
    an (H, W) int64 tensor of source offsets sy * w + sx, -1 where the pixel is filled with 0.  The model the kernel is tested against."""
    f32 = torch.float32
    x = torch.arange(plan.W, dtype=f32)[None, :] + torch.tensor(plan.x0, dtype=f32)
    y = torch.arange(plan.H, dtype=f32)[:, None] + torch.tensor(plan.y0, dtype=f32)
    t = [torch.tensor(v, dtype=f32) for v in (plan.t00, plan.t10, plan.t01, plan.t11)]
    gx, gy = x * t[0] + y * t[1], x * t[2] + y * t[3]      # tensor ops: each product and each sum is rounded
    ix = torch.round(((gx + 1) * plan.Wp - 1) / 2).long()  # torch.round: halves to even
    iy = torch.round(((gy + 1) * plan.Hp - 1) / 2).long()
    inside = (ix >= 0) & (ix < plan.Wp) & (iy >= 0) & (iy < plan.Hp)
    sx, sy = ix - plan.pad, iy - plan.pad
    if plan.circular:
        sx, sy = sx % plan.w, sy % plan.h
    else:
        inside &= (sx >= 0) & (sx < plan.w) & (sy >= 0) & (sy < plan.h)
    return torch.where(inside, sy * plan.w + sx, torch.full_like(sx, -1))


def _rotate_geom(plan: RotatePlan) -> N.RotateGeom:
    return N.RotateGeom(plan.pad, int(plan.circular), plan.x0, plan.y0, plan.t00, plan.t10, plan.t01, plan.t11, plan.cos_r, plan.sin_r)


def _rotate_raw(t: torch.Tensor, plan: RotatePlan, nfp: int, out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """t [B,P,h,w] (rows dense) -> [B,P,H,W] (a new tensor, or `out`: rows dense, not overlapping t)."""
    B, P, h, w = t.shape
    if out is None:
        out = torch.empty((B, P, plan.H, plan.W), dtype=t.dtype, device=t.device)
    geom = _rotate_geom(plan)
    launch(t.device, N.lib().pbr_rotate_planes, t.data_ptr(), t.stride(0), t.stride(1), out.data_ptr(), out.stride(0), out.stride(1), B, P, h, w,
           plan.H, plan.W, ctypes.byref(geom), nfp, *plan.normal_matrix, _DTYPES[t.dtype])
    LAUNCHES["rotate_planes"] += 1
    return out


class _RotateFn(torch.autograd.Function):
    """rotate_maps with its backward kernel (a gather over the source texels through the forward's own index function: no atomics)."""

    @staticmethod
    def forward(ctx, t, plan, nfp):
        x = _rows_dense(t.detach())
        ctx.save_for_backward(*((x,) if nfp >= 0 else ()))        # the normal triple's adjoint needs the texel's own normal
        ctx.geom = (tuple(x.shape), x.dtype, plan, nfp)
        return _rotate_raw(x, plan, nfp)

    @staticmethod
    def backward(ctx, grad_out):
        (B, P, h, w), dtype, plan, nfp = ctx.geom
        g = _rows_dense(grad_out.to(torch.float32))
        gi = torch.empty((B, P, h, w), dtype=torch.float32, device=g.device)
        src = ctx.saved_tensors[0] if nfp >= 0 else None
        geom = _rotate_geom(plan)
        launch(g.device, N.lib().pbr_rotate_planes_backward, g.data_ptr(), g.stride(0), g.stride(1), gi.data_ptr(), gi.stride(0), gi.stride(1),
               ptr(src), 0 if src is None else src.stride(0), 0 if src is None else src.stride(1), B, P, h, w, plan.H, plan.W, ctypes.byref(geom), nfp,
               *plan.normal_matrix)
        LAUNCHES["rotate_planes_backward"] += 1
        return gi, None, None


def rotate_maps(block: torch.Tensor, angle: float, expand: bool = False, padding_mode: str = "constant",
                normal_first_plane: Optional[int] = None) -> torch.Tensor:
    """MaterialBase.rotate (base.py:539-603) over every plane of `block` (P,h,w) | (B,P,h,w) in ONE launch: nearest-neighbour rotation by
    `angle` degrees (counter-clockwise, as torchvision's), `expand` as upstream computes the target size, `padding_mode` "constant"
    (zeros) | "circular".  Values are copied bit for bit; when `normal_first_plane` is given, planes normal_first_plane .. + 2 are a
    normal map and their vectors are rotated as utils.rotate_normals does (renormalised).  float32 / float16, P <= 32.  Differentiable
    for float32 (its own backward kernel: a deterministic gather); CPU tensors are staged through the device."""
    if not isinstance(block, torch.Tensor) or block.dim() not in (3, 4):
        raise ValueError("rotate_maps needs (P,h,w) or (B,P,h,w), got %s" % (tuple(block.shape) if isinstance(block, torch.Tensor) else type(block),))
    if block.dtype not in _DTYPES:
        raise TypeError("rotate_maps supports float32/float16, got %s" % block.dtype)
    P, h, w = block.shape[-3:]
    plan = rotate_plan(h, w, angle, expand, padding_mode)
    if P < 1 or P > 32:
        raise ValueError("rotate_maps takes 1 to 32 planes in one block, got %d" % P)
    nfp = -1 if normal_first_plane is None else int(normal_first_plane)
    if nfp != -1 and not 0 <= nfp <= P - 3:
        raise ValueError("normal_first_plane = %d leaves no three planes among %d" % (nfp, P))
    grad = _needs_grad(block)
    if grad and block.dtype != torch.float32:
        raise NotImplementedError("gradients through rotate_maps need a float32 block")
    b4 = block if block.dim() == 4 else block[None]
    if grad:
        res = _staged(b4, lambda x: _RotateFn.apply(x, plan, nfp))
    else:
        res = _staged(b4, lambda x: _rotate_raw(_rows_dense(x), plan, nfp))
    return res if block.dim() == 4 else res[0]
