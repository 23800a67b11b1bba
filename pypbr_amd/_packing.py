"""Packed material tensors (pypbr/materials/base.py:319-487: as_tensor / from_tensor; :279-291 normal_rgb): csrc/packing.hip.

A packed tensor is [C_total, H, W]: the maps of a material stacked along the channels.  Unpacking and packing are tables of plane
operations (include/pbr_hip.h: pbr_plane_op) -- AFFINE, one plane times a scale plus a bias, and NORMAL_XY, the z of a two-channel
normal map -- and a table of up to 32 operations is ONE launch, forward and backward."""
import torch

from . import _native as N
from ._dispatch import _DTYPES, LAUNCHES, _needs_grad, _rows_dense, launch
from ._upload import to_host

LAUNCHES.update({"plane_ops": 0, "plane_ops_backward": 0})


def _plane_ops_call(ops, batch: int, pixels: int, dtype: torch.dtype, device, backward: bool = False):
    """One call into pbr_plane_ops / pbr_plane_ops_backward: at most 32 operations."""
    table = (N.PlaneOp * len(ops))(*ops)
    fn = N.lib().pbr_plane_ops_backward if backward else N.lib().pbr_plane_ops
    launch(device, fn, table, len(ops), batch, pixels, _DTYPES[dtype])
    LAUNCHES["plane_ops_backward" if backward else "plane_ops"] += 1


def _run_plane_ops(ops, batch, pixels, dtype, device, backward=False):
    for i in range(0, len(ops), N.MAX_PLANE_OPS):
        _plane_ops_call(ops[i:i + N.MAX_PLANE_OPS], batch, pixels, dtype, device, backward)


def _plane_ptr(t: torch.Tensor, plane: int) -> int:
    """Address of plane `plane` of t [B,C,H,W]."""
    return t.data_ptr() + plane * t.stride(1) * t.element_size()


def _planes_of(block: torch.Tensor, first: int, count: int, squeeze: bool) -> torch.Tensor:
    """Planes [first, first + count) of the dense block [B,P,H,W] as a tensor of its own over the SAME memory -- not an autograd view of the
    block (the maps of a material are edited and replaced one by one) -- (count,H,W) when `squeeze`."""
    B, P, H, W = block.shape
    out = torch.empty(0, dtype=block.dtype, device=block.device)
    if squeeze:
        return out.set_(block.untyped_storage(), block.storage_offset() + first * H * W, (count, H, W), (H * W, W, 1))
    return out.set_(block.untyped_storage(), block.storage_offset() + first * H * W, (B, count, H, W), (P * H * W, H * W, W, 1))


def _unpack_layout(layout, channels: int):
    """[(name, channels), ...] -> [(name, first source channel, channels, planes written)]; a 2-channel map called "normal" gets its z."""
    plan, c = [], 0
    for item in layout:
        name, n = item
        n = int(n)
        if n < 1:
            raise ValueError("a map of a packed tensor has at least one channel, got %r" % (item,))
        plan.append((name, c, n, 3 if name == "normal" and n == 2 else n))
        c += n
    if c != channels:
        raise ValueError(f"Packed tensor has {channels} channels, but configuration expects {c} channels.")
    return plan


def _unpack_raw(x: torch.Tensor, plan, scale: float, bias: float, squeeze: bool):
    """x [B,C,H,W] on the device (rows dense) -> the maps of `plan`, back to back in ONE allocation."""
    B, _, H, W = x.shape
    block = torch.empty((B, sum(p[3] for p in plan), H, W), dtype=x.dtype, device=x.device)
    ops, first = [], 0
    for _, c, n, written in plan:
        if written != n:
            ops.append(N.PlaneOp(N.PLANE_NORMAL_XY, 0, _plane_ptr(x, c), x.stride(0), x.stride(1), _plane_ptr(block, first), block.stride(0),
                                 block.stride(1), None, 0, 0, scale, bias))
        else:
            ops.extend(N.PlaneOp(N.PLANE_AFFINE, 0, _plane_ptr(x, c + k), x.stride(0), 0, _plane_ptr(block, first + k), block.stride(0), 0,
                                 None, 0, 0, scale, bias) for k in range(n))
        first += written
    _run_plane_ops(ops, B, H * W, x.dtype, x.device)
    maps, first = [], 0
    for _, _, _, written in plan:
        maps.append(_planes_of(block, first, written, squeeze))
        first += written
    return maps


class _UnpackFn(torch.autograd.Function):
    """unpack_planes with its backward kernel: one launch writes the whole gradient of the packed tensor."""

    @staticmethod
    def forward(ctx, tensor, plan, scale, bias, squeeze):
        x = _rows_dense(tensor.detach())
        ctx.save_for_backward(x)
        ctx.args = (plan, scale, bias, squeeze)
        ctx.set_materialize_grads(False)
        return tuple(_unpack_raw(x, plan, scale, bias, squeeze))

    @staticmethod
    def backward(ctx, *grads):
        (x,) = ctx.saved_tensors
        plan, scale, bias, squeeze = ctx.args
        B, C, H, W = x.shape
        gi = torch.empty((B, C, H, W), dtype=torch.float32, device=x.device)
        ops, keep = [], []
        for (_, c, n, written), g in zip(plan, grads):
            if g is not None:
                g = _rows_dense(g.to(torch.float32))
                g = g[None] if squeeze else g
                keep.append(g)
            ptr = (lambda k: None) if g is None else (lambda k, g=g: _plane_ptr(g, k))
            gbs, gps = (0, 0) if g is None else (g.stride(0), g.stride(1))
            if written != n:
                ops.append(N.PlaneOp(N.PLANE_NORMAL_XY, 0, ptr(0), gbs, gps, _plane_ptr(gi, c), gi.stride(0), gi.stride(1),
                                     _plane_ptr(x, c), x.stride(0), x.stride(1), scale, bias))
            else:
                ops.extend(N.PlaneOp(N.PLANE_AFFINE, 0, ptr(k), gbs, 0, _plane_ptr(gi, c + k), gi.stride(0), 0, None, 0, 0, scale, bias)
                           for k in range(n))
        _run_plane_ops(ops, B, H * W, torch.float32, x.device, backward=True)
        return gi, None, None, None, None


def _on_device(tensors, fn):
    """fn over device tensors; CPU tensors travel there and the results back (differentiably when a gradient is wanted)."""
    if all(t.is_cuda for t in tensors):
        return fn(tensors)
    N.require_device()
    home = tensors[0].device
    res = fn([t.to("cuda") for t in tensors])
    back = (lambda r: r.to(home)) if _needs_grad(*tensors) else (lambda r: to_host(r, home))
    return [back(r) for r in res] if isinstance(res, (list, tuple)) else back(res)


def unpack_planes(tensor: torch.Tensor, layout, is_normalized: bool = False):
    """The maps of a packed tensor (MaterialBase.from_tensor, base.py:476-485): `layout` = [(name, channels), ...] in channel order; every
    map is its channels, times 0.5 plus 0.5 when `is_normalized`, and a 2-channel map called "normal" gets its z and is normalised
    (base.py:223-242, after the optional x 0.5 + 0.5) -- ONE launch for up to 32 operations (a plane, or a 2-channel normal map, each).
    [C,H,W] | [B,C,H,W], float32 / float16 (arithmetic in float32).  Returns the maps in the layout's order: new tensors, never views
    of `tensor`, back to back in one allocation.  A channel-sliced view is read in place; strided rows cost one dense copy.
    Differentiable for float32 (one backward launch); CPU tensors are staged through the device."""
    if not isinstance(tensor, torch.Tensor) or tensor.dim() not in (3, 4):
        raise ValueError("a packed tensor is [C,H,W] or [B,C,H,W], got %s" % (tuple(tensor.shape) if isinstance(tensor, torch.Tensor) else type(tensor),))
    if tensor.dtype not in _DTYPES:
        raise TypeError("unpack_planes supports float32/float16, got %s" % tensor.dtype)
    plan = _unpack_layout(layout, tensor.shape[-3])
    if tensor.shape[-1] < 1 or tensor.shape[-2] < 1 or (tensor.dim() == 4 and tensor.shape[0] < 1):
        raise ValueError("unpack_planes needs non-empty planes, got %s" % (tuple(tensor.shape),))
    scale, bias = (0.5, 0.5) if is_normalized else (1.0, 0.0)
    squeeze = tensor.dim() == 3
    grad = _needs_grad(tensor)
    if grad and tensor.dtype != torch.float32:
        raise NotImplementedError("gradients through unpack_planes need a float32 tensor")
    t4 = tensor[None] if squeeze else tensor
    if grad:
        return list(_on_device([t4], lambda ts: list(_UnpackFn.apply(ts[0], plan, scale, bias, squeeze))))
    return list(_on_device([t4], lambda ts: _unpack_raw(_rows_dense(ts[0].detach()), plan, scale, bias, squeeze)))


def _affine_plan(maps, limits, coeffs):
    """Checks the maps of a pack and returns (B, H, W, squeeze, [(channels, channels taken, scale, bias)])."""
    if not maps:
        raise ValueError("No valid texture maps found to stack.")
    first = maps[0]
    if first.dim() not in (3, 4):
        raise ValueError("maps are [C,H,W] or [B,C,H,W], got %s" % (tuple(first.shape),))
    for t in maps:
        if t.dim() != first.dim() or t.shape[-2:] != first.shape[-2:] or (t.dim() == 4 and t.shape[0] != first.shape[0]):
            raise ValueError("All texture maps must have the same spatial dimensions for concatenation.")
        if t.dtype != first.dtype or t.dtype not in _DTYPES:
            raise TypeError("the maps of a pack share one dtype, float32 or float16; got %s" % ([str(m.dtype) for m in maps],))
        if t.device != first.device:
            raise ValueError("the maps of a pack live on one device, got %s" % ([str(m.device) for m in maps],))
    if first.numel() == 0:
        raise ValueError("pack_planes needs non-empty planes, got %s" % (tuple(first.shape),))
    rows = []
    for t, limit, (scale, bias) in zip(maps, limits, coeffs):
        c = t.shape[-3]
        take = c if limit is None else int(limit)
        if take < 1 or take > c:
            raise ValueError("cannot take %s of %d channels" % (limit, c))
        rows.append((c, take, float(scale), float(bias)))
    return (1 if first.dim() == 3 else first.shape[0]), first.shape[-2], first.shape[-1], first.dim() == 3, rows


def _pack_raw(xs, rows, squeeze):
    """xs: [B,C_i,H,W] device tensors (rows dense) -> [B, sum(taken), H, W]."""
    B, _, H, W = xs[0].shape
    out = torch.empty((B, sum(r[1] for r in rows), H, W), dtype=xs[0].dtype, device=xs[0].device)
    ops, p = [], 0
    for x, (_, take, scale, bias) in zip(xs, rows):
        ops.extend(N.PlaneOp(N.PLANE_AFFINE, 0, _plane_ptr(x, k), x.stride(0), 0, _plane_ptr(out, p + k), out.stride(0), 0, None, 0, 0, scale, bias)
                   for k in range(take))
        p += take
    _run_plane_ops(ops, B, H * W, out.dtype, out.device)
    return out[0] if squeeze else out


class _PackFn(torch.autograd.Function):
    """pack_planes with its backward kernel: the gradients of all maps are one allocation written by one launch -- g x scale for the
    channels taken, 0 for the channels a limit cut."""

    @staticmethod
    def forward(ctx, rows, squeeze, *maps):
        xs = [_rows_dense(t.detach()) for t in maps]
        ctx.args = (rows, squeeze)
        return _pack_raw(xs, rows, squeeze)

    @staticmethod
    def backward(ctx, grad_out):
        rows, squeeze = ctx.args
        g = _rows_dense(grad_out.to(torch.float32))
        g = g[None] if squeeze else g
        B, _, H, W = g.shape
        wanted = ctx.needs_input_grad[2:]
        gi = torch.empty((B, sum(r[0] for r, w in zip(rows, wanted) if w), H, W), dtype=torch.float32, device=g.device)
        ops, grads, p, q = [], [], 0, 0
        for (c, take, scale, _), w in zip(rows, wanted):
            if w:
                ops.extend(N.PlaneOp(N.PLANE_AFFINE, 0, _plane_ptr(g, p + k) if k < take else None, g.stride(0), 0, _plane_ptr(gi, q + k),
                                     gi.stride(0), 0, None, 0, 0, scale, 0.0) for k in range(c))
                grads.append(_planes_of(gi, q, c, False))       # the maps arrive as [B,C,H,W] (_pack)
                q += c
            else:
                grads.append(None)
            p += take
        if ops:
            _run_plane_ops(ops, B, H * W, torch.float32, g.device, backward=True)
        return (None, None) + tuple(grads)


def _pack(maps, limits, coeffs):
    B, H, W, squeeze, rows = _affine_plan(maps, limits, coeffs)
    grad = _needs_grad(*maps)
    if grad and maps[0].dtype != torch.float32:
        raise NotImplementedError("gradients through pack_planes need float32 maps")
    m4 = [t[None] if squeeze else t for t in maps]
    if grad:
        return _on_device(m4, lambda ts: _PackFn.apply(rows, squeeze, *ts))
    return _on_device(m4, lambda ts: _pack_raw([_rows_dense(t.detach()) for t in ts], rows, squeeze))


def pack_planes(maps, limits=None, normalize_flags=None) -> torch.Tensor:
    """The maps stacked along the channels in ONE launch (MaterialBase.as_tensor, base.py:379-414): of map i its first `limits[i]` channels
    (None: all), as (t - 0.5) / 0.5 = 2 t - 1 where `normalize_flags[i]`.  [C_i,H,W] | [B,C_i,H,W] maps of one size, dtype (float32 /
    float16) and device.  Differentiable for float32 (one backward launch over all maps: channels a limit cut receive 0); CPU tensors
    are staged through the device."""
    maps = list(maps)
    limits = [None] * len(maps) if limits is None else list(limits)
    flags = [False] * len(maps) if normalize_flags is None else list(normalize_flags)
    if len(limits) != len(maps) or len(flags) != len(maps):
        raise ValueError("pack_planes needs one limit and one flag per map")
    return _pack(maps, limits, [(2.0, -1.0) if f else (1.0, 0.0) for f in flags])
