"""Geometric transforms (pypbr/materials/base.py:506-537, :605-655): csrc/geometry.hip.

crop, tile, the flips and roll are index maps, and so is every chain of them: per axis src(i) = (o + s i) mod N for i in [0, L), s = +-1
(DESIGN.md 3.9).  PlaneMap folds a chain on the host; remap_planes runs one map over all planes of a block in one launch."""
from typing import Tuple

import torch

from . import _native as N
from ._dispatch import _DTYPES, LAUNCHES, _needs_grad, _rows_dense, launch
from ._upload import _staged

LAUNCHES.update({"remap_planes": 0, "remap_planes_backward": 0})       # what the Compose tests count, never reset here


class PlaneMap:
    """The pending index map of one (H, W) map size: per axis [N, L, o, s] (source extent, output extent, offset, step) and the signs a
    flip leaves on the x / y plane of a normal map (base.py:605-639).  Pure host arithmetic.  `flip`, `crop`, `roll` and `tile` fold a
    stage into the map and return True, or return False and leave the map alone when the stage does not fold (a roll or a tile behind a
    crop to a non-multiple): the caller then materialises this map and starts a new one on its output size."""

    def __init__(self, h: int, w: int):
        self.y, self.x = [int(h), int(h), 0, 1], [int(w), int(w), 0, 1]
        self.neg = [False, False]                       # normal plane 0 (x), plane 1 (y)

    @property
    def size(self) -> Tuple[int, int]:
        return self.y[1], self.x[1]

    @property
    def source_size(self) -> Tuple[int, int]:
        return self.y[0], self.x[0]

    @property
    def ymap(self) -> Tuple[int, int]:
        return self.y[2], self.y[3]

    @property
    def xmap(self) -> Tuple[int, int]:
        return self.x[2], self.x[3]

    @property
    def identity(self) -> bool:
        return all(a[0] == a[1] and a[2] == 0 and a[3] == 1 for a in (self.y, self.x)) and not any(self.neg)

    def flip(self, horizontal: bool) -> bool:
        a = self.x if horizontal else self.y
        n, length, o, s = a
        a[2], a[3] = (o + s * (length - 1)) % n, -s
        self.neg[0 if horizontal else 1] ^= True
        return True

    def crop(self, top: int, left: int, height: int, width: int) -> bool:
        check_crop(self.size, top, left, height, width)
        for a, t, l in ((self.y, int(top), int(height)), (self.x, int(left), int(width))):
            a[2], a[1] = (a[2] + a[3] * t) % a[0], l
        return True

    def roll(self, dy: int, dx: int) -> bool:
        moves = [(a, int(d)) for a, d in ((self.y, dy), (self.x, dx)) if int(d) % a[1] != 0]
        if any(a[1] % a[0] != 0 for a, _ in moves):
            return False
        for a, d in moves:
            a[2] = (a[2] - a[3] * d) % a[0]
        return True

    def tile(self, ny: int, nx: int) -> bool:
        reps = [(a, int(n)) for a, n in ((self.y, ny), (self.x, nx)) if int(n) != 1]
        if any(n < 1 for _, n in reps):
            raise ValueError("tile counts must be >= 1, got %s" % ((ny, nx),))
        if any(a[1] % a[0] != 0 for a, _ in reps):
            return False
        for a, n in reps:
            a[1] *= n
        return True

    def indices(self):
        """(source row of every output row, source column of every output column): the map written out."""
        return tuple([(a[2] + a[3] * i) % a[0] for i in range(a[1])] for a in (self.y, self.x))


def check_crop(size, top, left, height, width):
    """In-bounds crops only (upstream pads the rest with zeros through torchvision: INTEGRATION.md); ValueError before any device work."""
    h, w = size
    top, left, height, width = int(top), int(left), int(height), int(width)
    if top < 0 or left < 0 or height < 1 or width < 1 or top + height > h or left + width > w:
        raise ValueError("crop (top=%d, left=%d, height=%d, width=%d) does not lie inside the %dx%d map; out-of-bounds crops are not supported"
                         % (top, left, height, width, h, w))


def fold_stages(h: int, w: int, stages) -> list:
    """Folds geometric stages -- ("flip_h",), ("flip_v",), ("crop", top, left, height, width), ("roll", dy, dx), ("tile", ny, nx) -- over
    an (h, w) map into as few PlaneMaps as the folding rules allow: the maps to run one after the other.  Identity maps are dropped, so
    the list is empty when the stages move nothing."""
    maps, cur = [], PlaneMap(h, w)
    for st in stages:
        kind, args = st[0], st[1:]
        if kind == "flip_h" or kind == "flip_v":
            cur.flip(kind == "flip_h")
            continue
        if kind not in ("crop", "roll", "tile"):
            raise ValueError("unknown geometric stage %r" % (kind,))
        if not getattr(cur, kind)(*args):
            maps.append(cur)
            cur = PlaneMap(*cur.size)
            if not getattr(cur, kind)(*args):   # pragma: no cover  (a fresh map has L == N: everything folds)
                raise AssertionError("stage %r does not fold into a fresh map" % (st,))
    maps.append(cur)
    return [m for m in maps if not m.identity]


def _axis_map(m, n, what):
    o, s = int(m[0]), int(m[1])
    if s not in (1, -1) or not 0 <= o < n:
        raise ValueError("%s = (offset, step) needs 0 <= offset < %d and step +1 | -1, got %s" % (what, n, (m[0], m[1])))
    return o, s


def _remap_raw(t: torch.Tensor, ymap, xmap, mask: int, ho: int, wo: int) -> torch.Tensor:
    """t [B,P,H,W] (rows dense) -> [B,P,ho,wo]."""
    B, P, H, W = t.shape
    out = torch.empty((B, P, ho, wo), dtype=t.dtype, device=t.device)
    launch(t.device, N.lib().pbr_remap_planes, t.data_ptr(), t.stride(0), t.stride(1), out.data_ptr(), out.stride(0), out.stride(1), B, P, H, W, ho, wo,
           ymap[0], ymap[1], xmap[0], xmap[1], mask, _DTYPES[t.dtype])
    LAUNCHES["remap_planes"] += 1
    return out


class _RemapFn(torch.autograd.Function):
    """remap_planes with its backward kernel (a gather over the source texels: no atomics)."""

    @staticmethod
    def forward(ctx, t, ymap, xmap, mask, ho, wo):
        x = _rows_dense(t.detach())
        ctx.geom = (tuple(x.shape), x.dtype, ymap, xmap, mask)
        return _remap_raw(x, ymap, xmap, mask, ho, wo)

    @staticmethod
    def backward(ctx, grad_out):
        (B, P, H, W), dtype, ymap, xmap, mask = ctx.geom
        g = _rows_dense(grad_out.to(torch.float32))
        ho, wo = g.shape[-2:]
        gi = torch.empty((B, P, H, W), dtype=torch.float32, device=g.device)
        launch(g.device, N.lib().pbr_remap_planes_backward, g.data_ptr(), g.stride(0), g.stride(1), gi.data_ptr(), gi.stride(0), gi.stride(1), B, P, H, W,
               ho, wo, ymap[0], ymap[1], xmap[0], xmap[1], mask)
        LAUNCHES["remap_planes_backward"] += 1
        return gi.to(dtype), None, None, None, None, None


def remap_planes(t: torch.Tensor, ymap, xmap, negate=(), out_size=None) -> torch.Tensor:
    """One index map over every plane of `t` [..., P, H, W] in one launch: out[..., p, i, j] = +-t[..., p, (oy + sy i) mod H, (ox + sx j) mod W]
    with ymap = (oy, sy), xmap = (ox, sx), steps +1 | -1, and `out_size` = (h_out, w_out) (default: the source's size; smaller is a crop,
    larger a tile).  `negate`: the planes (indices into P) whose values change sign -- a flip's x or y plane of a normal map.  float32 /
    float16, values copied bit for bit; P <= 32.  Differentiable (its own backward kernel, sums formed in float32); CPU tensors are
    staged through the device."""
    if not isinstance(t, torch.Tensor) or t.dim() < 3:
        raise ValueError("remap_planes needs [..., P, H, W], got %s" % (tuple(t.shape) if isinstance(t, torch.Tensor) else type(t),))
    if t.dtype not in _DTYPES:
        raise TypeError("remap_planes supports float32/float16, got %s" % t.dtype)
    P, H, W = t.shape[-3:]
    if H < 1 or W < 1 or P < 1:
        raise ValueError("remap_planes needs non-empty planes, got %s" % (tuple(t.shape),))
    if P > 32:
        raise ValueError("remap_planes takes at most 32 planes in one block (one sign bit each), got %d" % P)
    ym, xm = _axis_map(ymap, H, "ymap"), _axis_map(xmap, W, "xmap")
    ho, wo = (H, W) if out_size is None else (int(out_size[0]), int(out_size[1]))
    if ho < 1 or wo < 1:
        raise ValueError("out_size must be positive, got %s" % (out_size,))
    mask = 0
    for p in negate:
        if not 0 <= int(p) < P:
            raise ValueError("negate names plane %d of %d" % (int(p), P))
        mask |= 1 << int(p)
    t4 = t[None] if t.dim() == 3 else (t if t.dim() == 4 else t.reshape((-1,) + tuple(t.shape[-3:])))
    if _needs_grad(t):
        res = _staged(t4, lambda x: _RemapFn.apply(x, ym, xm, mask, ho, wo))
    else:
        res = _staged(t4, lambda x: _remap_raw(_rows_dense(x), ym, xm, mask, ho, wo))
    return res.reshape(tuple(t.shape[:-2]) + (ho, wo))
