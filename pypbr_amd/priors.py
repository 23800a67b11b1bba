"""Map smoothness priors of a fit: vectorial total variation (Charbonnier) or Tikhonov (L2) over the maps of a material, value and
gradients of ALL maps from ONE launch (csrc/smoothness.hip, pbr_smoothness_step; an extension: upstream has no prior).

    prior = MaterialSmoothness({"albedo": 0.1, "normal": 0.05, "roughness": 0.3, "metallic": 0.3})
    loss = data_loss(material, photographs) + prior(material, weights=1 - confidence); loss.backward(); opt.step()

include/pbr_hip.h has the definition, tools/smoothness_oracle.py states it in float64 numpy: forward differences (0 across the border, or
wrapped), the channels of a map coupled under one square root, `k sum w phi(s)` with k = lambda / (B H W) ("mean") or lambda ("sum").
The gradients are written, not accumulated: autograd adds them to `.grad` like any other op's.  There is no CPU path: `smoothness` needs
its maps on a ROCm device (the private `_composition`, the same definition in ATen, runs anywhere and is what the calls that the kernel
does not serve take: weights that require grad, maps whose rows are not dense).
"""
import torch
import torch.nn.functional as TF

from . import _native as N
from ._dispatch import _DTYPES, launch, plane_geometry, ptr, rows_are_dense
from .materials import FIT_MAPS as MAP_NAMES                # the names `lambdas` may carry: what MaterialBase._fit_maps looks for

# Launches since import (what the tests count; never reset here).
LAUNCHES = {"smoothness_step": 0}

KINDS = {"l2": N.SMOOTH_L2, "charbonnier": N.SMOOTH_CHARBONNIER}
REDUCTIONS = ("mean", "sum")


def _scale(lam, t, reduction):
    """k of the definition, in float64."""
    if reduction == "sum":
        return float(lam)
    return float(lam) / float((t.shape[0] if t.dim() == 4 else 1) * t.shape[-2] * t.shape[-1])


def _weight_fits(w, t):
    """[1,H,W] or [B,1,H,W] (or [1,1,H,W]) beside a [C,H,W] / [B,C,H,W] map."""
    hw = tuple(t.shape[-2:])
    if w.dim() == 3:
        return tuple(w.shape) == (1,) + hw
    if w.dim() == 4:
        return tuple(w.shape[1:]) == (1,) + hw and w.shape[0] in (1, t.shape[0] if t.dim() == 4 else 1)
    return False


def _check_arguments(tensors, lambdas, kind, eps, wrap, weights, reduction):
    """The ValueErrors of the surface, before any device work; returns (tensors, lambdas, weights) as lists of one length."""
    tensors, lambdas = list(tensors), [float(x) for x in lambdas]
    if len(lambdas) != len(tensors):
        raise ValueError("one lambda per tensor: %d tensors, %d lambdas" % (len(tensors), len(lambdas)))
    if kind not in KINDS:
        raise ValueError("kind is one of %s, got %r" % (sorted(KINDS), kind))
    if reduction not in REDUCTIONS:
        raise ValueError("reduction is 'mean' or 'sum', got %r" % (reduction,))
    if not float(eps) > 0.0:
        raise ValueError("eps must be > 0, got %r" % (eps,))
    for lam in lambdas:
        if not lam >= 0.0:
            raise ValueError("a lambda must be >= 0, got %r" % (lam,))
    for t in tensors:
        if not isinstance(t, torch.Tensor) or t.dim() not in (3, 4) or not 1 <= t.shape[-3] <= 4 or t.numel() == 0:
            raise ValueError("smoothness takes [C,H,W] / [B,C,H,W] tensors of 1 to 4 channels, got %s"
                             % (tuple(t.shape) if isinstance(t, torch.Tensor) else type(t),))
    if weights is None:
        each = [None] * len(tensors)
    elif isinstance(weights, torch.Tensor):                 # one plane for every entry of its size
        each = [weights if _weight_fits(weights, t) else None for t in tensors]
        if tensors and all(w is None for w in each):
            raise ValueError("weights of shape %s fit none of the tensors ([1,H,W] / [B,1,H,W])" % (tuple(weights.shape),))
    else:
        each = list(weights)
        if len(each) != len(tensors):
            raise ValueError("a sequence of weights is aligned with the tensors: %d tensors, %d weights" % (len(tensors), len(each)))
        for w, t in zip(each, tensors):
            if w is not None and not (isinstance(w, torch.Tensor) and _weight_fits(w, t)):
                raise ValueError("weights of shape %s do not fit a tensor of shape %s ([1,H,W] / [B,1,H,W])"
                                 % (tuple(w.shape) if isinstance(w, torch.Tensor) else type(w), tuple(t.shape)))
    return tensors, lambdas, each


def _forward_difference(x, dim, wrap):
    if wrap:
        return torch.roll(x, -1, dim) - x
    d = x.narrow(dim, 1, x.shape[dim] - 1) - x.narrow(dim, 0, x.shape[dim] - 1)
    return TF.pad(d, (0, 1) if dim == -1 else (0, 0, 0, 1))


def _composition(tensors, lambdas, kind="charbonnier", eps=1e-3, wrap=False, weights=None, reduction="mean"):
    """The definition in ATen, differentiable in the maps and the weights, on any device and dtype: (loss, terms) with the loss a 0-dim
    tensor and terms [n].  The arithmetic runs in the maps' dtype (float16 maps: in float32)."""
    tensors, lambdas, each = _check_arguments(tensors, lambdas, kind, eps, wrap, weights, reduction)
    terms = []
    for t, lam, w in zip(tensors, lambdas, each):
        x = t if t.dim() == 4 else t.unsqueeze(0)
        if x.dtype == torch.float16:
            x = x.float()
        dx, dy = _forward_difference(x, -1, wrap), _forward_difference(x, -2, wrap)
        s = (dx * dx + dy * dy).sum(dim=1, keepdim=True)
        phi = s if kind == "l2" else s / (torch.sqrt(s + eps * eps) + eps)
        if w is not None:
            phi = phi * w.to(device=x.device, dtype=x.dtype).reshape((-1, 1) + tuple(x.shape[-2:]))
        terms.append(phi.sum() * _scale(lam, t, reduction))
    if not terms:
        zero = torch.zeros((), dtype=torch.float32)
        return zero, torch.zeros(0, dtype=torch.float32)
    terms = torch.stack(terms)
    return terms.sum(), terms


def _entry(t, grad, w, k, kind, eps, wrap):
    """pbr_smooth_tensor of one map (dense rows), its gradient buffer (dense rows, of the map's shape, or None) and its float32 contiguous
    weights (or None)."""
    batch, channels, height, width, batch_stride, plane_stride = plane_geometry(t)
    grad_strides = plane_geometry(grad)[4:] if grad is not None else (0, 0)
    plane = height * width
    return N.SmoothTensor(t.data_ptr(), ptr(grad), ptr(w), batch_stride, plane_stride, *grad_strides,
                          plane if (w is not None and w.numel() > plane) else 0,
                          k, float(eps), _DTYPES[t.dtype], batch, channels, height, width, kind, int(bool(wrap)))


def _step(tensors, grads, weights, ks, kind, eps, wrap):
    """pbr_smoothness_step over the entries, N.MAX_SMOOTH_TENSORS per launch, on the current stream without synchronising: (loss, terms),
    float32 on the maps' device, the values of several launches added there.  `grads[i]` (None: value only) is written in the map's dtype;
    `weights[i]` is float32, contiguous, [1,H,W] / [B,1,H,W], or None; `ks[i]` the float64 scale."""
    device = tensors[0].device
    if any(t.device != device for t in tensors):
        raise RuntimeError("smoothness: the tensors of one call live on one device")
    lib = N.lib()
    terms = torch.empty(len(tensors), dtype=torch.float32, device=device)
    loss = None
    for first in range(0, len(tensors), N.MAX_SMOOTH_TENSORS):
        chunk = range(first, min(len(tensors), first + N.MAX_SMOOTH_TENSORS))
        table = (N.SmoothTensor * len(chunk))(*[_entry(tensors[i], grads[i], weights[i], ks[i], kind, eps, wrap) for i in chunk])
        nbytes = lib.pbr_smoothness_workspace_bytes(table, len(chunk))
        if nbytes == 0:                                      # a table the library refuses: raise what it says
            N.check(lib.pbr_smoothness_check(table, len(chunk)))
        ws = torch.empty((nbytes + 3) // 4, dtype=torch.float32, device=device)
        part = torch.empty((), dtype=torch.float32, device=device)
        launch(device, lib.pbr_smoothness_step, table, len(chunk), part.data_ptr(), terms[first:].data_ptr(), ws.data_ptr(), nbytes)
        LAUNCHES["smoothness_step"] += 1
        loss = part if loss is None else loss + part
    return loss, terms


def _run(tensors, weights, ks, kind, eps, wrap, wanted):
    """One evaluation: the gradients of the wanted maps in ONE allocation per dtype (each block on a 32-byte boundary: the quad path),
    in the maps' own shapes.  Returns (loss, terms, grads, blocks) -- blocks: the allocations, what backward scales."""
    device = tensors[0].device
    count = {}
    for t, want in zip(tensors, wanted):
        if want:
            count[t.dtype] = count.get(t.dtype, 0) + (t.numel() + 15) // 16 * 16
    blocks = {dt: torch.empty(n, dtype=dt, device=device) for dt, n in count.items()}
    at = dict.fromkeys(blocks, 0)
    grads = []
    for t, want in zip(tensors, wanted):
        if not want:
            grads.append(None)
            continue
        grads.append(blocks[t.dtype][at[t.dtype]:at[t.dtype] + t.numel()].view(t.shape))
        at[t.dtype] += (t.numel() + 15) // 16 * 16
    loss, terms = _step(tensors, grads, weights, ks, kind, eps, wrap)
    return loss, terms, grads, list(blocks.values())


class _SmoothnessFn(torch.autograd.Function):
    """(loss, terms) with the maps' gradients from the forward launch (functional._MseStepFn's bridge): forward keeps them, backward
    hands them over scaled by the upstream gradient of the loss on the device -- one pbr_scale_by_device_scalar per dtype, which returns
    at once when the scalar is exactly 1; no host synchronisation.  `terms` carries no gradient."""

    @staticmethod
    def forward(ctx, spec, *tensors):
        weights, ks, kind, eps, wrap = spec
        wanted = [bool(need) for need in ctx.needs_input_grad[1:]]
        loss, terms, grads, blocks = _run(tensors, weights, ks, kind, eps, wrap, wanted)
        ctx.spec, ctx.wanted, ctx.kept = spec, wanted, (grads, blocks)
        ctx.save_for_backward(*tensors)
        ctx.mark_non_differentiable(terms)
        return loss, terms

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, grad_loss, _grad_terms=None):
        tensors = ctx.saved_tensors                          # in-place edits of the maps since forward are detected, as for any op
        kept, ctx.kept = ctx.kept, None
        if kept is None:                                     # differentiated again: the first call gave the buffers away
            weights, ks, kind, eps, wrap = ctx.spec
            kept = _run(tensors, weights, ks, kind, eps, wrap, ctx.wanted)[2:]
        grads, blocks = kept
        if blocks:
            k = grad_loss.detach().to(blocks[0].device, torch.float32).reshape(1).contiguous()
            for block in blocks:
                launch(block.device, N.lib().pbr_scale_by_device_scalar, block.data_ptr(), block.numel(), _DTYPES[block.dtype], k.data_ptr())
        return (None, *grads)


def smoothness(tensors, lambdas, *, kind="charbonnier", eps=1e-3, wrap=False, weights=None, reduction="mean", return_terms=False):
    """The smoothness prior of several maps, `sum_i k_i sum_{b,y,x} w_i phi(s_i)`, as a 0-dim float32 tensor on the maps' device; with
    `return_terms` also the per-tensor values, [len(tensors)] (0 where lambda is 0: such an entry is dropped from the launch).

    `tensors`: [C,H,W] / [B,C,H,W] float32 or float16 device tensors, 1 to 4 channels, of any sizes.  `lambdas`: one float per tensor.
    `kind`: "charbonnier" (phi = sqrt(s + eps^2) - eps: total variation, smooth at 0) or "l2" (phi = s).  `wrap`: differences across the
    border wrap around (tileable textures) instead of being 0.  `weights`: None; ONE tensor [1,H,W] / [B,1,H,W], used for every entry of
    that size; or a sequence aligned with `tensors` whose items may be None.  bool / uint8 masks become float32 at the call.  A weight
    multiplies, it does not skip.  `reduction`: "mean" divides by B H W, "sum" does not.

    All entries go into one launch (N.MAX_SMOOTH_TENSORS per launch; more take several, their values added on the device), which also
    leaves the gradients of the maps that require grad; without any, only the value is computed.  Weights that require grad and maps
    whose rows are not dense take the ATen composition of the same definition."""
    tensors, lambdas, each = _check_arguments(tensors, lambdas, kind, eps, wrap, weights, reduction)
    for t in tensors:
        if not t.is_cuda:
            raise RuntimeError("smoothness needs tensors on a ROCm device; there is no CPU path")
        if t.dtype not in _DTYPES:
            raise TypeError("smoothness supports float32/float16 maps, got %s" % t.dtype)
    if not tensors:
        raise ValueError("smoothness needs at least one tensor")
    live = [i for i, lam in enumerate(lambdas) if lam != 0.0]
    device = tensors[0].device
    if not live:
        zero = torch.zeros((), dtype=torch.float32, device=device)
        return (zero, torch.zeros(len(tensors), dtype=torch.float32, device=device)) if return_terms else zero
    grad_on = torch.is_grad_enabled()
    if any(not rows_are_dense(tensors[i]) for i in live) or (grad_on and any(each[i] is not None and each[i].requires_grad for i in live)):
        loss, some = _composition([tensors[i] for i in live], [lambdas[i] for i in live], kind, eps, wrap, [each[i] for i in live], reduction)
        loss, some = loss.float(), some.float()
    else:
        ws = [None if each[i] is None else each[i].detach().to(device, torch.float32).contiguous() for i in live]
        spec = (ws, [_scale(lambdas[i], tensors[i], reduction) for i in live], KINDS[kind], float(eps), bool(wrap))
        loss, some = _SmoothnessFn.apply(spec, *[tensors[i] for i in live])
    if not return_terms:
        return loss
    if len(live) == len(tensors):
        return loss, some
    terms = torch.zeros(len(tensors), dtype=torch.float32, device=device)
    terms[torch.tensor(live, device=device)] = some.detach()
    return loss, terms


class MaterialSmoothness(torch.nn.Module):
    """MaterialSmoothness(lambdas={"albedo": ..., "normal": ..., "roughness": ..., "metallic": ..., "specular": ..., "height": ...},
    kind="charbonnier", eps=1e-3, wrap=False, reduction="mean"): `smoothness` over the stored maps of a material, as
    optim.material_param_groups finds them, in one launch.  Names absent from `lambdas`, or that the material does not store, are skipped.
    `forward(material, weights=None)`: `weights` as in `smoothness` -- one plane, e.g. `1 - confidence` of capture.photometric_stereo, serves
    every map of its size.  The maps must be materialised: a pending lazy blend, a lazy tile or undecoded maps raise ValueError."""

    def __init__(self, lambdas, kind="charbonnier", eps=1e-3, wrap=False, reduction="mean"):
        super().__init__()
        unknown = sorted(set(lambdas) - set(MAP_NAMES))
        if unknown:
            raise ValueError("MaterialSmoothness knows the maps %s, got %s" % (list(MAP_NAMES), unknown))
        _check_arguments([], [], kind, eps, wrap, None, reduction)
        if any(not float(v) >= 0.0 for v in lambdas.values()):
            raise ValueError("a lambda must be >= 0, got %r" % (dict(lambdas),))
        self.lambdas = {k: float(v) for k, v in lambdas.items()}
        self.kind, self.eps, self.wrap, self.reduction = kind, float(eps), bool(wrap), reduction

    def forward(self, material, weights=None):
        if not material._is_materialised():
            raise ValueError("MaterialSmoothness needs materialised maps: call materialize_blend() / materialize_tile(), or read the maps "
                             "once, before fitting a material with a pending lazy blend, a lazy tile or undecoded maps")
        maps = {k: t for k, t in material._fit_maps().items() if k in self.lambdas}
        if not maps:
            raise ValueError("the material stores none of the maps %s" % sorted(self.lambdas))
        return smoothness(list(maps.values()), [self.lambdas[k] for k in maps], kind=self.kind, eps=self.eps, wrap=self.wrap,
                          weights=weights, reduction=self.reduction)

    def extra_repr(self):
        return "lambdas=%r, kind=%r, eps=%g, wrap=%r, reduction=%r" % (self.lambdas, self.kind, self.eps, self.wrap, self.reduction)
