"""What the Python side of every kernel family shares: the dtype codes of the C ABI (include/pbr_hip.h, bound in _native.py), the checks
on tensors that go to a kernel, the launch counters, and `launch` -- the ONE place where a C entry point is called under its tensors'
device with torch's current stream.  Nothing here knows a family; _upload, the family modules and functional import from it, never the
other way round."""
import torch

from . import _native as N

_DTYPES = {torch.float32: N.F32, torch.float16: N.F16}

# Launches since import, by entry point: what the Compose / packing / rotation tests count, never reset here.  ONE dict, mutated in place
# (pypbr_amd.functional.LAUNCHES is this object); the family modules add their keys when they are imported.
LAUNCHES = {}


def _stream_ptr(device: torch.device) -> int:
    return torch.cuda.current_stream(device).cuda_stream


def launch(device: torch.device, fn, *args) -> None:
    """fn(*args, stream) with `device` current and torch's current stream of it (looked up inside the device guard) -- the C entry points
    take the stream, a raw hipStream_t, last -- and the status through N.check.  RenderPlan's methods, which accept an explicit stream,
    keep their own form (functional.py)."""
    with torch.cuda.device(device):
        N.check(fn(*args, _stream_ptr(device)))


def ptr(t):
    """The address a C entry point gets for an optional tensor: NULL for None."""
    return None if t is None else t.data_ptr()


def _needs_grad(*tensors) -> bool:
    return torch.is_grad_enabled() and any(isinstance(t, torch.Tensor) and t.requires_grad for t in tensors)


def _device_tensor(t: torch.Tensor, what: str) -> torch.Tensor:
    if not t.is_cuda:
        raise RuntimeError("%s needs a tensor on a ROCm device; there is no CPU path" % what)
    if t.dtype not in _DTYPES:
        raise TypeError("%s supports float32/float16, got %s" % (what, t.dtype))
    return t.contiguous()


def _grad_like(g: torch.Tensor, like: torch.Tensor) -> torch.Tensor:
    """The upstream gradient in the maps' storage type, contiguous (the backward kernels read it as the maps are stored)."""
    return g.to(like.dtype).contiguous()


def rows_are_dense(t: torch.Tensor) -> bool:
    """The kernels take any batch / plane strides but dense rows of non-negative strides: this is that rule, for every caller."""
    return t.stride(-1) == 1 and (t.shape[-2] == 1 or t.stride(-2) == t.shape[-1]) and all(s >= 0 for s in t.stride())


def _rows_dense(t: torch.Tensor) -> torch.Tensor:
    """`t` as the kernels take it: itself when its rows are dense, else a contiguous copy."""
    return t if rows_are_dense(t) else t.contiguous()


def plane_geometry(t: torch.Tensor):
    """(batch, channels, height, width, batch stride, plane stride) of a [C,H,W] / [B,C,H,W] view with dense rows, strides in elements as
    they are (0 for the batch stride of a [C,H,W] view): what the entries of a launch table carry."""
    four = t.dim() == 4
    return (t.shape[0] if four else 1), t.shape[-3], t.shape[-2], t.shape[-1], (t.stride(0) if four else 0), t.stride(-3)
