"""Normal -> height by Poisson reconstruction (pypbr/utils/functions.py:180-323, materials/base.py:731-751): csrc/height_ops.hip around
torch.fft.rfft2 / irfft2.  The two transforms are the FFT library's; the divergence, the division by the Laplacian's eigenvalues, the
mean / min / max reductions, the normalisation and every backward stage are the library's kernels."""
import torch

from . import _native as N
from ._dispatch import _DTYPES, _needs_grad, _rows_dense, launch
from ._normal_ops import _directx
from ._upload import _staged


def _divergence_raw(n: torch.Tensor, scale: float, directx: bool) -> torch.Tensor:
    """n [B,3,H,W] (rows dense, float32 / float16) -> upstream's div_g [B,H,W], float32."""
    B, _, H, W = n.shape
    div = torch.empty((B, H, W), dtype=torch.float32, device=n.device)
    launch(n.device, N.lib().pbr_normal_divergence, n.data_ptr(), n.stride(0), n.stride(1), div.data_ptr(), div.stride(0), B, H, W, float(scale),
           int(directx), _DTYPES[n.dtype])
    return div


def _poisson_scale_raw(spectrum: torch.Tensor, width: int) -> torch.Tensor:
    """The half spectrum [B,H,W/2+1] (complex64, contiguous) over the Laplacian's eigenvalues, in place; `width` is the real width."""
    B, H, Wh = spectrum.shape
    parts = torch.view_as_real(spectrum)
    launch(spectrum.device, N.lib().pbr_poisson_scale, parts.data_ptr(), H * Wh, B, H, int(width))
    return spectrum


def _poisson_solve(d: torch.Tensor) -> torch.Tensor:
    """functions.py:286-323 on [B,H,W] float32: irfft2(rfft2(d) / den) -- the spectrum of a real image is Hermitian and den is real and
    even, so this is upstream's ifft2(fft2(d) / den).real at half the bytes.  Its own adjoint, for the same reason."""
    H, W = d.shape[-2:]
    spectrum = _poisson_scale_raw(torch.fft.rfft2(d).contiguous(), W)
    return torch.fft.irfft2(spectrum, s=(H, W)).contiguous()          # s: an odd width is not what the half spectrum implies


def _workspace(B: int, H: int, W: int, device) -> torch.Tensor:
    nbytes = N.lib().pbr_height_workspace_bytes(B, H, W)
    if nbytes == 0:
        raise ValueError("a height map of %d x %d is beyond the reductions' 2^31 pixels" % (H, W))
    return torch.empty((nbytes // 8,), dtype=torch.float64, device=device)     # (8-byte aligned)


def _normalize_raw(h: torch.Tensor, dtype: torch.dtype):
    """h [B,H,W] float32 (contiguous) -> (out [B,1,H,W] in `dtype`, stats [B,5] float32: mean, min, range, argmin, argmax)."""
    B, H, W = h.shape
    ws = _workspace(B, H, W, h.device)
    out = torch.empty((B, 1, H, W), dtype=dtype, device=h.device)
    stats = torch.empty((B, 5), dtype=torch.float32, device=h.device)
    lib = N.lib()
    launch(h.device, lib.pbr_height_stats, h.data_ptr(), h.stride(0), ws.data_ptr(), B, H, W)
    launch(h.device, lib.pbr_height_normalize, h.data_ptr(), h.stride(0), ws.data_ptr(), out.data_ptr(), out.stride(0), stats.data_ptr(), B, H, W,
           _DTYPES[dtype])
    return out, stats


def _normalize_backward_raw(grad_out: torch.Tensor, out: torch.Tensor, stats: torch.Tensor) -> torch.Tensor:
    """G, out [B,1,H,W] float32 (contiguous), stats of the forward -> dh [B,H,W]."""
    B, _, H, W = out.shape
    ws = _workspace(B, H, W, out.device)
    dh = torch.empty((B, H, W), dtype=torch.float32, device=out.device)
    launch(out.device, N.lib().pbr_height_normalize_backward, grad_out.data_ptr(), grad_out.stride(0), out.data_ptr(), out.stride(0),
           stats.data_ptr(), ws.data_ptr(), dh.data_ptr(), dh.stride(0), B, H, W)
    return dh


def _divergence_backward_raw(n: torch.Tensor, dd: torch.Tensor, scale: float, directx: bool) -> torch.Tensor:
    """n [B,3,H,W] float32 (rows dense), dd [B,H,W] -> the gradient of the normals."""
    B, _, H, W = n.shape
    gn = torch.empty((B, 3, H, W), dtype=torch.float32, device=n.device)
    launch(n.device, N.lib().pbr_normal_divergence_backward, n.data_ptr(), n.stride(0), n.stride(1), dd.data_ptr(), dd.stride(0), gn.data_ptr(),
           gn.stride(0), gn.stride(1), B, H, W, float(scale), int(directx))
    return gn


def _hfn_raw(n: torch.Tensor, scale: float, directx: bool):
    """n [B,3,H,W] -> (height [B,1,H,W] in n's dtype, stats)."""
    n = _rows_dense(n)
    return _normalize_raw(_poisson_solve(_divergence_raw(n, scale, directx)), n.dtype)


class _HeightFromNormalFn(torch.autograd.Function):
    """compute_height_from_normal with its backward stages: the normalisation's adjoint, the solve again, the divergence's adjoint."""

    @staticmethod
    def forward(ctx, normal, scale, directx):
        n = _rows_dense(normal.detach())
        out, stats = _hfn_raw(n, scale, directx)
        ctx.save_for_backward(n, out, stats)
        ctx.args = (float(scale), bool(directx))
        return out

    @staticmethod
    @torch.autograd.function.once_differentiable        # raw kernels: a second derivative raises instead of being silently wrong
    def backward(ctx, grad_out):
        n, out, stats = ctx.saved_tensors
        scale, directx = ctx.args
        g = grad_out.to(torch.float32).contiguous()
        dd = _poisson_solve(_normalize_backward_raw(g, out, stats))
        return _divergence_backward_raw(n, dd, scale, directx), None, None


def height_from_normal(normal: torch.Tensor, scale: float = 1.0, convention="opengl") -> torch.Tensor:
    """utils.compute_height_from_normal (functions.py:180-247) on the device: (3,H,W) -> (1,H,W), (B,3,H,W) -> (B,1,H,W), each image of a
    batch solved and normalised to [0, 1] on its own.  float32 / float16 storage (float32 for the transforms and everything between);
    differentiable for float32; CPU tensors are staged through the device.  Two stated differences from upstream: the
    Laplacian's eigenvalues are evaluated without upstream's low-frequency cancellation (the result tracks the float64 evaluation), and
    the gradient of min / max goes to the first of several equal extrema."""
    if normal is None:
        raise ValueError("Normal map is required to compute height.")
    if normal.dim() not in (3, 4) or normal.shape[-3] != 3:
        raise ValueError("Normal map must have three channels.")
    directx = _directx(convention)
    if normal.dtype not in _DTYPES:
        raise TypeError("height_from_normal supports float32/float16, got %s" % normal.dtype)
    grad = _needs_grad(normal)
    if grad and normal.dtype != torch.float32:
        raise NotImplementedError("gradients through height_from_normal need a float32 normal map")
    n4 = normal if normal.dim() == 4 else normal[None]
    if grad:
        out = _staged(n4, lambda t: _HeightFromNormalFn.apply(t, scale, directx))
    else:
        out = _staged(n4, lambda t: _hfn_raw(t, scale, directx)[0])
    return out if normal.dim() == 4 else out[0]
