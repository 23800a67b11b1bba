"""Normal -> height (csrc/height_ops.hip around torch.fft.rfft2 / irfft2) on one SIZE^2 fp32 normal map: the whole forward and the
forward + backward against upstream's op sequence restated in ATen on the same device (functions.py:180-323, fft2 / ifft2 and its
autograd backward), then every stage and both transforms on their own with their algorithmic bytes.  HIP events around each call,
3 warm-ups, the median of 20.  Prints one JSON object per line.    python tools/height_probe.py [SIZE=4096]"""
import json
import math
import os
import sys

import torch
import torch.nn.functional as TF

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
WARMUP, REPS = 3, 20


def aten_height(n, scale=1.0):
    """upstream's statements (OpenGL), on whatever device n is on."""
    nz = n[2] + 1e-8
    gx, gy = -n[0] / nz * scale, -n[1] / nz * scale
    gx, gy = gx[None, None], gy[None, None]
    gxp, gyp = TF.pad(gx, (0, 1, 0, 0), mode="replicate"), TF.pad(gy, (0, 0, 0, 1), mode="replicate")
    div = ((gxp[:, :, :, 1:] - gxp[:, :, :, :-1]) + (gyp[:, :, 1:, :] - gyp[:, :, :-1, :]))[0, 0]
    H, W = div.shape
    y = torch.arange(0, H, dtype=torch.float32, device=n.device).view(-1, 1)
    x = torch.arange(0, W, dtype=torch.float32, device=n.device).view(1, -1)
    denom = (2 * torch.cos(2 * math.pi * x / W) - 2) + (2 * torch.cos(2 * math.pi * y / H) - 2)
    denom[0, 0] = 1.0
    f = torch.fft.fft2(div) / denom
    f[0, 0] = 0
    h = torch.fft.ifft2(f).real
    h = h - h.mean()
    mn, mx = h.min(), h.max()
    return ((h - mn) / (mx - mn + 1e-8)).unsqueeze(0)


def median_us(fn):
    for _ in range(WARMUP):
        fn()
    torch.cuda.synchronize()
    times = []
    for _ in range(REPS):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        times.append(a.elapsed_time(b) * 1e3)
    return sorted(times)[len(times) // 2]


def main():
    from pypbr_amd import _height_ops as HO, functional as F
    S = int(sys.argv[1]) if len(sys.argv) > 1 else 4096
    px = S * S
    g = torch.Generator().manual_seed(1)
    z = 0.3 + 0.7 * torch.rand(1, S, S, generator=g)
    phi = 2.0 * math.pi * torch.rand(1, S, S, generator=g)
    n = torch.cat([torch.sqrt(1 - z * z) * torch.cos(phi), torch.sqrt(1 - z * z) * torch.sin(phi), z]).cuda()
    G = torch.randn(1, S, S, generator=g).cuda()

    def report(what, us, nbytes=None):
        rec = {"what": what, "size": S, "median_us": round(us, 1)}
        if nbytes is not None:
            rec.update(bytes_per_px=nbytes, tb_per_s=round(nbytes * px / us / 1e6, 3))
        print(json.dumps(rec), flush=True)

    ours, aten = F.height_from_normal(n, 1.0), aten_height(n)
    print(json.dumps({"what": "max |hip - aten fp32|", "size": S, "value": float((ours - aten).abs().max())}), flush=True)
    report("forward, hip stages + rfft2/irfft2", median_us(lambda: F.height_from_normal(n, 1.0)))
    report("forward, aten chain", median_us(lambda: aten_height(n)))

    def both(fn):
        m = n.detach().requires_grad_()
        (fn(m) * G).sum().backward()
    report("forward + backward, hip stages + rfft2/irfft2", median_us(lambda: both(lambda m: F.height_from_normal(m, 1.0))))
    report("forward + backward, aten chain + autograd", median_us(lambda: both(aten_height)))

    n4 = n[None]
    div = HO._divergence_raw(n4, 1.0, False)
    spec = torch.fft.rfft2(div).contiguous()
    h = torch.fft.irfft2(spec, s=(S, S)).contiguous()
    out, stats = HO._normalize_raw(h, torch.float32)
    G4 = G[None].contiguous()
    report("stage 1 normal_divergence", median_us(lambda: HO._divergence_raw(n4, 1.0, False)), 16)
    report("rfft2", median_us(lambda: torch.fft.rfft2(div)))
    report("stage 2 poisson_scale", median_us(lambda: HO._poisson_scale_raw(spec, S)), 8)
    report("irfft2", median_us(lambda: torch.fft.irfft2(spec, s=(S, S))))
    from pypbr_amd import _native as N
    from pypbr_amd._dispatch import launch
    lib, ws = N.lib(), HO._workspace(1, S, S, h.device)
    report("stage 3 height_stats", median_us(lambda: launch(h.device, lib.pbr_height_stats, h.data_ptr(), h.stride(0), ws.data_ptr(), 1, S, S)), 4)
    report("stage 4 height_normalize", median_us(lambda: launch(h.device, lib.pbr_height_normalize, h.data_ptr(), h.stride(0), ws.data_ptr(), out.data_ptr(),
                                                                out.stride(0), stats.data_ptr(), 1, S, S, N.F32)), 8)
    report("stage 5 height_normalize_backward (sums + dh)", median_us(lambda: HO._normalize_backward_raw(G4, out, stats)), 16)
    report("stage 7 normal_divergence_backward", median_us(lambda: HO._divergence_backward_raw(n4, h, 1.0, False)), 28)


if __name__ == "__main__":
    main()
