#!/usr/bin/env python3
"""Photometric-stereo initialisation (csrc/photometric.hip) at the sizes of a real capture: 4096^2 and 1024^2 grids under L = 2, 8 and 16
point lights, per-shot weights, sRGB targets of a bumpy Lambertian surface (slope amplitude 1.0, lights at heights 0.35 / 0.5: attached
shadows, so the reweighting passes run), K = 3.

  product     pbr_photometric_stereo of the library as built: the shots are READ again in every pass;
  cache16     the same source built with -DPBR_PHOTOMETRIC_CACHE=16: every shot's r_lc and weight kept in registers, one pixel per lane, the
              shot loops unrolled under l < L predicates (`--build`, on the machine that has hipcc);
  baseline    the same definition written with ATen float32 on the same device: L geometry grids, the sRGB curve, K masked normal-matrix
              sums, an adjugate solve, the albedo sums.

HIP events around the call, 3 warm-ups, the median of 20, the candidates alternating.  Bytes the kernel must move: 16 L + 28 per pixel
(12 L + 28 without weights); what the re-reading passes fetch again is not counted.  Run by hand; not a test, asserts no duration.

    python tools/photometric_probe.py --build
    python tools/photometric_probe.py [--out profiles/photometric_probe.json] [--sizes 4096,1024] [--lights 2,8,16]"""
import argparse
import ctypes
import json
import math
import os
import statistics
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
CSRC = os.path.join(ROOT, "pypbr_amd", "csrc")
VARIANTS = {"cache16": ["-DPBR_PHOTOMETRIC_CACHE=16"]}
HBM_PEAK = 8.0e12     # bytes / s, the MI355X's specification


def variant_path(name):
    return os.path.join(ROOT, "tools", "libphotometric_%s.so" % name)


def build_variants():
    flags = ["-O3", "-std=c++17", "-fPIC", "--offload-arch=gfx950", "-ffp-contract=on", "-fno-slp-vectorize", "-fno-gpu-rdc", "-Wno-unused-function"]
    jobs = [subprocess.Popen([os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")] + flags + extra + ["-shared", os.path.join(CSRC, "photometric.hip"), "-o", variant_path(name)])
            for name, extra in VARIANTS.items()]
    if any(j.wait() for j in jobs):
        sys.exit("a variant did not build")
    print("built", ", ".join(VARIANTS))


ap = argparse.ArgumentParser()
ap.add_argument("--build", action="store_true")
ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "photometric_probe.json"))
ap.add_argument("--sizes", default="4096,1024")
ap.add_argument("--lights", default="2,8,16")
ap.add_argument("--reps", type=int, default=20)
args = ap.parse_args()
if args.build:
    build_variants()
    sys.exit(0)

import torch  # noqa: E402

from pypbr_amd import _native as N  # noqa: E402

assert torch.cuda.is_available(), "the probe measures on a ROCm device"
dev = torch.device("cuda", 0)
REPS, WARM = args.reps, 3
K, TAU, KAPPA, INTENSITY = 3, 0.1, 1e-4, 0.3


def median_us(fns):
    times = [[] for _ in fns]
    for rep in range(WARM + REPS):
        for k, fn in enumerate(fns):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            fn()
            e1.record()
            e1.synchronize()
            if rep >= WARM:
                times[k].append(e0.elapsed_time(e1) * 1e3)
    return [statistics.median(t) for t in times]


def entry_point(lib):
    fn = lib.pbr_photometric_stereo
    fn.argtypes = N.lib().pbr_photometric_stereo.argtypes
    fn.restype = ctypes.c_int
    return fn


def light_rows(L):
    return [[0.7 * math.cos(2 * math.pi * ((3 * l) % max(L, 1) + 0.25) / L), 0.7 * math.sin(2 * math.pi * ((3 * l) % max(L, 1) + 0.25) / L), 0.35 if l % 2 == 0 else 0.5]
            for l in range(L)]


def geometry(lights, H, W):
    xs, ys = torch.linspace(-0.5, 0.5, W, device=dev), torch.linspace(-0.5, 0.5, H, device=dev)
    yv, xv = torch.meshgrid(ys, xs, indexing="ij")
    P = torch.stack([xv, -yv, torch.zeros_like(xv)])
    d = torch.tensor(lights, device=dev).view(-1, 3, 1, 1) - P[None]
    dist = d.norm(dim=1, keepdim=True)
    return d / (dist + 1e-7), 1.0 / (dist[:, 0] ** 2 + 1e-7), P


def scene(L, H, W):
    """sRGB targets [L,3,H,W] of a bumpy Lambertian surface and per-shot weights [L,1,H,W] (a tenth of them zero)."""
    lights = light_rows(L)
    w, att, P = geometry(lights, H, W)
    x, y = P[0], P[1]
    n = torch.stack([-torch.sin(7 * x + 1) * torch.cos(5 * y), -torch.cos(6 * y) * torch.sin(4 * x + 2), torch.ones_like(x)])
    n = n / n.norm(dim=0, keepdim=True)
    gen = torch.Generator(device=dev).manual_seed(3)
    rho = torch.rand((3, H, W), device=dev, generator=gen) * 0.75 + 0.15
    targets = torch.empty((L, 3, H, W), device=dev)
    for l in range(L):
        lin = (rho / math.pi * INTENSITY * ((w[l] * n).sum(dim=0).clamp_min(0.0) * att[l])).clamp(0.0, 1.0)
        targets[l] = torch.where(lin <= 0.0031308, lin * 12.92, 1.055 * lin.pow(1 / 2.4) - 0.055)
    weights = (torch.rand((L, 1, H, W), device=dev, generator=gen) > 0.1).float()
    return lights, targets, weights


def baseline(targets, weights, lights, out):
    """The definition with ATen, float32, K full passes (no early exit), every shot's geometry a grid of its own."""
    L, _, H, W = targets.shape
    w, att, _ = geometry(lights, H, W)                                              # [L,3,H,W], [L,H,W]
    t = targets.clamp(0.0, 1.0)
    lin = torch.where(t <= 0.04045, t / 12.92, ((t + 0.055) / 1.055).pow(2.4))
    r = lin / (INTENSITY * att[:, None])
    y = r.mean(dim=1)
    wt = weights[:, 0]
    mask = torch.ones_like(wt, dtype=torch.bool)
    valid = torch.ones((H, W), dtype=torch.bool, device=dev)
    g = torch.zeros((3, H, W), device=dev)
    conf = torch.zeros((H, W), device=dev)
    used = wt != 0
    for k in range(K):
        use = mask & (wt != 0) & valid
        u = torch.where(use, wt, torch.zeros_like(wt))
        uw = u[:, None] * w
        a00, a01, a02 = (uw[:, 0] * w[:, 0]).sum(0), (uw[:, 0] * w[:, 1]).sum(0), (uw[:, 0] * w[:, 2]).sum(0)
        a11, a12, a22 = (uw[:, 1] * w[:, 1]).sum(0), (uw[:, 1] * w[:, 2]).sum(0), (uw[:, 2] * w[:, 2]).sum(0)
        b = (uw * torch.where(use, y, torch.zeros_like(y))[:, None]).sum(0)            # [3,H,W]
        # the adjugate by hand: batched LU (torch.linalg.solve) over 16.8 M 3 x 3 systems would dominate everything else
        c00, c01, c02 = a11 * a22 - a12 * a12, a02 * a12 - a01 * a22, a01 * a12 - a02 * a11
        c11, c12, c22 = a00 * a22 - a02 * a02, a01 * a02 - a00 * a12, a00 * a11 - a01 * a01
        tr, det = a00 + a11 + a22, a00 * c00 + a01 * c01 + a02 * c02
        c = torch.where(tr > 0, det / (tr / 3) ** 3, torch.zeros_like(tr))
        ok = valid & ~(c < KAPPA)
        gk = torch.stack([c00 * b[0] + c01 * b[1] + c02 * b[2], c01 * b[0] + c11 * b[1] + c12 * b[2], c02 * b[0] + c12 * b[1] + c22 * b[2]]) / det
        norm = gk.norm(dim=0)
        ok = ok & (norm > 0) & torch.isfinite(norm) & (gk[2] > 0)
        g, conf, used = torch.where(ok, gk, g), torch.where(ok, c, conf), torch.where(ok, use, used)
        valid = valid & ok
        if k < K - 1:
            mask = torch.where(ok, (w * gk[None]).sum(dim=1) > TAU * norm, mask)
    used = torch.where(valid, used, wt != 0)
    flat = torch.tensor([0.0, 0.0, 1.0], device=dev).view(3, 1, 1)
    n = torch.where(valid, g / g.norm(dim=0).clamp_min(1e-30), flat)
    s = (w * n[None]).sum(dim=1).clamp_min(0.0)
    us = torch.where(used, wt * s, torch.zeros_like(s))
    den = (us * s).sum(dim=0)
    num = (us[:, None] * torch.where(used[:, None], r, torch.zeros_like(r))).sum(dim=0)
    out[0].copy_(n)
    out[1].copy_(torch.where(den == 0, torch.zeros_like(num), (math.pi * num / den).clamp(0.0, 1.0)))
    out[2].copy_(torch.where(valid, conf, torch.zeros_like(conf)))


libs = {"product": N.lib().pbr_photometric_stereo}
for name in VARIANTS:
    if os.path.exists(variant_path(name)):
        libs[name] = entry_point(ctypes.CDLL(variant_path(name)))
    else:
        print("variant %s is not built (tools/photometric_probe.py --build): skipped" % name)
records = []
for size in [int(v) for v in args.sizes.split(",")]:
    H = W = size
    for L in [int(v) for v in args.lights.split(",")]:
        lights, targets, weights = scene(L, H, W)
        rows = (ctypes.c_float * (3 * L))(*[v for row in lights for v in row])
        ints = (ctypes.c_float * (3 * L))(*([INTENSITY] * (3 * L)))
        bufs = {k: (torch.empty((3, H, W), device=dev), torch.empty((3, H, W), device=dev), torch.empty((H, W), device=dev)) for k in list(libs) + ["baseline"]}
        stream = torch.cuda.current_stream().cuda_stream

        def call(fn, out, with_weights=True):
            def go():
                rc = fn(targets.data_ptr(), weights.data_ptr() if with_weights else None, 0, L, H, W, rows, ints, N.LIGHT_POINT, 1.0, 1, K, TAU, KAPPA, 0,
                        out[0].data_ptr(), out[1].data_ptr(), out[2].data_ptr(), stream)
                assert rc == 0, rc
            return go
        names = list(libs)
        fns = [call(libs[k], bufs[k]) for k in names] + [lambda: baseline(targets, weights, lights, bufs["baseline"])]
        t = median_us(fns)
        ref = bufs["product"]
        agree = {}
        for k in names[1:] + ["baseline"]:
            both = (bufs[k][2] > 0) & (ref[2] > 0) & (ref[2] >= 0.05)
            agree[k] = {"validity_differs_on_share": float(((bufs[k][2] > 0) != (ref[2] > 0)).float().mean()),
                        "normal_mean_abs_diff_where_both_valid_c_ge_0.05": float((bufs[k][0] - ref[0]).abs().amax(dim=0)[both].mean()) if bool(both.any()) else 0.0,
                        "bit_equal": bool(all(torch.equal(a, b) for a, b in zip(bufs[k], ref)))}
        t_now = median_us([call(libs["product"], ref, with_weights=False)])[0]
        nbytes, nbytes_now = (16 * L + 28) * H * W, (12 * L + 28) * H * W
        rec = {"grid": size, "lights": L, "iterations": K,
               "time_us": {k: round(v, 1) for k, v in zip(names + ["baseline"], t)}, "time_us_product_without_weights": round(t_now, 1),
               "bytes_per_pixel": 16 * L + 28, "product_fraction_of_hbm_peak": round(nbytes / (t[0] * 1e-6) / HBM_PEAK, 4),
               "product_without_weights_fraction_of_hbm_peak": round(nbytes_now / (t_now * 1e-6) / HBM_PEAK, 4),
               "baseline_over_product": round(t[-1] / t[0], 2),
               "cache16_over_product": round(t[names.index("cache16")] / t[0], 4) if "cache16" in names else None,
               "against_product": agree, "valid_share": float((ref[2] > 0).float().mean())}
        records.append(rec)
        print(json.dumps(rec), flush=True)
        del bufs, targets, weights
        torch.cuda.empty_cache()

out = {"what": "photometric-stereo initialisation (csrc/photometric.hip): the library's kernel (shots read again in every pass), the same source "
               "keeping the shots in registers (cache16), and the same definition written with ATen float32; point lights, per-shot weights, sRGB "
               "targets, K = 3 (tools/photometric_probe.py)",
       "timing": "HIP events around the call, %d warm-ups, median of %d, the candidates alternating in one process" % (WARM, REPS),
       "hbm_peak_bytes_per_s": HBM_PEAK, "device": torch.cuda.get_device_name(0), "stamp": N.build_stamp(), "records": records}
os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
with open(args.out, "w") as f:
    json.dump(out, f, indent=1)
print("wrote", args.out)
