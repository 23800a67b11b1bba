#!/usr/bin/env python3
"""Photograph rectification (csrc/rectify.hip) on the shapes of a real capture: L = 8 photographs of 3000 x 4000 x 3 onto a 4096^2 and a
1024^2 grid at supersample 1, 2 and 4, each shot under its own mildly rotated, mildly tilted homography, so no output row is axis-aligned.

  product     pbr_rectify_images of the library as built;
  variants    the same source built with another tile shape (-DPBR_RECTIFY_TILE_W_LOG2=k: a tile is 2^k lanes wide and 256 / 2^k rows
              high, a lane being 4 pixels) or with float32 coordinates (-DPBR_RECTIFY_COORD=float: NOT the product -- it is here to price
              the float64 projective map), each a small library of its own next to this file (`--build`, on the machine that has hipcc);
  baseline    what a user writes today with ATen on the same device and data, per photograph: uint8 -> float and permute, the clip mask,
              the sampling grid, two grid_sample calls (image, coverage), avg_pool2d for S > 1, divide and clamp.  float32 throughout.

HIP events around the call, 3 warm-ups, the median of 20, the candidates alternating.  Bytes moved by the kernel: 16 per output pixel
written plus every source sample once.  Run by hand; not a test, asserts no duration.

    python tools/rectify_probe.py --build                      # compiles the variants (no GPU needed)
    python tools/rectify_probe.py [--out profiles/rectify_probe.json] [--sizes 4096,1024] [--supersample 1,2,4]"""
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
VARIANTS = {          # name -> extra flags; "tile8x32" is the product's shape, built the same way so that the variants compare like with like
    "tile8x32": ["-DPBR_RECTIFY_TILE_W_LOG2=3"], "tile16x16": ["-DPBR_RECTIFY_TILE_W_LOG2=4"], "tile32x8": ["-DPBR_RECTIFY_TILE_W_LOG2=5"],
    "tile64x4": ["-DPBR_RECTIFY_TILE_W_LOG2=6"], "tile4x64": ["-DPBR_RECTIFY_TILE_W_LOG2=2"],
    "f32coords": ["-DPBR_RECTIFY_TILE_W_LOG2=3", "-DPBR_RECTIFY_COORD=float"],
}
HBM_PEAK = 8.0e12     # bytes / s, the MI355X's specification


def variant_path(name):
    return os.path.join(ROOT, "tools", "librectify_%s.so" % name)


def build_variants():
    flags = ["-O3", "-std=c++17", "-fPIC", "--offload-arch=gfx950", "-ffp-contract=on", "-fno-slp-vectorize", "-fno-gpu-rdc", "-Wno-unused-function"]
    jobs = [subprocess.Popen([os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")] + flags + extra + ["-shared", os.path.join(CSRC, "rectify.hip"), "-o", variant_path(name)])
            for name, extra in VARIANTS.items()]
    if any(j.wait() for j in jobs):
        sys.exit("a variant did not build")
    print("built", ", ".join(VARIANTS))


ap = argparse.ArgumentParser()
ap.add_argument("--build", action="store_true")
ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "rectify_probe.json"))
ap.add_argument("--sizes", default="4096,1024")
ap.add_argument("--supersample", default="1,2,4")
ap.add_argument("--images", type=int, default=8)
ap.add_argument("--source", default="3000,4000")
ap.add_argument("--reps", type=int, default=20)
args = ap.parse_args()
if args.build:
    build_variants()
    sys.exit(0)

import numpy as np  # noqa: E402
import torch  # noqa: E402
import torch.nn.functional as TF  # noqa: E402

from pypbr_amd import _native as N, capture  # noqa: E402

assert torch.cuda.is_available(), "the probe measures on a ROCm device"
dev = torch.device("cuda", 0)
REPS, WARM = args.reps, 3
L = args.images
Hs, Ws = (int(v) for v in args.source.split(","))
CLIP = 250


def shot_corners(l):
    """The grid's corners in photograph l: a square of 0.8 Hs, turned by 4 + l degrees about the photograph's centre, its far edge drawn in
    by 6 % (a tilted camera)."""
    a, half = math.radians(4.0 + l), 0.4 * Hs
    out = []
    for sx, sy, k in ((-1, -1, 0.94), (1, -1, 0.94), (1, 1, 1.0), (-1, 1, 1.0)):
        x, y = sx * half * k, sy * half
        out.append((Ws / 2 + x * math.cos(a) - y * math.sin(a) + 7.3 * l, Hs / 2 + x * math.sin(a) + y * math.cos(a) - 5.1 * l))
    return out


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
    fn = lib.pbr_rectify_images
    fn.argtypes = N.lib().pbr_rectify_images.argtypes
    fn.restype = ctypes.c_int
    return fn


def baseline(photos, homs, size, S, clip, out_t, out_w):
    """One photograph at a time (at S = 4 the grid of all eight would be 17 GB)."""
    H, W = size
    ys = (torch.arange(H * S, device=dev, dtype=torch.float32) + 0.5) / S
    xs = (torch.arange(W * S, device=dev, dtype=torch.float32) + 0.5) / S
    Y, X = torch.meshgrid(ys, xs, indexing="ij")
    for l in range(photos.shape[0]):
        m = homs[l]
        img = photos[l].permute(2, 0, 1).float().div_(255.0)[None]
        if clip:
            ones = (photos[l].amax(dim=2) < clip).float()[None, None]
            img = img * ones
        else:
            ones = torch.ones((1, 1, Hs, Ws), device=dev)
        d = m[2][0] * X + m[2][1] * Y + m[2][2]
        u, v = (m[0][0] * X + m[0][1] * Y + m[0][2]) / d, (m[1][0] * X + m[1][1] * Y + m[1][2]) / d
        grid = torch.stack([u * (2.0 / Ws) - 1.0, v * (2.0 / Hs) - 1.0], dim=-1)[None]
        grid = torch.where((d > 0)[None, ..., None], grid, torch.full_like(grid, -3.0))
        val = TF.grid_sample(img, grid, mode="bilinear", padding_mode="zeros", align_corners=False)
        cov = TF.grid_sample(ones, grid, mode="bilinear", padding_mode="zeros", align_corners=False)
        if S > 1:
            val, cov = TF.avg_pool2d(val, S), TF.avg_pool2d(cov, S)
        out_w[l] = cov[0]
        out_t[l] = torch.where(cov > 0, (val / cov).clamp_(0.0, 1.0), torch.zeros_like(val))[0]


torch.manual_seed(5)
photos = torch.randint(0, 256, (L, Hs, Ws, 3), dtype=torch.uint8, device=dev)
libs = {"product": N.lib().pbr_rectify_images}
for name in VARIANTS:
    if os.path.exists(variant_path(name)):
        libs[name] = entry_point(ctypes.CDLL(variant_path(name)))
    else:
        print("variant %s is not built (tools/rectify_probe.py --build): skipped" % name)
records = []
for size in [int(v) for v in args.sizes.split(",")]:
    H = W = size
    homs = capture.homography_from_corners(np.array([shot_corners(l) for l in range(L)]), (H, W))
    table = (ctypes.c_double * (9 * L))(*homs.reshape(-1).tolist())
    homs32 = homs.float().tolist()
    bufs = {k: (torch.empty((L, 3, H, W), device=dev), torch.empty((L, 1, H, W), device=dev)) for k in list(libs) + ["baseline"]}
    for S in [int(v) for v in args.supersample.split(",")]:
        stream = torch.cuda.current_stream().cuda_stream

        def call(fn, t, w, clip=CLIP):
            def go():
                rc = fn(photos.data_ptr(), L, Hs, Ws, Hs * Ws * 3, Ws * 3, 3, 1, table, t.data_ptr(), w.data_ptr(), H, W, S, clip, 0, stream)
                assert rc == 0, rc
            return go
        names = list(libs)
        fns = [call(libs[k], *bufs[k]) for k in names] + [lambda: baseline(photos, homs32, (H, W), S, CLIP, *bufs["baseline"])]
        t = median_us(fns)
        ref_t, ref_w = bufs["product"]
        agree = {}
        for k in names[1:] + ["baseline"]:
            agree[k] = {"targets_x_weights_max_abs_diff": float((bufs[k][0] * bufs[k][1] - ref_t * ref_w).abs().max()),
                        "weights_max_abs_diff": float((bufs[k][1] - ref_w).abs().max()),
                        "bit_equal": bool(torch.equal(bufs[k][0], ref_t) and torch.equal(bufs[k][1], ref_w))}
        nbytes = 16 * L * H * W + L * Hs * Ws * 3
        rec = {"grid": size, "supersample": S, "clip_level": CLIP, "images": L, "source": [Hs, Ws, 3],
               "time_us": {k: round(v, 1) for k, v in zip(names + ["baseline"], t)},
               "bytes_moved": nbytes, "product_bytes_per_s": round(nbytes / (t[0] * 1e-6), 0),
               "product_fraction_of_hbm_peak": round(nbytes / (t[0] * 1e-6) / HBM_PEAK, 4),
               "baseline_over_product": round(t[-1] / t[0], 2),
               "f32coords_over_f64": round(t[names.index("f32coords")] / t[names.index("tile8x32")], 4) if "f32coords" in names else None,
               "against_product": agree,
               "covered_share": float((ref_w > 0).float().mean())}
        records.append(rec)
        print(json.dumps(rec), flush=True)
    del bufs
    torch.cuda.empty_cache()

out = {"what": "photograph rectification (csrc/rectify.hip): the library's kernel, the same source under other tile shapes and with float32 "
               "coordinates, and the ATen composition a user writes today; %d photographs of %d x %d x 3 (tools/rectify_probe.py)" % (L, Hs, Ws),
       "timing": "HIP events around the call, %d warm-ups, median of %d, the candidates alternating in one process; the baseline's time "
                 "includes its uint8 -> float conversion and grid construction, the kernel reads the uint8 samples as they are" % (WARM, REPS),
       "hbm_peak_bytes_per_s": HBM_PEAK, "device": torch.cuda.get_device_name(0), "stamp": N.build_stamp(), "records": records}
os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
with open(args.out, "w") as f:
    json.dump(out, f, indent=1)
print("wrote", args.out)
