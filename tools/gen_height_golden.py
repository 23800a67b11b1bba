"""Writes tests/golden/height_ops.npz and tests/golden/height_ops_grad.npz: the REAL reference's compute_height_from_normal
(pypbr/utils/functions.py:180-323), its divergence and its autograd, next to this tool's own float64 evaluation of the same definition --
the fixtures of tests/test_gpu_height_ops.py.  Development container only: it imports the reference through
oracle/ref_import.import_reference() (nothing under oracle/ is changed).  Only float arrays are stored (the torch version and the ATen
thread count as float arrays too: meta_torch, meta_threads).  Two files, so that each stays below 1 MiB.

    python tools/gen_height_golden.py [OUT_DIR]        (default: tests/golden)

height_ops.npz       in__<input> the normal map; per case <input>__<scale>__<convention>:
                     div__<case>   upstream's _compute_divergence of upstream's gradient field (float32)
                     ref32__<case> upstream's float32 output
                     ref64__<case> height64() below in float64, stored as float64
height_ops_grad.npz  for the FIRST case of every input: G__<case> a seeded upstream gradient, g32__<case> upstream's float32 autograd
                     of sum(G out), g64__<case> float64 autograd of height64() (stored as float32)

ref64 is this tool's evaluation because upstream hard-codes float32 frequency grids (functions.py:300-301): feeding it float64 normals
does not give a float64 evaluation.  height64() is upstream's definition with the Laplacian's eigenvalues written as
-4 (sin^2(pi kx / W) + sin^2(pi ky / H)), which is (2 cos(2 pi kx / W) - 2) + (2 cos(2 pi ky / H) - 2) exactly.

The tool asserts what the tests rely on: no ties among the extrema (the two smallest and the two largest values of every ref64 at
least 1e-3 apart), and |ref32 - ref64| <= 5e-6 on every shape up to 64 x 64.
"""
import math
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden")
CROP = 96
THREADS = 8
SMALL = 64 * 64                      # "up to 64 x 64": the shapes on which upstream's float32 is itself within 5e-6 of float64
# (scale, convention) varied across the inputs, not crossed; the first case of an input carries the gradients
CASES = {
    "n1x1": ((1.0, "opengl"), (2.5, "directx")),
    "n1x17": ((2.5, "opengl"), (1.0, "directx")),
    "n5x1": ((1.0, "directx"), (2.5, "opengl")),
    "n2x2": ((2.5, "directx"), (1.0, "opengl")),
    "n37x53": ((1.0, "opengl"), (2.5, "directx")),
    "n64x64": ((2.5, "opengl"),),
    "n72x200": ((1.0, "directx"),),
    "tiles": ((1.0, "opengl"),),
}


def _synthetic():
    """Seeded unit normals with n_z >= 0.3."""
    g = torch.Generator().manual_seed(20261018)
    maps = {}
    for name in CASES:
        if name == "tiles":
            continue
        h, w = (int(v) for v in name[1:].split("x"))
        z = 0.3 + 0.7 * torch.rand(1, h, w, generator=g)
        phi = 2.0 * math.pi * torch.rand(1, h, w, generator=g)
        r = torch.sqrt(1.0 - z * z)
        n = torch.cat([r * torch.cos(phi), r * torch.sin(phi), z])
        n = n / n.norm(dim=0, keepdim=True)
        assert float(n[2].min()) >= 0.3 - 1e-6
        maps[name] = n
    return maps


def height64(normal, scale, directx):
    """The definition in float64 (differentiable): (3,H,W) -> (1,H,W)."""
    n = normal.double()
    ze = n[2] + 1e-8
    gx, gy = -n[0] / ze * scale, (n[1] if directx else -n[1]) / ze * scale
    dgx = torch.cat([gx[:, 1:], gx[:, -1:]], 1) - gx
    dgy = torch.cat([gy[1:], gy[-1:]], 0) - gy
    div = dgx + dgy
    H, W = div.shape
    ky = torch.arange(H, dtype=torch.float64).view(-1, 1)
    kx = torch.arange(W, dtype=torch.float64).view(1, -1)
    den = -4.0 * (torch.sin(math.pi * kx / W) ** 2 + torch.sin(math.pi * ky / H) ** 2)
    den[0, 0] = 1.0
    keep = torch.ones(H, W, dtype=torch.float64)
    keep[0, 0] = 0.0
    h = torch.fft.ifft2(torch.fft.fft2(div) / den * keep).real
    h = h - h.mean()
    mn, mx = h.min(), h.max()
    return ((h - mn) / (mx - mn + 1e-8))[None]


def case_key(name, scale, conv):
    return "%s__%g__%s" % (name, scale, conv)


def generate(out_dir: str):
    sys.path.insert(0, os.path.join(ROOT, "oracle"))
    from ref_import import import_reference
    import_reference()
    from pypbr.io import load_material_from_folder
    from pypbr.utils.enums import NormalConvention
    from pypbr.utils.functions import _compute_divergence, compute_height_from_normal

    torch.set_num_threads(THREADS)
    conventions = {"opengl": NormalConvention.OPENGL, "directx": NormalConvention.DIRECTX}
    normals = _synthetic()
    mat = load_material_from_folder(os.path.join(GOLDEN, "tiles"), preferred_workflow="metallic")
    normals["tiles"] = mat._maps["normal"][:, :CROP, :CROP].contiguous().float()

    fwd, grad = {}, {}
    g = torch.Generator().manual_seed(77)
    for name, cases in CASES.items():
        n = normals[name]
        fwd["in__" + name] = n
        for ci, (scale, conv) in enumerate(cases):
            key = case_key(name, scale, conv)
            # upstream's gradient field, statement by statement (functions.py:206-225), through upstream's own divergence
            nz = n[2] + 1e-8
            gx = -n[0] / nz
            gy = -n[1] / nz if conv == "opengl" else n[1] / nz
            fwd["div__" + key] = _compute_divergence(gx * scale, gy * scale)
            ref32 = compute_height_from_normal(n.clone(), scale, convention=conventions[conv])
            ref64 = height64(n, scale, conv == "directx")
            fwd["ref32__" + key], fwd["ref64__" + key] = ref32, ref64
            flat = np.sort(ref64.numpy().reshape(-1))
            if flat.size >= 2:
                assert flat[1] - flat[0] >= 1e-3 and flat[-1] - flat[-2] >= 1e-3, (key, flat[1] - flat[0], flat[-1] - flat[-2])
            err = float((ref32.double() - ref64).abs().max())
            print("%-28s |ref32 - ref64| max %.2e" % (key, err))
            if n.shape[1] * n.shape[2] <= SMALL:
                assert err <= 5e-6, (key, err)
            if ci == 0:
                G = torch.randn(ref32.shape, generator=g)
                a = n.clone().requires_grad_()
                (compute_height_from_normal(a, scale, convention=conventions[conv]) * G).sum().backward()
                b = n.clone().double().requires_grad_()
                (height64(b, scale, conv == "directx") * G.double()).sum().backward()
                grad["G__" + key], grad["g32__" + key], grad["g64__" + key] = G, a.grad, b.grad.float()
                print("%-28s |g32 - g64| max %.2e (|g64| max %.2e)" % (key, float((a.grad.double() - b.grad).abs().max()), float(b.grad.abs().max())))

    paths = []
    for fname, z in (("height_ops.npz", fwd), ("height_ops_grad.npz", grad)):
        arrays = {k: np.ascontiguousarray(v.detach().numpy()) for k, v in z.items()}
        for k, a in arrays.items():
            assert a.dtype == (np.float64 if k.startswith("ref64__") else np.float32), (k, a.dtype)
        arrays["meta_torch"] = np.frombuffer(torch.__version__.encode().ljust(32, b"\0"), dtype=np.uint8).astype(np.float32)
        arrays["meta_threads"] = np.array([torch.get_num_threads()], dtype=np.float32)
        os.makedirs(out_dir, exist_ok=True)
        path = os.path.join(out_dir, fname)
        np.savez_compressed(path, **arrays)
        assert os.path.getsize(path) < 2 ** 20, (path, os.path.getsize(path))
        paths.append(path)
    return paths


def meta(z) -> tuple:
    """(torch version, ATen threads) the file was generated with."""
    return bytes(z["meta_torch"].astype(np.uint8)).rstrip(b"\0").decode(), int(z["meta_threads"][0])


if __name__ == "__main__":
    for p in generate(sys.argv[1] if len(sys.argv) > 1 else GOLDEN):
        print("%s: %d bytes" % (p, os.path.getsize(p)))
