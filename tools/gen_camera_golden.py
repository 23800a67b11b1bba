#!/usr/bin/env python3
"""Writes tests/golden/camera.npz: the perspective camera's fixture, from the real upstream package.

Runs where upstream exists (imported through oracle/ref_import.py); the tests only read the file.  Definition: with a camera at C, pixel
(y, x) of the render equals pixel (y, x) of upstream's CookTorranceBRDF.forward called with view_dir = C - P(y, x), P the surface point of
the point light's grid.  So every case is evaluated PIXEL BY PIXEL: H*W upstream calls on real BasecolorMetallicMaterial /
DiffuseSpecularMaterial objects, one pixel kept from each.

Per case the file holds the inputs (maps as stored -- float16 for the fp16 case, evaluated as their float32 values --, camera, lights,
intensities, light_size and the flags, the latter as one JSON string under "cases"), `ref32` (upstream, float32) and `ref64` (the same
evaluation in float64 through oracle/torch_oracle.py, which is pinned bit-equal to upstream).  Several lights are upstream calls summed the
way the library sums them: per-light clamp (upstream's own, return_srgb=False), sum, clamp, upstream's linear_to_srgb.

The inputs are drawn so that the camera matters: roughness in [0.2, 1] (above every recorded parity threshold), normals with n_z > 0 --
N.V > 0 everywhere for the orthographic view (0, 0, 1) -- but tilted enough that N.V changes sign across the image for the camera.  The
script asserts that, and that neither zeros nor saturated values cover more than half of a case.
"""
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "oracle"))
sys.path.insert(0, os.path.join(ROOT, "tools"))
from ref_import import import_reference  # noqa: E402
import torch_oracle as T  # noqa: E402
import camera_oracle as CO  # noqa: E402

CAMERAS = {"near_axis": [0.1, -0.2, 1.5], "close": [0.0, 0.0, 0.6], "on_pixel": [0.0, 0.0, 0.0]}
LIGHTS = {   # light_type -> up to three lights (position | direction) and their intensities
    "point": ([[0.1, 0.1, 1.0], [-0.3, 0.2, 1.4], [0.25, -0.35, 0.9]], [[1.0, 1.0, 1.0], [0.8, 0.6, 0.5], [0.3, 0.5, 0.9]]),
    "directional": ([[0.1, 0.1, 1.0], [-0.2, 0.15, 1.0], [0.3, -0.1, 0.8]], [[0.9, 0.9, 0.9], [0.5, 0.4, 0.3], [0.2, 0.3, 0.6]]),
}
# name: shape ([B,] H, W), workflow, light type, lights, sRGB (albedo / specular decode and result encode) on, normal map, light_size, camera, fp16 maps
CASES = [
    dict(name="A_metallic_point_1", shape=(7, 12), workflow="metallic", light_type="point", L=1, srgb=True, normal=True, light_size=1.0, camera="near_axis"),
    dict(name="A_specular_directional_3", shape=(7, 12), workflow="specular", light_type="directional", L=3, srgb=False, normal=True, light_size=2.0, camera="close"),
    dict(name="A_converted_point_3", shape=(7, 12), workflow="converted", light_type="point", L=3, srgb=True, normal=True, light_size=1.0, camera="close"),
    dict(name="A_metallic_directional_1_flat", shape=(7, 12), workflow="metallic", light_type="directional", L=1, srgb=True, normal=False, light_size=2.0, camera="near_axis"),
    dict(name="B_specular_point_1", shape=(5, 9), workflow="specular", light_type="point", L=1, srgb=True, normal=True, light_size=1.0, camera="close"),
    dict(name="B_metallic_directional_3", shape=(5, 9), workflow="metallic", light_type="directional", L=3, srgb=False, normal=True, light_size=2.0, camera="near_axis"),
    dict(name="B_converted_directional_1", shape=(5, 9), workflow="converted", light_type="directional", L=1, srgb=True, normal=True, light_size=1.0, camera="close"),
    dict(name="B_specular_point_1_on_pixel", shape=(5, 9), workflow="specular", light_type="point", L=1, srgb=True, normal=True, light_size=1.0, camera="on_pixel",
         inputs_of="B_specular_point_1", forward_only=True),
    dict(name="C_metallic_point_1_f16", shape=(2, 6, 16), workflow="metallic", light_type="point", L=1, srgb=True, normal=True, light_size=1.0, camera="near_axis", f16=True),
    dict(name="C_converted_point_3_f16", shape=(2, 6, 16), workflow="converted", light_type="point", L=3, srgb=False, normal=True, light_size=2.0, camera="close", f16=True),
    dict(name="C_specular_directional_3_f16", shape=(2, 6, 16), workflow="specular", light_type="directional", L=3, srgb=True, normal=True, light_size=1.0, camera="close", f16=True),
]


def draw(seed, shape, f16):
    """One material (or a batch): roughness in [0.2, 1]; unit normals with n_z > 0, tilted up to ~76 degrees."""
    g = torch.Generator().manual_seed(seed)
    lead = tuple(shape[:-2])
    H, W = shape[-2:]
    a = torch.rand(*lead, 3, H, W, generator=g)
    nxy = torch.rand(*lead, 2, H, W, generator=g) * 2 - 1
    n = torch.cat([nxy, torch.full((*lead, 1, H, W), 0.35)], dim=-3)
    n = n / n.norm(dim=-3, keepdim=True)
    r = torch.rand(*lead, 1, H, W, generator=g) * 0.8 + 0.2
    m = torch.rand(*lead, 1, H, W, generator=g)
    s = torch.rand(*lead, 3, H, W, generator=g) * 0.5
    if f16:
        a, n, r, m, s = (t.half() for t in (a, n, r, m, s))
        r = r.clamp(min=0.2)
    return a, n, r, m, s


def upstream_pixelwise(pypbr, case, maps, C, lights, intens):
    """ref32 (3,H,W): upstream's forward once per pixel, with that pixel's C - P as view_dir."""
    from pypbr.materials import BasecolorMetallicMaterial, DiffuseSpecularMaterial
    from pypbr.models import CookTorranceBRDF
    from pypbr.utils import linear_to_srgb
    a, n, r, m, s = maps
    srgb = case["srgb"]
    if case["workflow"] == "specular":
        mat = DiffuseSpecularMaterial(albedo=a, normal=n, roughness=r, specular=s, albedo_is_srgb=srgb, specular_is_srgb=srgb)
    else:
        mat = BasecolorMetallicMaterial(albedo=a, normal=n, roughness=r, metallic=m, albedo_is_srgb=srgb)
        if case["workflow"] == "converted":
            mat = mat.to_diffuse_specular_material()        # albedo_is_srgb False, specular_is_srgb True (upstream's second decode)
    if n is None:
        mat.normal = None
    brdf = CookTorranceBRDF(light_type=case["light_type"])
    _, H, W = a.shape
    e = CO.view_offsets(C, H, W, case["light_size"])
    out = torch.zeros(3, H, W)
    for y in range(H):
        for x in range(W):
            view = e[:, y, x].clone()
            if case["L"] == 1:
                px = brdf(mat, view, lights[0], intens[0], case["light_size"], return_srgb=srgb)
            else:
                px = sum(brdf(mat, view, lights[l], intens[l], case["light_size"], return_srgb=False) for l in range(case["L"])).clamp(0.0, 1.0)
                px = linear_to_srgb(px) if srgb else px
            out[:, y, x] = px[:, y, x]
    return out


def oracle_pixelwise(case, maps, C, lights, intens):
    """ref64 (3,H,W): the same, through torch_oracle in float64."""
    a, n, r, m, s = (None if t is None else t.double() for t in maps)
    srgb = case["srgb"]
    _, H, W = a.shape
    e = CO.view_offsets(C.double(), H, W, case["light_size"])
    kw = dict(light_type=case["light_type"], light_size=case["light_size"], return_srgb=srgb)
    out = torch.zeros(3, H, W, dtype=torch.float64)
    for y in range(H):
        for x in range(W):
            view = e[:, y, x].clone()
            if case["workflow"] == "converted":
                def one(l, rs):
                    return T.cook_torrance_converted(a, n, r, m, albedo_is_srgb=srgb, view=view, light=lights[l].double(), intensity=intens[l].double(),
                                                     **dict(kw, return_srgb=rs))
            else:
                def one(l, rs):
                    return T.cook_torrance(a, n, r, m if case["workflow"] == "metallic" else None, s if case["workflow"] == "specular" else None,
                                           albedo_is_srgb=srgb, specular_is_srgb=srgb, view=view, light=lights[l].double(), intensity=intens[l].double(),
                                           **dict(kw, return_srgb=rs))
            if case["L"] == 1:
                px = one(0, srgb)
            else:
                px = sum(one(l, False) for l in range(case["L"])).clamp(0.0, 1.0)
                px = T.linear_to_srgb(px) if srgb else px
            out[:, y, x] = px[:, y, x]
    return out


def ndv_signs(n, C, light_size):
    """(N.V for the camera, N.V for the orthographic view (0,0,1)) of one (3,H,W) unit normal map, float64."""
    _, H, W = n.shape
    v = torch.nn.functional.normalize(CO.view_offsets(C.double(), H, W, light_size), dim=0)
    nn_ = torch.nn.functional.normalize(n.double(), dim=0)
    return (nn_ * v).sum(0), nn_[2]


def main():
    torch.set_num_threads(8)
    pypbr = import_reference()
    data, meta, drawn = {}, [], {}
    for case in CASES:
        name, shape = case["name"], case["shape"]
        batched = len(shape) == 3
        C = torch.tensor(CAMERAS[case["camera"]])
        lights = torch.tensor(LIGHTS[case["light_type"]][0][:case["L"]])
        intens = torch.tensor(LIGHTS[case["light_type"]][1][:case["L"]])
        if case.get("inputs_of"):
            seed, maps = drawn[case["inputs_of"]]
        else:
            seed = 1000 + 17 * len(meta)
            while True:                 # the first seed whose normals make N.V change sign for the camera (asserted below for what is kept)
                maps = draw(seed, shape, case.get("f16", False))
                mats = maps[1] if batched else maps[1][None]
                if not case["normal"] or all((ndv_signs(nm.float(), C, case["light_size"])[0] < 0).any() for nm in mats):
                    break
                seed += 1
            drawn[name] = (seed, maps)
        a, n, r, m, s = maps
        if not case["normal"]:
            n = None
        per_material = []
        for b in range(shape[0] if batched else 1):
            pick = lambda t: None if t is None else (t[b] if batched else t).float()
            mb = tuple(pick(t) for t in (a, n, r, m, s))
            ref32 = upstream_pixelwise(pypbr, case, mb, C, lights, intens)
            ref64 = oracle_pixelwise(case, mb, C, lights, intens)
            assert torch.isfinite(ref32).all() and torch.isfinite(ref64).all(), name
            if mb[1] is not None and not case.get("forward_only"):
                cam, ortho = ndv_signs(mb[1], C, case["light_size"])
                assert (cam < 0).any() and (cam > 0).any() and (ortho > 0).all(), (name, "N.V must change sign for the camera only")
            if not case.get("forward_only"):
                assert (ref64 <= 0).double().mean() <= 0.5 and (ref64 >= 1).double().mean() <= 0.5, (name, "more than half zero or saturated")
            per_material.append((ref32, ref64))
            print("%-34s b=%d  |ref32 - ref64| = %.2e  zeros %.0f %%  saturated %.0f %%" % (
                name, b, (ref32.double() - ref64).abs().max(), 100 * (ref64 <= 0).double().mean(), 100 * (ref64 >= 1).double().mean()))
        stack = lambda i: torch.stack([p[i] for p in per_material]) if batched else per_material[0][i]
        for key, t in (("albedo", a), ("normal", n), ("roughness", r), ("metallic", m), ("specular", s)):
            if t is not None and (key not in ("metallic", "specular") or (key == "specular") == (case["workflow"] == "specular")):
                data["%s/%s" % (name, key)] = t.numpy()
        data["%s/camera" % name] = C.numpy()
        data["%s/lights" % name] = lights.numpy()
        data["%s/intensities" % name] = intens.numpy()
        data["%s/ref32" % name] = stack(0).numpy()
        data["%s/ref64" % name] = stack(1).numpy()
        meta.append({k: v for k, v in dict(case, seed=seed).items() if k != "inputs_of"})
    data["cases"] = np.array(json.dumps(meta))
    path = os.path.join(ROOT, "tests", "golden", "camera.npz")
    np.savez_compressed(path, **data)
    print("wrote %s: %d cases, %d bytes" % (path, len(meta), os.path.getsize(path)))


if __name__ == "__main__":
    main()
