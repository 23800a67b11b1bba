"""CPU statement of the perspective camera (`view_type="point"`): the Cook-Torrance evaluation with a (3,H,W) VIEW MAP.

TEST INFRASTRUCTURE ONLY (tests/test_camera_host.py, tests/test_gpu_camera.py; the product never imports it).

Definition: the argument upstream calls `view_dir` is a camera position C in the point light's coordinates; the surface
point of pixel (y, x) is P = (xs[x], -ys[y], 0) with xs = linspace(-s/2, s/2, W), ys = linspace(-s/2, s/2, H_total), s = light_size or
1.0 -- the point light's grid (cooktorrance.py:130-136), for both light types -- and that pixel's view vector is F.normalize(C - P).
Pixel (y, x) of the result is pixel (y, x) of upstream's forward called with view_dir = C - P(y, x); tests/golden/camera.npz holds
exactly that, evaluated pixel by pixel by tools/gen_camera_golden.py.  This file says the same for all pixels at once: the terms are
oracle/torch_oracle.py's (pinned bit-equal to upstream), called in its order, with the view a map instead of one expanded vector.  With
every pixel's view forced to one vector it therefore IS torch_oracle.cook_torrance, bit for bit.

Plain (C,H,W) tensors in, any float dtype (`dtype=`): float32 for parity, float64 for the gradient tests, which differentiate this file
with autograd.  Several lights sum as the library sums them (torch_oracle.cook_torrance_multi): per-light clamp, sum, clamp, encode.
"""
import math
import os
import sys
from typing import Optional

import torch
import torch.nn.functional as F

sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "oracle"))
import torch_oracle as T  # noqa: E402


def surface_points(H: int, W: int, light_size=None, y_offset: int = 0, H_total: Optional[int] = None) -> torch.Tensor:
    """(3,H,W) float32: P = (xs, -ys, 0) over the point light's grid -- float32 whatever the maps' dtype, as upstream's linspace is."""
    size = light_size or 1.0
    xs = torch.linspace(-size / 2, size / 2, W)
    ys = torch.linspace(-size / 2, size / 2, H if H_total is None else H_total)[y_offset:y_offset + H]
    yv, xv = torch.meshgrid(ys, xs, indexing="ij")
    return torch.stack([xv, -yv, torch.zeros_like(xv)], dim=0)


def view_offsets(camera: torch.Tensor, H: int, W: int, light_size=None, y_offset: int = 0, H_total: Optional[int] = None) -> torch.Tensor:
    """(3,H,W) in the camera's dtype: C - P, what each pixel hands upstream as its `view_dir`."""
    return camera.view(3, 1, 1) - surface_points(H, W, light_size, y_offset, H_total).to(camera.dtype)


def cook_torrance_camera(albedo, normal, roughness, metallic=None, specular=None, *, camera, lights, intensities,
                         light_type: str = "point", light_size=None, albedo_is_srgb: bool = True, specular_is_srgb: bool = True,
                         return_srgb: bool = True, converted: bool = False, y_offset: int = 0, H_total: Optional[int] = None,
                         view_map: Optional[torch.Tensor] = None, dtype: torch.dtype = torch.float64) -> torch.Tensor:
    """(3,H,W) in `dtype`.  `camera` [3], `lights` [L,3] (or [3]), `intensities` [L,3] / [1,3] / [3]: tensors (they may require grad).
    `converted`: BasecolorMetallicMaterial.to_diffuse_specular_material() first, then the specular workflow (torch_oracle.cook_torrance_converted,
    upstream's second decode of the specular map included).  `view_map` (3,H,W): UNIT view vectors to use instead of the camera's."""
    cast = lambda t: None if t is None else t.to(dtype)
    albedo, normal, roughness, metallic, specular = (cast(t) for t in (albedo, normal, roughness, metallic, specular))
    lights, intensities = lights.to(dtype).reshape(-1, 3), intensities.to(dtype).reshape(-1, 3)
    if intensities.shape[0] == 1 and lights.shape[0] > 1:
        intensities = intensities.expand(lights.shape[0], 3)
    _, H, W = albedo.shape
    H_total = H if H_total is None else H_total

    base = T.srgb_to_linear(albedo) if albedo_is_srgb else albedo
    if converted:
        base, specular = T.metallic_to_diffuse_specular(base, metallic)
        metallic = None
    if metallic is not None:
        f0 = torch.lerp(torch.full_like(base, 0.04), base, metallic)
    elif specular is not None:
        f0 = T.srgb_to_linear(specular) if specular_is_srgb else specular
    else:
        raise ValueError("Material must have either 'metallic' or 'specular' property.")

    if view_map is None:
        view_map = F.normalize(view_offsets(camera.to(dtype), H, W, light_size, y_offset, H_total), dim=0)
    vmap = view_map.to(dtype)
    if normal is None:
        normal = torch.tensor([0.0, 0.0, 1.0], dtype=dtype).view(3, 1, 1).expand(3, H, W)
    n = F.normalize(normal, dim=0)
    ndv = torch.clamp((n * vmap).sum(dim=0, keepdim=True), 0.0, 1.0)

    total = None
    for l in range(lights.shape[0]):
        lmap, att = T._light_geometry(light_type, lights[l], light_size, H, W, dtype, y_offset, H_total)
        half = F.normalize(vmap + lmap, dim=0)
        cos_theta = torch.clamp((half * vmap).sum(dim=0, keepdim=True), 0.0, 1.0)
        fr = T._fresnel(cos_theta, f0)
        ndf = T._ggx(n, half, roughness)
        geo = T._smith(n, vmap, lmap, roughness)
        ndl = torch.clamp((n * lmap).sum(dim=0, keepdim=True), 0.0, 1.0)
        spec = (fr * ndf * geo) / (4.0 * ndv * ndl + 1e-7)
        kd = (1.0 - fr) * (1.0 - metallic) if metallic is not None else 1.0 - fr
        diff = kd * base / math.pi
        radiance = intensities[l].view(3, 1, 1) * (ndl * att)
        color = torch.clamp((diff + spec) * radiance, 0.0, 1.0)
        total = color if total is None else total + color
    if lights.shape[0] > 1:
        total = torch.clamp(total, 0.0, 1.0)
    return T.linear_to_srgb(total) if return_srgb else total
