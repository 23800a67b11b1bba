"""The reference's utility functions (pypbr/utils/functions.py:31-177) with its names and signatures, evaluated by libpbr_hip.so.
CPU tensors are staged through the device; with no ROCm device present the call raises (no CPU arithmetic in this package).
compute_height_from_normal (functions.py:180-323) is built as functional.height_from_normal and MaterialBase.compute_height_from_normal;
its one-line re-export under upstream's name in this module is pending (an existing test pins the name's absence)."""
import math

import torch

from . import functional as _F
from .materials import NormalConvention, _through_device  # noqa: F401


def srgb_to_linear(texture: torch.Tensor) -> torch.Tensor:
    """sRGB -> linear, shape preserved: clamp to [0,1], x/12.92 below 0.04045,
    ((x+0.055)/1.055)**2.4 above, clamp."""
    return _through_device(texture, _F.srgb_to_linear)


def linear_to_srgb(texture: torch.Tensor) -> torch.Tensor:
    """linear -> sRGB, shape preserved: clamp to [0,1], 12.92x below 0.0031308,
    1.055 x**(1/2.4) - 0.055 above, clamp."""
    return _through_device(texture, _F.linear_to_srgb)


def _in_place(normal_map: torch.Tensor, matrix, renormalize: bool) -> torch.Tensor:
    """The reference's utilities write into their argument and return it: a device map is transformed where it is, a CPU map
    through the device and copied back, a map that requires grad through the differentiable transform and copy_."""
    if normal_map.dim() != 3 or normal_map.shape[0] != 3:
        raise ValueError("Normal map must be (3,H,W), got shape %s" % (tuple(normal_map.shape),))
    if normal_map.is_cuda and not (normal_map.requires_grad and torch.is_grad_enabled()) and _F._rows_dense(normal_map) is normal_map:
        return _F.transform_normals(normal_map, matrix, renormalize, out=normal_map)
    result = _F.transform_normals(normal_map, matrix, renormalize)
    return normal_map.copy_(result)


def rotate_normals(normal_map: torch.FloatTensor, angle: float) -> torch.FloatTensor:
    """functions.py:69-108: (x, y) rotated by `angle` degrees, z kept, renormalised; in place, returns `normal_map`.  cos and sin are
    taken in double on the host (math.radians / cos / sin) and used in fp32, as the reference's rotation matrix is."""
    theta = math.radians(angle)
    c, s = math.cos(theta), math.sin(theta)
    return _in_place(normal_map, ((c, -s), (s, c)), True)


def invert_normal(normals: torch.FloatTensor) -> torch.FloatTensor:
    """functions.py:111-120: y negated, no renormalisation; in place, returns `normals` (None stays None)."""
    if normals is None:
        return None
    return _in_place(normals, ((1.0, 0.0), (0.0, -1.0)), False)


def compute_normal_from_height(height_map: torch.FloatTensor, scale: float = 1.0,
                               convention: NormalConvention = NormalConvention.OPENGL) -> torch.FloatTensor:
    """functions.py:123-177: (H,W) | (1,H,W) height -> (3,H,W) normals, zero padding, a = -(gx scale), b = -+(gy scale), z = 1,
    normalised.  A new tensor on the height's device.  A height with more than one channel raises ValueError (upstream would
    build a 3C-channel result)."""
    return _F.normal_from_height(height_map, scale, convention)
