"""Material rotation: upstream's rotate family (MaterialBase.rotate, base.py:539-603; transforms `Rotate` / `RandomRotate`,
transforms.py:206-273; `random_rotate`'s draw, transforms/functional.py:202-228) on the MI355X.

Upstream pads every map, rotates it with torchvision's nearest-neighbour `rotate(expand=True)`, centre-crops it back and rotates the
normal vectors.  Here the whole chain is one closed-form index function per output pixel (functional.rotate_plan) and one
`pbr_rotate_planes` launch over all planes of a block of maps, the normal map's vectors rotated in the same launch: no padded copy, no
grid tensor, no torchvision.

    rotation.rotate(material, 33.3)                         # in place, returns the material: MaterialBase.rotate's semantics
    rotation.random_rotate(material, 0.0, 360.0)            # the same after upstream's draw from random.random()
    Compose([RandomCrop(24, 24), rotation.RandomRotate(), Tile(2)])        # the classes return a NEW material, as every transform does

The module stands on its own: `transforms`, `transforms.functional` and `MaterialBase` do not carry the upstream names yet
(INTEGRATION.md).  A `Rotate` instance is an ordinary callable to `Compose`: it ends a fused run of geometric stages.
"""
from random import random

import torch

from . import functional as F_
from .materials import MaterialBase, _as_block

__all__ = ["rotate", "random_rotate", "Rotate", "RandomRotate"]


def rotate(material: MaterialBase, angle: float, expand: bool = False, padding_mode: str = "constant") -> MaterialBase:
    """Rotates every map of `material` by `angle` degrees IN PLACE and returns it (base.py:539-603).  All float32 (C,H,W) maps of one
    size -- one shared allocation after from_tensor, an upload or a resize -- go through ONE pbr_rotate_planes launch over all their
    planes, the normal map among them; other maps (batches, fp16, maps that require grad) one launch each through the differentiable
    path; a material whose maps differ in size gets one launch per size.  Host-resident and image-backed materials travel to the device
    first, as for `crop`; a pending lazy blend or lazy tile is carried out first.  ValueError for a padding mode other than "constant" /
    "circular" and for a circular padding that does not fit a map (upstream's F.pad raises there) -- before any device work."""
    if padding_mode not in F_.PADDING_MODES:
        raise ValueError("Invalid padding mode %r. Must be 'constant' or 'circular'." % (padding_mode,))
    material.materialize_blend()
    material.materialize_tile()
    for name, t in material._raw.items():
        if t is not None:
            F_.rotate_plan(t.shape[-2], t.shape[-1], angle, expand, padding_mode)          # raises for a padding that does not fit
            if name == "normal" and t.shape[-3] != 3:
                raise ValueError("Normal map must have 3 channels, got shape %s" % (tuple(t.shape),))
    maps = material._resident(keep=True)
    store = material._raw

    def run(t, nfp):
        return F_.rotate_maps(t, angle, expand, padding_mode, normal_first_plane=nfp)
    groups = {}
    for name, t in maps.items():
        if t.dim() == 3 and t.dtype == torch.float32 and t.shape[0] <= 32 and not (t.requires_grad and torch.is_grad_enabled()):
            groups.setdefault(tuple(t.shape[-2:]), []).append(name)
        elif t.shape[-3] <= 32:
            store[name] = run(t, 0 if name == "normal" else None)
        else:                                                    # a map of more than 32 planes: blocks of 32
            store[name] = torch.cat([run(t[..., i:i + 32, :, :], None) for i in range(0, t.shape[-3], 32)], dim=-3)
    for names in groups.values():
        names.sort(key=lambda k: maps[k].data_ptr())
        while names:                                             # at most 32 planes share a launch
            take, planes = [], 0
            while names and planes + maps[names[0]].shape[0] <= 32:
                planes += maps[names[0]].shape[0]
                take.append(names.pop(0))
            ts = [maps[k] for k in take]
            first = {k: sum(t.shape[0] for t in ts[:i]) for i, k in enumerate(take)}
            out = run(_as_block(ts), first.get("normal"))
            for k, t in zip(take, ts):
                store[k] = out[first[k]:first[k] + t.shape[0]]
    return material


def random_angle(min_angle: float = 0.0, max_angle: float = 360.0) -> float:
    """The angle as transforms/functional.py:223 draws it: after random.seed(k) it is upstream's."""
    return min_angle + (max_angle - min_angle) * random()


def random_rotate(material: MaterialBase, min_angle: float = 0.0, max_angle: float = 360.0, expand: bool = False,
                  padding_mode: str = "constant") -> MaterialBase:
    """`rotate` by an angle drawn as upstream draws it (one random.random()); in place, returns the material."""
    if padding_mode not in F_.PADDING_MODES:                     # before the draw: a refused call leaves the random stream alone
        raise ValueError("Invalid padding mode %r. Must be 'constant' or 'circular'." % (padding_mode,))
    return rotate(material, random_angle(min_angle, max_angle), expand=expand, padding_mode=padding_mode)


class Rotate:
    """transforms.py:206-236: rotates all maps by `angle` degrees; returns a new material (every map is replaced, so the input's tensors
    are shared until then and nothing is cloned)."""

    def __init__(self, angle: float, expand: bool = False, padding_mode: str = "constant"):
        if padding_mode not in F_.PADDING_MODES:
            raise ValueError("Invalid padding mode.")
        self.angle, self.expand, self.padding_mode = angle, expand, padding_mode

    def __call__(self, material: MaterialBase) -> MaterialBase:
        return rotate(_fresh(material), self.angle, expand=self.expand, padding_mode=self.padding_mode)


class RandomRotate:
    """transforms.py:239-273: rotates all maps by an angle drawn from [min_angle, max_angle) at every call; returns a new material."""

    def __init__(self, min_angle: float = 0.0, max_angle: float = 360.0, expand: bool = False, padding_mode: str = "constant"):
        if padding_mode not in F_.PADDING_MODES:
            raise ValueError("Invalid padding mode.")
        self.min_angle, self.max_angle, self.expand, self.padding_mode = min_angle, max_angle, expand, padding_mode

    def __call__(self, material: MaterialBase) -> MaterialBase:
        return random_rotate(_fresh(material), self.min_angle, self.max_angle, expand=self.expand, padding_mode=self.padding_mode)


def _fresh(material: MaterialBase) -> MaterialBase:
    """A material over the same tensors with a map dict of its own: rotate replaces every map, the input keeps its own.  Pending lazy
    work is carried out on the input first, once, not on every copy."""
    material.materialize_blend()
    material.materialize_tile()
    return material._shallow()
