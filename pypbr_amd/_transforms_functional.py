"""The functional forms of pypbr.transforms (pypbr/transforms/functional.py), reachable as `pypbr_amd.transforms.functional`.

Each takes a material and returns a NEW one, leaving its argument untouched: the argument is cloned and the clone's in-place method runs
(kernels of libpbr_hip.so on a ROCm device).  The random forms draw from Python's `random.random()` in upstream's order and with upstream's
arithmetic (functional.py:87-88, :151-152, :273, :290), so after `random.seed(k)` they make upstream's choices.  The rotate family is not
among them (it is built apart from this module and not re-exported here): INTEGRATION.md.
"""
from random import random
from typing import Tuple

from .materials import MaterialBase

__all__ = ["resize", "random_resize", "crop", "center_crop", "random_crop", "tile", "flip_horizontal", "flip_vertical",
           "random_horizontal_flip", "random_vertical_flip", "roll", "invert_normal_map", "adjust_normal_strength", "to_linear", "to_srgb"]


def resize(material: MaterialBase, size: Tuple[int, int], antialias: bool = True) -> MaterialBase:
    return material.clone().resize(size=size, antialias=antialias)


def random_resize_size(min_size: int, max_size: int) -> Tuple[int, int]:
    """(height, width) as functional.py:87-88 draws them: height first."""
    height = int(min_size + (max_size - min_size) * random())
    width = int(min_size + (max_size - min_size) * random())
    return height, width


def random_resize(material: MaterialBase, min_size: int, max_size: int, antialias: bool = True) -> MaterialBase:
    new = material.clone()
    return new.resize(size=random_resize_size(min_size, max_size), antialias=antialias)


def crop(material: MaterialBase, top: int, left: int, height: int, width: int) -> MaterialBase:
    return material.clone().crop(top=top, left=left, height=height, width=width)


def center_crop_window(size: Tuple[int, int], crop_size: Tuple[int, int]) -> Tuple[int, int, int, int]:
    """(top, left, height, width) of functional.py:129-133."""
    height, width = size
    crop_height, crop_width = crop_size
    return (height - crop_height) // 2, (width - crop_width) // 2, crop_height, crop_width


def random_crop_window(size: Tuple[int, int], crop_size: Tuple[int, int]) -> Tuple[int, int, int, int]:
    """(top, left, height, width) as functional.py:149-152 draws them: top first."""
    height, width = size
    crop_height, crop_width = crop_size
    top = int((height - crop_height) * random())
    left = int((width - crop_width) * random())
    return top, left, crop_height, crop_width


def center_crop(material: MaterialBase, crop_size: Tuple[int, int]) -> MaterialBase:
    new = material.clone()
    top, left, height, width = center_crop_window(new.size, crop_size)
    return new.crop(top=top, left=left, height=height, width=width)


def random_crop(material: MaterialBase, crop_size: Tuple[int, int]) -> MaterialBase:
    new = material.clone()
    top, left, height, width = random_crop_window(new.size, crop_size)
    return new.crop(top=top, left=left, height=height, width=width)


def tile(material: MaterialBase, num_tiles: int) -> MaterialBase:
    return material.clone().tile(num_tiles=num_tiles)


def flip_horizontal(material: MaterialBase) -> MaterialBase:
    return material.clone().flip_horizontal()


def flip_vertical(material: MaterialBase) -> MaterialBase:
    return material.clone().flip_vertical()


def random_horizontal_flip(material: MaterialBase, p: float = 0.5) -> MaterialBase:
    new = material.clone()
    if random() < p:
        new.flip_horizontal()
    return new


def random_vertical_flip(material: MaterialBase, p: float = 0.5) -> MaterialBase:
    new = material.clone()
    if random() < p:
        new.flip_vertical()
    return new


def roll(material: MaterialBase, shift: Tuple[int, int]) -> MaterialBase:
    return material.clone().roll(shift=shift)


def invert_normal_map(material: MaterialBase) -> MaterialBase:
    return material.clone().invert_normal()


def adjust_normal_strength(material: MaterialBase, strength_factor: float) -> MaterialBase:
    return material.clone().adjust_normal_strength(strength_factor=strength_factor)


def to_linear(material: MaterialBase) -> MaterialBase:
    return material.clone().to_linear()


def to_srgb(material: MaterialBase) -> MaterialBase:
    return material.clone().to_srgb()
