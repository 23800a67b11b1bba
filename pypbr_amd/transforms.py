"""pypbr.transforms for the MI355X build: upstream's transform classes (pypbr/transforms/transforms.py) and, as `transforms.functional`,
their functional forms -- all but the rotate family (`Rotate`, `RandomRotate`, `rotate`, `random_rotate`), which is built in a module
of its own and not re-exported here: the names stay absent from this module as an absent module's would be, and a
`Rotate` instance from that module is an ordinary callable to `Compose`.

Every transform takes a material and returns a new one.  `Compose` does what upstream's does -- each stage applied to the previous
stage's result -- but a maximal run of GEOMETRIC stages (`Crop`, `CenterCrop`, `RandomCrop`, `FlipHorizontal`, `FlipVertical`,
`RandomHorizontalFlip`, `RandomVerticalFlip`, `Roll`, `Tile`) is an index map per axis (functional.PlaneMap): the run is
folded on the host into as few maps as the rules allow -- one, unless a roll or a tile follows a crop to a non-multiple -- and each map
is ONE pbr_remap_planes launch per block of maps, with no clone per stage.  The random stages still draw
stage by stage, in order, so `random.seed(k)` fixes the same choices fused and unfused, and the results are bit-equal.
"""
from typing import Callable, List, Tuple

from . import _transforms_functional as functional
from .materials import MaterialBase

__all__ = ["functional", "Compose", "Resize", "RandomResize", "Crop", "CenterCrop", "RandomCrop", "Tile", "FlipHorizontal", "FlipVertical",
           "RandomHorizontalFlip", "RandomVerticalFlip", "Roll", "InvertNormal", "AdjustNormalStrength", "ToLinear", "ToSrgb"]


class Resize:
    def __init__(self, size: Tuple[int, int], antialias: bool = True):
        self.size, self.antialias = size, antialias

    def __call__(self, material: MaterialBase) -> MaterialBase:
        return functional.resize(material, size=self.size, antialias=self.antialias)


class RandomResize:
    def __init__(self, min_size: int, max_size: int, antialias: bool = True):
        self.min_size, self.max_size, self.antialias = min_size, max_size, antialias

    def __call__(self, material: MaterialBase) -> MaterialBase:
        return functional.random_resize(material, min_size=self.min_size, max_size=self.max_size, antialias=self.antialias)


class Crop:
    def __init__(self, top: int, left: int, height: int, width: int):
        self.top, self.left, self.height, self.width = top, left, height, width

    def __call__(self, material: MaterialBase) -> MaterialBase:
        return functional.crop(material, top=self.top, left=self.left, height=self.height, width=self.width)

    def _stage(self, size):
        return ("crop", self.top, self.left, self.height, self.width)


class CenterCrop:
    def __init__(self, height: int, width: int):
        self.height, self.width = height, width

    def __call__(self, material: MaterialBase) -> MaterialBase:
        return functional.center_crop(material, crop_size=(self.height, self.width))

    def _stage(self, size):
        return ("crop",) + functional.center_crop_window(size, (self.height, self.width))


class RandomCrop:
    def __init__(self, height: int, width: int):
        self.height, self.width = height, width

    def __call__(self, material: MaterialBase) -> MaterialBase:
        return functional.random_crop(material, crop_size=(self.height, self.width))

    def _stage(self, size):
        return ("crop",) + functional.random_crop_window(size, (self.height, self.width))


class Tile:
    def __init__(self, num_tiles: int):
        self.num_tiles = num_tiles

    def __call__(self, material: MaterialBase) -> MaterialBase:
        return functional.tile(material, num_tiles=self.num_tiles)

    def _stage(self, size):
        return ("tile", self.num_tiles, self.num_tiles)


class FlipHorizontal:
    def __call__(self, material: MaterialBase) -> MaterialBase:
        return functional.flip_horizontal(material)

    def _stage(self, size):
        return ("flip_h",)


class FlipVertical:
    def __call__(self, material: MaterialBase) -> MaterialBase:
        return functional.flip_vertical(material)

    def _stage(self, size):
        return ("flip_v",)


class RandomHorizontalFlip:
    def __call__(self, material: MaterialBase, p: float = 0.5) -> MaterialBase:
        return functional.random_horizontal_flip(material, p)

    def _stage(self, size, p: float = 0.5):
        return ("flip_h",) if functional.random() < p else None


class RandomVerticalFlip:
    def __call__(self, material: MaterialBase, p: float = 0.5) -> MaterialBase:
        return functional.random_vertical_flip(material, p)

    def _stage(self, size, p: float = 0.5):
        return ("flip_v",) if functional.random() < p else None


class Roll:
    def __init__(self, shift: Tuple[int, int]):
        self.shift = shift

    def __call__(self, material: MaterialBase) -> MaterialBase:
        return functional.roll(material, shift=self.shift)

    def _stage(self, size):
        dy, dx = self.shift
        return ("roll", int(dy), int(dx))


class InvertNormal:
    def __call__(self, material: MaterialBase) -> MaterialBase:
        return functional.invert_normal_map(material)


class AdjustNormalStrength:
    def __init__(self, strength_factor: float):
        self.strength_factor = strength_factor

    def __call__(self, material: MaterialBase) -> MaterialBase:
        return functional.adjust_normal_strength(material, strength_factor=self.strength_factor)


class ToLinear:
    def __call__(self, material: MaterialBase) -> MaterialBase:
        return functional.to_linear(material)


class ToSrgb:
    def __call__(self, material: MaterialBase) -> MaterialBase:
        return functional.to_srgb(material)


_GEOMETRIC = (Crop, CenterCrop, RandomCrop, Tile, FlipHorizontal, FlipVertical, RandomHorizontalFlip, RandomVerticalFlip, Roll)


def _fusable(transform) -> bool:
    """The geometric classes themselves (a subclass may override __call__), and a Tile upstream would not turn into empty maps."""
    if type(transform) not in _GEOMETRIC:
        return False
    return not isinstance(transform, Tile) or (isinstance(transform.num_tiles, int) and transform.num_tiles >= 1)


def _size_after(size, stage):
    if stage[0] == "crop":
        return int(stage[3]), int(stage[4])
    if stage[0] == "tile":
        return size[0] * stage[1], size[1] * stage[2]
    return size


class Compose:
    """Upstream's Compose (transforms.py:33-56) with runs of geometric stages fused; `fuse=False` applies every stage on its own, as
    upstream does (what the tests compare the fused form against)."""

    def __init__(self, transforms: List[Callable], fuse: bool = True):
        self.transforms = transforms
        self.fuse = fuse

    def __call__(self, material: MaterialBase) -> MaterialBase:
        run = []
        for transform in self.transforms:
            if self.fuse and isinstance(material, MaterialBase) and _fusable(transform):
                run.append(transform)
                continue
            material = transform(self._geometric_run(material, run))
            run = []
        return self._geometric_run(material, run)

    @staticmethod
    def _resolve(size, run) -> list:
        """The stages (functional.fold_stages) of a run of geometric transforms on a material of `size`, resolved in order: CenterCrop /
        RandomCrop see the size the stages before them leave, the random stages draw here, a crop outside the map raises.  Host only."""
        from .functional import check_crop
        stages = []
        for transform in run:
            stage = transform._stage(size)
            if stage is not None:
                if stage[0] == "crop":
                    check_crop(size, *stage[1:])
                stages.append(stage)
                size = _size_after(size, stage)
        return stages

    @staticmethod
    def _geometric_run(material, run):
        """A run as one index map: resolved and folded on the host, launched once per block of maps; the input material keeps its maps."""
        if not run:
            return material
        if len(run) == 1 or material.size is None:
            for transform in run:
                material = transform(material)
            return material
        return material._shallow()._geometry(Compose._resolve(material.size, run), fresh=True)
