"""Writes tests/golden/geometry.npz: outputs of the REAL reference's geometric material transforms -- MaterialBase.flip_horizontal,
flip_vertical, roll, tile and crop (pypbr/materials/base.py:506-537, :605-655), chains of them, and what pypbr.transforms' RandomCrop,
RandomHorizontalFlip and RandomVerticalFlip produce after random.seed(k) -- the fixture of tests/test_gpu_geometry.py and
tests/test_geometry_host.py.  Development container only: it imports the reference through oracle/ref_import.import_reference()
(nothing under oracle/ is changed).

The reference crops through torchvision.transforms.functional.crop, and the import stand-in for torchvision has no `crop`: this tool adds
one to the stand-in module after import_reference() -- an in-bounds slice, img[..., top:top + height, left:left + width], which is what
torchvision does for a window inside a tensor.  So the VALUES of every crop are this tool's restatement; which window is cropped (the
random draws included), the flips with their sign changes, roll and tile are the reference's own code.

Only float arrays are stored; the torch version and the ATen thread count they were made with are stored as float arrays too (meta_torch
as the version's bytes, meta_threads).  The synthetic maps hold multiples of 1/255 so that the file compresses to a few hundred KB.

    python tools/gen_geometry_golden.py [OUT_DIR]        (default: tests/golden)

Keys: in__<material>__<map> inputs, out__<case>__<map> outputs; CASES below says what each case runs on which material.
"""
import os
import random
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden")
CROP = 96
THREADS = 8
MAPS = ("albedo", "normal", "roughness", "metallic", "height")
SIZES = ((1, 1), (1, 17), (5, 1), (37, 53))
WINDOWS = {"1x1": (0, 0, 1, 1), "1x17": (0, 3, 1, 9), "5x1": (1, 0, 3, 1), "37x53": (5, 9, 20, 31)}
SEEDS = (0, 1, 2, 3)
RANDOM_CROP = (11, 13)


def _cases():
    """case -> (material, stages): ("flip_h",) | ("flip_v",) | ("crop", top, left, height, width) | ("roll", dy, dx) | ("tile", n, n), or
    one ("random", seed): Compose([RandomCrop(*RANDOM_CROP), RandomHorizontalFlip(), RandomVerticalFlip()]) after random.seed(seed)."""
    cases = {}
    for h, w in SIZES:
        m = "%dx%d" % (h, w)
        win = WINDOWS[m]
        cases[m + "__flip_h"] = (m, [("flip_h",)])
        cases[m + "__flip_v"] = (m, [("flip_v",)])
        cases[m + "__roll"] = (m, [("roll", -3, w + 5)])
        cases[m + "__crop"] = (m, [("crop",) + win])
        cases[m + "__chain_a"] = (m, [("flip_h",), ("roll", 2, 3), ("flip_v",), ("crop",) + win])
        if (h, w) != (37, 53):
            cases[m + "__tile"] = (m, [("tile", 2, 2)])
            cases[m + "__chain_t"] = (m, [("roll", 1, 1), ("tile", 3, 3), ("flip_h",), ("roll", 2, -1)])
    cases["37x53__chain_b"] = ("37x53", [("crop", 4, 6, 10, 12), ("tile", 2, 2), ("roll", 7, -5), ("flip_h",)])
    cases["37x53__chain_c"] = ("37x53", [("flip_v",), ("crop", 0, 0, 7, 9), ("roll", 3, 4), ("tile", 2, 2)])      # a roll that does not fold
    for k in SEEDS:
        cases["37x53__random%d" % k] = ("37x53", [("random", k)])
    cases["tiles__flip_v"] = ("tiles", [("flip_v",)])
    cases["tiles__chain_d"] = ("tiles", [("roll", 10, -20), ("flip_h",), ("crop", 16, 8, 48, 64)])
    return cases


CASES = _cases()


def _synthetic():
    g = torch.Generator().manual_seed(20261017)
    mats = {}

    def q(*shape):
        return torch.randint(0, 256, shape, generator=g).to(torch.float32) / 255.0
    for h, w in SIZES:
        normal = q(3, h, w) * 2.0 - 1.0
        normal[0, 0, 0] = -1.0                       # signed: the reference keeps the map as it is (base.py:212)
        mats["%dx%d" % (h, w)] = {"albedo": q(3, h, w), "normal": normal, "roughness": q(1, h, w), "metallic": q(1, h, w), "height": q(1, h, w)}
    return mats


def apply_stages(material, stages, transforms=None):
    """Runs a case's stages through a material's own methods (the reference's, or this package's: the same names)."""
    for st in stages:
        if st[0] == "flip_h":
            material.flip_horizontal()
        elif st[0] == "flip_v":
            material.flip_vertical()
        elif st[0] == "crop":
            material.crop(*st[1:])
        elif st[0] == "roll":
            material.roll((st[1], st[2]))
        elif st[0] == "tile":
            material.tile(st[1])
        elif st[0] == "random":
            random.seed(st[1])
            material = transforms.Compose([transforms.RandomCrop(*RANDOM_CROP), transforms.RandomHorizontalFlip(),
                                           transforms.RandomVerticalFlip()])(material)
        else:
            raise ValueError(st)
    return material


def generate(out_dir: str) -> str:
    sys.path.insert(0, os.path.join(ROOT, "oracle"))
    from ref_import import import_reference
    import_reference()
    sys.modules["torchvision.transforms.functional"].crop = lambda img, top, left, height, width: img[..., top:top + height, left:left + width]
    from pypbr import transforms
    from pypbr.io import load_material_from_folder
    from pypbr.materials import BasecolorMetallicMaterial

    torch.set_num_threads(THREADS)
    inputs = _synthetic()
    mat = load_material_from_folder(os.path.join(GOLDEN, "tiles"), preferred_workflow="metallic")
    inputs["tiles"] = {k: mat._maps[k][:, :CROP, :CROP].contiguous().clone() for k in MAPS}
    z = {}
    for m, maps in inputs.items():
        for k, v in maps.items():
            z["in__%s__%s" % (m, k)] = v
    for case, (m, stages) in CASES.items():
        material = BasecolorMetallicMaterial(**{k: v.clone() for k, v in inputs[m].items()})
        material = apply_stages(material, stages, transforms)
        for k in MAPS:
            z["out__%s__%s" % (case, k)] = material._maps[k]

    arrays = {k: np.ascontiguousarray(v.detach().numpy().astype(np.float32)) for k, v in z.items()}
    arrays["meta_torch"] = np.frombuffer(torch.__version__.encode().ljust(32, b"\0"), dtype=np.uint8).astype(np.float32)
    arrays["meta_threads"] = np.array([torch.get_num_threads()], dtype=np.float32)
    os.makedirs(out_dir, exist_ok=True)
    path = os.path.join(out_dir, "geometry.npz")
    np.savez_compressed(path, **arrays)
    return path


def meta(z) -> tuple:
    """(torch version, ATen threads) the file was generated with."""
    return bytes(z["meta_torch"].astype(np.uint8)).rstrip(b"\0").decode(), int(z["meta_threads"][0])


if __name__ == "__main__":
    p = generate(sys.argv[1] if len(sys.argv) > 1 else GOLDEN)
    print("%s: %d bytes" % (p, os.path.getsize(p)))
