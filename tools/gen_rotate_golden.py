"""Writes tests/golden/rotate.npz: outputs of the REAL reference's MaterialBase.rotate (pypbr/materials/base.py:539-603, with
utils.rotate_normals on the normal map) -- the fixture of tests/test_gpu_rotation.py and tests/test_rotation_host.py.  Development
container only: it imports the reference through oracle/ref_import.import_reference() (nothing under oracle/ is changed).

The reference rotates through torchvision.transforms.functional.rotate and center_crop, and the import stand-in for torchvision has
neither: this tool adds tools/rotate_oracle.py's restatements of the two to the stand-in module after import_reference().  So the
sampling is that restatement's (torchvision itself is installed nowhere here: rotate_oracle.py's header); the target size, the padding,
the order of the steps and the rotation of the normal vectors are the reference's own code.

Only float arrays are stored; the torch version and the ATen thread count they were made with are stored as float arrays too (meta_torch
as the version's bytes, meta_threads).  The colour and roughness maps hold multiples of 1/255 so that the file compresses well.

    python tools/gen_rotate_golden.py [OUT_DIR]        (default: tests/golden)

Keys: in__<h>x<w>__<map> inputs; out__<case>__<map> outputs and band__<case> (1.0 where the pixel lies in the tie band, see `band`) for
every case of CASES; random__<seed> the angle RandomRotate draws after random.seed(seed) and out__random<seed>__<map> what it leaves.

The tie band: a pixel whose sampling coordinate lies within BAND_ULPS * 2^-24 * max(Hp, Wp) pixel of a half-integer, on either axis, may
round to either neighbour in two correct fp32 implementations (the coordinate passes about six fp32 roundings at magnitudes below 4,
scaled by size / 2: about 5.5 * 2^-24 * size each, and two implementations may differ by twice that).  STRICT angles must keep at most
1 % of a case's pixels in the band and TIE angles at most 10 %; `check_band_caps` asserts it for every case the tests run, here and in
the host suite.  A case that exceeds its cap gets another angle or size, never a wider allowance.
"""
import os
import random
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden")
THREADS = 8
MAPS = ("albedo", "normal", "roughness")
SIZES = ((8, 8), (13, 9), (16, 24), (33, 47), (64, 64))
STRICT = (0.0, 17.0, 33.3, -71.5, 90.0, 123.4, 180.0, 270.0, 360.0)
TIES = (45.0, -30.0)
TIE_SIZES = ((13, 9), (16, 24), (64, 64))
MODES = ("constant", "circular")
BAND_ULPS = 16
STRICT_CAP, TIE_CAP = 0.01, 0.10
SEEDS = (0, 1, 2)
RANDOM_SIZE, RANDOM_RANGE = (13, 9), (-40.0, 200.0)


def case_name(h, w, angle, expand, mode):
    return "%dx%d__%g__%s__%s" % (h, w, angle, "expand" if expand else "same", mode)


def fits(h, w, angle, expand, mode) -> bool:
    """Can upstream run the case at all?  (circular padding wider than the map: F.pad raises)"""
    sys.path.insert(0, ROOT)
    from pypbr_amd import functional as F
    try:
        F.rotate_plan(h, w, angle, expand, mode)
    except ValueError:
        return False
    return True


def matrix():
    """Every (h, w, angle, expand, mode, strict) the GPU tests run: the sizes x the strict angles, the tie sizes x the tie angles."""
    out = []
    for h, w in SIZES:
        for angle in STRICT + (TIES if (h, w) in TIE_SIZES else ()):
            for expand in (False, True):
                for mode in MODES:
                    if fits(h, w, angle, expand, mode):
                        out.append((h, w, angle, expand, mode, angle in STRICT))
    return out


def _golden_cases():
    """The part of the matrix whose outputs are stored (the file stays a few hundred KB): every angle at 13x9, a few at the others, 180
    degrees of 64x64 expanded (upstream's 65x65)."""
    keep = []
    for h, w, angle, expand, mode, strict in matrix():
        if (h, w) == (13, 9) and (not expand or angle in (17.0, 90.0, 180.0, 45.0)):
            keep.append((h, w, angle, expand, mode))
        elif (h, w) == (8, 8) and angle in (33.3, 90.0):
            keep.append((h, w, angle, expand, mode))
        elif (h, w) == (16, 24) and ((angle in (17.0, -71.5, 45.0) and not expand) or (angle == 123.4 and expand)):
            keep.append((h, w, angle, expand, mode))
        elif (h, w) == (33, 47) and ((angle == 33.3 and not expand and mode == "constant") or (angle == 270.0 and not expand and mode == "circular")):
            keep.append((h, w, angle, expand, mode))
        elif (h, w) == (64, 64) and angle == 180.0 and expand and mode == "constant":
            keep.append((h, w, angle, expand, mode))
    return keep


CASES = {case_name(*c): c for c in _golden_cases()}


def coordinates(plan):
    """The sampling coordinates (fx, fy) of every output pixel in float64, from the plan's fp32 matrix entries: (H, W) tensors."""
    f64 = torch.float64
    x = torch.arange(plan.W, dtype=f64)[None, :] + plan.x0
    y = torch.arange(plan.H, dtype=f64)[:, None] + plan.y0
    gx, gy = x * plan.t00 + y * plan.t10, x * plan.t01 + y * plan.t11
    return ((gx + 1) * plan.Wp - 1) / 2, ((gy + 1) * plan.Hp - 1) / 2


def band(plan):
    """(on x, on y): bool (H, W) tensors, True where the coordinate lies within the guard distance of a half-integer."""
    guard = BAND_ULPS * 2.0 ** -24 * max(plan.Hp, plan.Wp)
    fx, fy = coordinates(plan)
    return tuple((f - torch.floor(f) - 0.5).abs() < guard for f in (fx, fy))


def _unpad(plan, ix, iy):
    inside = (ix >= 0) & (ix < plan.Wp) & (iy >= 0) & (iy < plan.Hp)
    sx, sy = ix - plan.pad, iy - plan.pad
    if plan.circular:
        sx, sy = sx % plan.w, sy % plan.h
    else:
        inside &= (sx >= 0) & (sx < plan.w) & (sy >= 0) & (sy < plan.h)
    return torch.where(inside, sy * plan.w + sx, torch.full_like(sx, -1))


def candidates(plan):
    """The source offsets (-1: fill) a correct implementation may pick per output pixel: four (H, W) int64 tensors -- the texels on either
    side of a tie on x, times either side of a tie on y; outside the band all four are the one nearest texel."""
    fx, fy = coordinates(plan)
    bx, by = band(plan)
    lo_x = torch.where(bx, torch.floor(fx), torch.round(fx)).long()
    lo_y = torch.where(by, torch.floor(fy), torch.round(fy)).long()
    hi_x, hi_y = lo_x + bx.long(), lo_y + by.long()
    return [_unpad(plan, ix, iy) for iy in (lo_y, hi_y) for ix in (lo_x, hi_x)]


def check_band_caps():
    """The two conditions of the module docstring over the whole test matrix; returns the largest shares found."""
    sys.path.insert(0, ROOT)
    from pypbr_amd import functional as F
    worst = {True: 0.0, False: 0.0}
    for h, w, angle, expand, mode, strict in matrix():
        bx, by = band(F.rotate_plan(h, w, angle, expand, mode))
        share = float((bx | by).float().mean())
        cap = STRICT_CAP if strict else TIE_CAP
        assert share <= cap, "%s: %.4f of the pixels lie in the tie band (cap %.2f): choose another angle or size" % (
            case_name(h, w, angle, expand, mode), share, cap)
        worst[strict] = max(worst[strict], share)
    return worst[True], worst[False]


def inputs():
    g = torch.Generator().manual_seed(20261018)
    maps = {}
    for h, w in SIZES:
        n = torch.cat([torch.rand(2, h, w, generator=g) * 2.0 - 1.0, torch.rand(1, h, w, generator=g) + 0.2])
        maps["%dx%d" % (h, w)] = {"albedo": torch.randint(1, 256, (3, h, w), generator=g).float() / 255.0,
                                  "normal": n / n.norm(dim=0, keepdim=True),
                                  "roughness": torch.randint(1, 256, (1, h, w), generator=g).float() / 255.0}
    return maps


def generate(out_dir: str) -> str:
    sys.path.insert(0, os.path.join(ROOT, "oracle"))
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    sys.path.insert(0, ROOT)
    from ref_import import import_reference
    import_reference()
    import rotate_oracle
    import torchvision.transforms.functional as TF          # the in-memory stand-in
    TF.rotate, TF.center_crop = rotate_oracle.rotate, rotate_oracle.center_crop
    from pypbr.materials import BasecolorMetallicMaterial
    from pypbr.transforms import RandomRotate
    from pypbr_amd import functional as F

    torch.set_num_threads(THREADS)
    strict_share, tie_share = check_band_caps()
    print("tie band: at most %.4f of a strict case's pixels, %.4f of a tie case's" % (strict_share, tie_share))
    z = {}
    ins = inputs()
    for size, maps in ins.items():
        for k, v in maps.items():
            z["in__%s__%s" % (size, k)] = v

    def material(size):
        return BasecolorMetallicMaterial(**{k: v.clone() for k, v in ins[size].items()})
    for name, (h, w, angle, expand, mode) in CASES.items():
        mat = material("%dx%d" % (h, w))
        assert mat.rotate(angle, expand=expand, padding_mode=mode) is mat
        for k in MAPS:
            z["out__%s__%s" % (name, k)] = mat._maps[k]
        bx, by = band(F.rotate_plan(h, w, angle, expand, mode))
        z["band__" + name] = (bx | by).float()
    for seed in SEEDS:
        random.seed(seed)
        angle = RANDOM_RANGE[0] + (RANDOM_RANGE[1] - RANDOM_RANGE[0]) * random.random()
        random.seed(seed)
        out = RandomRotate(*RANDOM_RANGE)(material("%dx%d" % RANDOM_SIZE))
        z["random__%d" % seed] = torch.tensor([angle], dtype=torch.float64)
        for k in MAPS:
            z["out__random%d__%s" % (seed, k)] = out._maps[k]

    arrays = {k: np.ascontiguousarray(v.detach().numpy()) for k, v in z.items()}
    arrays = {k: (v if v.dtype == np.float64 else v.astype(np.float32)) for k, v in arrays.items()}
    arrays["meta_torch"] = np.frombuffer(torch.__version__.encode().ljust(32, b"\0"), dtype=np.uint8).astype(np.float32)
    arrays["meta_threads"] = np.array([torch.get_num_threads()], dtype=np.float32)
    os.makedirs(out_dir, exist_ok=True)
    path = os.path.join(out_dir, "rotate.npz")
    np.savez_compressed(path, **arrays)
    return path


def meta(z) -> tuple:
    """(torch version, ATen threads) the file was generated with."""
    return bytes(z["meta_torch"].astype(np.uint8)).rstrip(b"\0").decode(), int(z["meta_threads"][0])


if __name__ == "__main__":
    p = generate(sys.argv[1] if len(sys.argv) > 1 else GOLDEN)
    print("%s: %d bytes, %d cases" % (p, os.path.getsize(p), len(CASES)))
