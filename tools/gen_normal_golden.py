"""Writes tests/golden/normal_ops.npz: outputs of the REAL reference's normal-map operations (pypbr/utils/functions.py:69-177,
pypbr/materials/base.py:673-729), the fixture of tests/test_gpu_normal_ops.py.  Development container only: it imports the reference
through oracle/ref_import.import_reference() (nothing under oracle/ is changed).  Only float arrays are stored; the torch version and
the ATen thread count they were made with are stored as float arrays too (meta_torch as the version's bytes, meta_threads).

    python tools/gen_normal_golden.py [OUT_DIR]        (default: tests/golden)

Keys: in_<name> inputs; cnfh__<input>__<scale>__<convention>, rot__<input>__<angle>, str__<input>__<factor>, inv__<input> outputs;
chain__tiles (load tiles, resize(64), tile(2), compute_normal_from_height(3)); fresh__tiles (load tiles,
compute_normal_from_height(10) at once -- the height still as the PNG's 16-bit samples -- the top-left 96^2 of the result).
"""
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden")
CROP = 96
SCALES = (1.0, 2.5, 10.0)
ANGLES = (0.0, 30.0, 90.0, -45.0, 400.0)
FACTORS = (0.0, 0.5, 2.0, -1.0)
THREADS = 8


def _synthetic():
    g = torch.Generator().manual_seed(20261016)
    maps = {}
    for h, w in ((1, 1), (1, 17), (5, 1), (37, 53)):
        maps["h%dx%d" % (h, w)] = torch.rand(1, h, w, generator=g) * 2.0 - 0.5
        n = torch.cat([torch.rand(2, h, w, generator=g) * 2.0 - 1.0, torch.rand(1, h, w, generator=g) + 0.2])
        maps["n%dx%d" % (h, w)] = n / n.norm(dim=0, keepdim=True)
    return maps


def generate(out_dir: str) -> str:
    sys.path.insert(0, os.path.join(ROOT, "oracle"))
    from ref_import import import_reference
    import_reference()
    from pypbr.io import load_material_from_folder
    from pypbr.utils.functions import compute_normal_from_height, invert_normal, rotate_normals
    from pypbr.utils.enums import NormalConvention

    torch.set_num_threads(THREADS)
    z = {}
    heights, normals = {}, {}
    mat = load_material_from_folder(os.path.join(GOLDEN, "tiles"), preferred_workflow="metallic")
    heights["tiles"] = mat._maps["height"][:, :CROP, :CROP].contiguous()
    syn = _synthetic()
    heights.update({k: v for k, v in syn.items() if k.startswith("h")})
    normals.update({k: v for k, v in syn.items() if k.startswith("n")})
    for k, v in heights.items():
        z["in_height_" + k] = v
    for k, v in normals.items():
        z["in_normal_" + k] = v

    # every case on the synthetic maps; on the 96^2 crop one (each crop result is 110 KB: the file stays small)
    conventions = (("opengl", NormalConvention.OPENGL), ("directx", NormalConvention.DIRECTX))
    crop_cases = {"cnfh": {("tiles", 2.5, "opengl")}, "rot": set(), "str": set(), "inv": set()}

    def wanted(kind, *key):
        return key[0] != "tiles" or key in crop_cases[kind]
    for k, h in heights.items():
        for s in SCALES:
            for cname, conv in conventions:
                if wanted("cnfh", k, s, cname):
                    z["cnfh__%s__%g__%s" % (k, s, cname)] = compute_normal_from_height(h.clone(), s, convention=conv)
    for k, n in normals.items():
        for a in ANGLES:
            if wanted("rot", k, a):
                z["rot__%s__%g" % (k, a)] = rotate_normals(n.clone(), a)
        for f in FACTORS:
            if wanted("str", k, f):
                t = n.clone()                # base.py:689-706 on a bare map: normal[:2] *= f, F.normalize
                t[:2] *= f
                z["str__%s__%g" % (k, f)] = torch.nn.functional.normalize(t, dim=0)
        if wanted("inv", k):
            z["inv__" + k] = invert_normal(n.clone())

    mat = load_material_from_folder(os.path.join(GOLDEN, "tiles"), preferred_workflow="metallic")
    mat.resize(64).tile(2).compute_normal_from_height(3.0)
    z["chain__tiles"] = mat._maps["normal"]
    mat = load_material_from_folder(os.path.join(GOLDEN, "tiles"), preferred_workflow="metallic")
    mat.compute_normal_from_height(10.0)
    z["fresh__tiles"] = mat._maps["normal"][:, :CROP, :CROP]

    arrays = {k: np.ascontiguousarray(v.detach().numpy().astype(np.float32)) for k, v in z.items()}
    arrays["meta_torch"] = np.frombuffer(torch.__version__.encode().ljust(32, b"\0"), dtype=np.uint8).astype(np.float32)
    arrays["meta_threads"] = np.array([torch.get_num_threads()], dtype=np.float32)
    os.makedirs(out_dir, exist_ok=True)
    path = os.path.join(out_dir, "normal_ops.npz")
    np.savez_compressed(path, **arrays)
    return path


def meta(z) -> tuple:
    """(torch version, ATen threads) the file was generated with."""
    return bytes(z["meta_torch"].astype(np.uint8)).rstrip(b"\0").decode(), int(z["meta_threads"][0])


if __name__ == "__main__":
    p = generate(sys.argv[1] if len(sys.argv) > 1 else GOLDEN)
    print("%s: %d bytes" % (p, os.path.getsize(p)))
