"""Writes tests/golden/export.npz: what the REAL reference's MaterialBase.to_pil (pypbr/materials/base.py:793-850) and
io.save_material_to_folder (pypbr/io.py:189-230) make of seeded maps -- the fixture of tests/test_export_host.py and
tests/test_gpu_image_encode.py.  Development container only: it imports the reference through oracle/ref_import.import_reference()
(nothing under oracle/ is changed).

    python tools/gen_export_golden.py [OUT_DIR]        (default: tests/golden)

The stand-in torchvision module of oracle/ref_import.py has no `to_pil_image`, and torchvision is not installed where this runs, so the
tool hangs one onto sys.modules["torchvision.transforms.functional"] after the import: a restatement of torchvision's own for float
tensors -- pic.mul(255).byte(), transposed to (H,W,C), Image.fromarray (2-D for one channel) -- written from torchvision's source as
remembered, not checked against an installed copy.

Per size s = <H>x<W> of SIZES (a BasecolorMetallicMaterial on the CPU with albedo, normal, roughness, height, metallic):
  in__<map>__<s>        float32 inputs in [0, 1], a seeded uniform (not multiples of 1/255), for albedo, roughness, metallic, height
  nrm__<s>              the floats the reference's _maps["normal"] holds after its own processing: seeded unit normals given signed
                        (kept as they are, base.py:212) or, for the sizes of ENCODED_NORMALS, given as colours (decoded, base.py:216-217)
  pil8__<map>__<s>      np.array of to_pil()[map]: uint8 (H,W,3) / (H,W)
  pil16__height__<s>    np.array of to_pil({"height": "I;16"})["height"]: uint16 (H,W); every other map of that call equals pil8
  modes8 / modes16      the images' modes in dict order, the maps' names in `names`
For the size PNG_SIZE, through save_material_to_folder:
  files__default / files__override / files__jpg   the sorted file names written (override: OVERRIDE; jpg: format="jpg")
  png__<map>            the samples of the PNGs it wrote, read back
`restate` below is the numpy fp32 restatement of the operation order that the tests use as their host oracle; the tool asserts that it
reproduces every sample array it stores."""
import os
import sys
import tempfile

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden")
SIZES = ((1, 1), (1, 17), (5, 1), (37, 53), (24, 256))
ENCODED_NORMALS = ((1, 17), (37, 53))
PNG_SIZE = (37, 53)
OVERRIDE = {"albedo": "basecolor", "height": "displacement"}
FLOAT_MAPS = (("albedo", 3), ("roughness", 1), ("height", 1), ("metallic", 1))
SIXTEEN = ("I", "I;16", "I;16B", "I;16L", "I;16N")


def restate(t, bits: int = 8, normal: bool = False) -> np.ndarray:
    """(C,H,W) floats -> the (H,W,C) samples of MaterialBase.to_pil, every product and sum an fp32 operation of its own:
    [(v + 1.0) * 0.5 for a normal map,] v * 255 | 65535, truncated toward zero.  Outside [0, 1], where upstream is undefined, the rule
    of this build: saturate, NaN -> 0."""
    v = np.asarray(t, dtype=np.float32)
    assert v.ndim == 3, v.shape
    top = np.float32(255.0 if bits == 8 else 65535.0)
    with np.errstate(invalid="ignore", over="ignore"):
        if normal:
            v = (v + np.float32(1.0)) * np.float32(0.5)
        p = v * top
        assert p.dtype == np.float32
        p = np.clip(np.where(np.isnan(p), np.float32(0.0), p), np.float32(0.0), top)
    return np.ascontiguousarray(p.astype(np.uint8 if bits == 8 else np.uint16).transpose(1, 2, 0))


def size_key(h, w):
    return "%dx%d" % (h, w)


def inputs():
    """name__size -> seeded float32 tensors: uniform maps in [0, 1] and unit normals (one component forced negative, so that the
    reference keeps a signed map as it is)."""
    g = torch.Generator().manual_seed(20261018)
    out = {}
    for h, w in SIZES:
        s = size_key(h, w)
        for name, c in FLOAT_MAPS:
            out["%s__%s" % (name, s)] = torch.rand(c, h, w, generator=g)
        n = torch.randn(3, h, w, generator=g)
        n = n / n.norm(dim=0, keepdim=True)
        n[0, 0, 0] = -n[0, 0, 0].abs() - 1e-3
        n = n / n.norm(dim=0, keepdim=True)
        out["normal__" + s] = n
    return out


def _to_pil_image(pic, mode=None):
    """torchvision.transforms.functional.to_pil_image for a float (C,H,W) tensor, restated."""
    from PIL import Image
    arr = pic.mul(255).byte().numpy().transpose(1, 2, 0)
    if arr.shape[2] == 1:
        return Image.fromarray(np.ascontiguousarray(arr[:, :, 0]))
    return Image.fromarray(np.ascontiguousarray(arr))


def _strings(items):
    return np.array(list(items), dtype=np.str_)


def generate(out_dir: str) -> str:
    sys.path.insert(0, os.path.join(ROOT, "oracle"))
    from ref_import import import_reference
    import_reference()
    sys.modules["torchvision.transforms.functional"].to_pil_image = _to_pil_image
    from PIL import Image
    from pypbr.io import save_material_to_folder
    from pypbr.materials import BasecolorMetallicMaterial

    z, src = {}, inputs()
    modes8 = modes16 = names = None
    for h, w in SIZES:
        s = size_key(h, w)
        normal = src["normal__" + s]
        given = (normal + 1.0) * 0.5 if (h, w) in ENCODED_NORMALS else normal
        mat = BasecolorMetallicMaterial(albedo=src["albedo__" + s].clone(), normal=given.clone(), roughness=src["roughness__" + s].clone(),
                                        metallic=src["metallic__" + s].clone(), height=src["height__" + s].clone())
        for name, _ in FLOAT_MAPS:
            assert torch.equal(mat._maps[name], src["%s__%s" % (name, s)]), name
            z["in__%s__%s" % (name, s)] = src["%s__%s" % (name, s)].numpy()
        held = mat._maps["normal"].clone()
        assert float(held.min()) < 0
        z["nrm__" + s] = held.numpy()
        plain, deep = mat.to_pil(), mat.to_pil({"height": "I;16"})
        assert list(plain) == list(deep) == list(mat._maps)
        names = list(plain)
        modes8, modes16 = [im.mode for im in plain.values()], [im.mode for im in deep.values()]
        for name, im in plain.items():
            a = np.array(im)
            assert a.dtype == np.uint8 and im.size == (w, h)
            floats = held if name == "normal" else mat._maps[name]
            want = restate(floats.numpy(), 8, name == "normal")
            assert np.array_equal(a.reshape(want.shape), want), (s, name)
            z["pil8__%s__%s" % (name, s)] = a
            if name != "height":
                assert np.array_equal(np.array(deep[name]), a), (s, name)
        a = np.array(deep["height"])
        assert a.dtype == np.uint16 and a.shape == (h, w)
        assert np.array_equal(a[:, :, None], restate(mat._maps["height"].numpy(), 16)), s
        z["pil16__height__" + s] = a
        if (h, w) == PNG_SIZE:
            with tempfile.TemporaryDirectory() as tmp:
                for tag, kw in (("default", {}), ("override", {"map_names": OVERRIDE}), ("jpg", {"format": "jpg"})):
                    folder = os.path.join(tmp, tag)
                    save_material_to_folder(mat, folder, **kw)
                    z["files__" + tag] = _strings(sorted(os.listdir(folder)))
                for name in names:
                    with Image.open(os.path.join(tmp, "default", name + ".png")) as im:
                        z["png__" + name] = np.array(im)
                    assert np.array_equal(z["png__" + name], z["pil8__%s__%s" % (name, s)]), name
    z["names"], z["modes8"], z["modes16"] = _strings(names), _strings(modes8), _strings(modes16)
    z["meta_torch"] = _strings([torch.__version__])
    os.makedirs(out_dir, exist_ok=True)
    path = os.path.join(out_dir, "export.npz")
    np.savez_compressed(path, **z)
    assert os.path.getsize(path) < 2 ** 20, os.path.getsize(path)
    return path


if __name__ == "__main__":
    p = generate(sys.argv[1] if len(sys.argv) > 1 else GOLDEN)
    print("%s: %d bytes" % (p, os.path.getsize(p)))
    g = np.load(p)
    print("names %s  modes8 %s  modes16 %s" % (list(g["names"]), list(g["modes8"]), list(g["modes16"])))
    for tag in ("default", "override", "jpg"):
        print("files %-8s %s" % (tag, list(g["files__" + tag])))
