"""Material export on the host side (no GPU): the C ABI declares and exports pbr_pack_images (ABI still 9) and returns every caller-error
code before any device work; the numpy restatement of the operation order (tools/gen_export_golden.restate, the GPU tests' host oracle)
reproduces every array of tests/golden/export.npz, which is what the real reference makes; a CPU-home material whose maps are still an
image's samples hands them back with upstream's modes and no device; io.save_material_to_folder names its files as upstream does."""
import ctypes
import os
import subprocess
import sys

import numpy as np
import pytest
import torch
from PIL import Image

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
import gen_export_golden as G  # noqa: E402

import abi_header  # noqa: E402
from pypbr_amd import _native as N  # noqa: E402
from pypbr_amd import functional as F  # noqa: E402
from pypbr_amd import io as pio  # noqa: E402
from pypbr_amd import materials as M  # noqa: E402

GOLD = np.load(os.path.join(ROOT, "tests", "golden", "export.npz"))
H, W = 48, 52


def test_header_declares_and_library_exports_the_entry_point():
    raw, text = abi_header.RAW, abi_header.TEXT
    assert "pbr_image_pack;" in text and "#define PBR_MAX_IMAGE_PACKS 8" in raw and N.MAX_IMAGE_PACKS == 8
    assert N.ABI_VERSION == 9 and "#define PBR_HIP_ABI_VERSION 9" in raw
    lib = N.lib()
    assert lib.pbr_abi_version() == 9
    assert lib.pbr_pack_images is not None
    assert ctypes.sizeof(N.ImagePack) == 56                      # 2 pointers, 3 x int64, 4 x int32
    assert F.pack_image is not None and F.download_samples is not None


def test_restatement_reproduces_every_array_of_the_golden_file():
    assert list(GOLD["names"]) == ["albedo", "normal", "roughness", "height", "metallic"]
    assert list(GOLD["modes8"]) == ["RGB", "RGB", "L", "L", "L"] and list(GOLD["modes16"]) == ["RGB", "RGB", "L", "I;16", "L"]
    checked = 0
    for h, w in G.SIZES:
        s = G.size_key(h, w)
        for name in GOLD["names"]:
            floats = GOLD["nrm__" + s] if name == "normal" else GOLD["in__%s__%s" % (name, s)]
            assert floats.dtype == np.float32 and floats.shape[1:] == (h, w)
            want = GOLD["pil8__%s__%s" % (name, s)]
            got = G.restate(floats, 8, name == "normal")
            assert want.dtype == np.uint8 and np.array_equal(got.reshape(want.shape), want), (s, name)
            checked += 1
        want = GOLD["pil16__height__" + s]
        assert want.dtype == np.uint16 and np.array_equal(G.restate(GOLD["in__height__" + s], 16)[:, :, 0], want), s
        n = GOLD["nrm__" + s]
        assert n.min() < 0 and np.allclose((n.astype(np.float64) ** 2).sum(0), 1.0, atol=1e-5)
        # the inputs are off the 1/255 grid, so truncation (not a round trip) is what the arrays pin
        a = GOLD["in__albedo__" + s]
        assert not np.array_equal(np.round(a * 255) / 255, a)
    s = G.size_key(*G.PNG_SIZE)
    for name in GOLD["names"]:
        assert np.array_equal(GOLD["png__" + name], GOLD["pil8__%s__%s" % (name, s)]), name
    assert checked == 25 and os.path.getsize(os.path.join(ROOT, "tests", "golden", "export.npz")) < (1 << 20)


def test_restatement_saturates_and_sends_nan_to_zero():
    v = np.array([-0.0, -1e-7, np.nextafter(np.float32(1), np.float32(2)), 2.0, 1e30, np.inf, -np.inf, np.nan, 1e-40, 0.5],
                 dtype=np.float32).reshape(1, 1, -1)
    assert G.restate(v, 8).reshape(-1).tolist() == [0, 0, 255, 255, 255, 255, 0, 0, 0, 127]
    assert G.restate(v, 16).reshape(-1).tolist() == [0, 0, 65535, 65535, 65535, 65535, 0, 0, 0, 32767]
    k8, k16 = np.arange(256, dtype=np.float32), np.arange(65536, dtype=np.float32)
    assert np.array_equal(G.restate((k8 / np.float32(255)).reshape(1, 1, -1), 8).reshape(-1), np.arange(256))
    assert np.array_equal(G.restate((k16 / np.float32(65535)).reshape(1, 1, -1), 16).reshape(-1), np.arange(65536))


def test_golden_file_is_what_the_reference_makes(tmp_path):
    sys.path.insert(0, os.path.join(ROOT, "oracle"))
    from ref_import import reference_available
    if not reference_available():
        pytest.skip("the reference tree is not on this machine")
    out = subprocess.run([sys.executable, "-W", "ignore", os.path.join(ROOT, "tools", "gen_export_golden.py"), str(tmp_path)],
                         capture_output=True, text=True, timeout=600)
    assert out.returncode == 0, out.stderr[-2000:]
    fresh = np.load(os.path.join(tmp_path, "export.npz"))
    assert sorted(fresh.files) == sorted(GOLD.files)
    for k in GOLD.files:
        if k != "meta_torch":
            assert fresh[k].dtype == GOLD[k].dtype and np.array_equal(fresh[k], GOLD[k]), k


def _row(src=0x10000, dst=0x80000, channels=3, bits=8, normal=0, sc=64, sh=8, sw=1):
    return N.ImagePack(src, sc, sh, sw, dst, channels, bits, normal, 0)


def test_pack_images_caller_errors_come_back_without_a_device():
    """Every check runs before anything is launched: the pointers are never dereferenced."""
    lib = N.lib()

    def call(rows, n=None, h=8, w=8):
        table = (N.ImagePack * max(1, len(rows)))(*rows)
        return lib.pbr_pack_images(table, len(rows) if n is None else n, h, w, None)
    assert lib.pbr_pack_images(None, 1, 8, 8, None) == N.ERR_NULL_MAP
    assert call([_row(src=None)]) == N.ERR_NULL_MAP and call([_row(dst=None)]) == N.ERR_NULL_MAP
    assert call([_row(), _row(dst=None)]) == N.ERR_NULL_MAP
    assert call([_row()], n=0) == N.ERR_SHAPE and call([_row()], n=9) == N.ERR_SHAPE and call([_row()], n=-1) == N.ERR_SHAPE
    assert call([_row()], h=0) == N.ERR_SHAPE and call([_row()], w=0) == N.ERR_SHAPE and call([_row()], h=-3) == N.ERR_SHAPE
    assert call([_row()], h=(1 << 20) + 1, w=1 << 20) == N.ERR_SHAPE                 # H * W > 2^40
    assert call([_row(sc=-1)]) == N.ERR_SHAPE and call([_row(sh=-1)]) == N.ERR_SHAPE and call([_row(sw=-1)]) == N.ERR_SHAPE
    assert call([_row(bits=16, dst=0x80001)]) == N.ERR_SHAPE                         # uint16 samples at an odd address
    assert call([_row(), _row(dst=0x80000 + 8 * 8 * 3 - 1, channels=1)]) == N.ERR_SHAPE      # the second map starts on the first's last byte
    assert call([_row(bits=16, channels=1), _row(dst=0x80000 + 8 * 8 * 2 - 2, channels=1)]) == N.ERR_SHAPE
    assert call([_row(dst=0x90000), _row(), _row(dst=0x90010, channels=1)]) == N.ERR_SHAPE   # the third inside the first
    assert call([_row(bits=0)]) == N.ERR_DTYPE and call([_row(bits=32)]) == N.ERR_DTYPE and call([_row(bits=12)]) == N.ERR_DTYPE
    assert call([_row(channels=0)]) == N.ERR_CHANNELS and call([_row(channels=5)]) == N.ERR_CHANNELS
    assert call([_row(channels=1, normal=1)]) == N.ERR_CHANNELS and call([_row(channels=4, normal=1)]) == N.ERR_CHANNELS
    assert call([_row(), _row(dst=0x90000, channels=2, normal=1)]) == N.ERR_CHANNELS


def test_python_argument_errors_need_no_device():
    with pytest.raises(TypeError):
        F.pack_image(torch.rand(3, 4, 4), bits=12)
    with pytest.raises(TypeError):
        F.pack_image(torch.rand(3, 4, 4).double())
    with pytest.raises(ValueError):
        F.pack_image(torch.rand(4, 4))
    with pytest.raises(ValueError):
        F.pack_image(torch.rand(1, 4, 4), encode_normal=True)
    with pytest.raises(ValueError):
        F.pack_image(torch.rand(5, 4, 4))
    assert F.download_samples({"albedo": None}, 8) == {}
    m = M.BasecolorMetallicMaterial(albedo=torch.rand(3, 4, 5), roughness=torch.rand(1, 4, 5))
    with pytest.raises(ValueError, match="16-bit mode"):
        m.to_pil({"albedo": "I;16"})
    assert M.MaterialBase().to_pil() == {} and M.MaterialBase().to_numpy() == {}


@pytest.fixture()
def samples():
    rng = np.random.default_rng(7)
    return {"albedo": rng.integers(0, 256, (H, W, 3), dtype=np.uint8), "roughness": rng.integers(0, 256, (H, W), dtype=np.uint8),
            "metallic": rng.integers(0, 256, (H, W), dtype=np.uint8), "height8": rng.integers(0, 256, (H, W), dtype=np.uint8),
            "height16": rng.integers(0, 65536, (H, W), dtype=np.uint16)}


def _material(samples, height):
    """A CPU-home material from in-memory PIL images (no normal map), the maps kept as the images' samples."""
    h = Image.fromarray(samples[height])
    assert h.mode == ("I;16" if height == "height16" else "L")
    m = M.BasecolorMetallicMaterial(albedo=Image.fromarray(samples["albedo"]), roughness=Image.fromarray(samples["roughness"]),
                                    metallic=Image.fromarray(samples["metallic"]), height=h)
    assert list(m._raw) == ["albedo", "roughness", "height", "metallic"] and m.device.type == "cpu"
    return m


def test_cpu_home_material_hands_its_samples_back_without_a_device(samples, monkeypatch):
    monkeypatch.setattr(M, "DEFER_IMAGE_DECODE", True)
    m = _material(samples, "height8")
    assert all(F.is_encoded(t) for t in m._raw.values())             # the path under test: the maps are still samples
    before = dict(m._raw)
    pil = m.to_pil()
    assert list(pil) == list(before)
    assert [im.mode for im in pil.values()] == ["RGB", "L", "L", "L"] and all(im.size == (W, H) for im in pil.values())
    for name, key in (("albedo", "albedo"), ("roughness", "roughness"), ("height", "height8"), ("metallic", "metallic")):
        assert np.array_equal(np.array(pil[name]), samples[key]), name
    assert all(m._raw[k] is v for k, v in before.items())            # nothing converted, nothing moved
    assert [im.mode for im in m.to_pil({"albedo": "CMYK", "height": "L"}).values()] == ["RGB", "L", "L", "L"]     # other modes are ignored

    deep = _material(samples, "height16")
    assert all(F.is_encoded(t) for t in deep._raw.values()) and deep._raw["height"].dtype == torch.uint16
    pil = deep.to_pil({"height": "I;16"})
    assert [im.mode for im in pil.values()] == ["RGB", "L", "I;16", "L"]
    got = np.array(pil["height"])
    assert got.dtype == np.uint16 and np.array_equal(got, samples["height16"])
    assert np.array_equal(np.array(pil["albedo"]), samples["albedo"]) and np.array_equal(np.array(pil["metallic"]), samples["metallic"])
    if not torch.cuda.is_available():                                # another width than the samples' own is device work
        with pytest.raises(RuntimeError):
            deep.to_pil()
        with pytest.raises(RuntimeError):
            m.to_pil({"height": "I;16"})
    # to_numpy is upstream's dict of float maps
    arrays = m.to_numpy()
    assert list(arrays) == list(before) and all(a.dtype == np.float32 for a in arrays.values())
    assert np.array_equal(arrays["albedo"], (torch.from_numpy(samples["albedo"]).permute(2, 0, 1).float() / 255).numpy())
    assert arrays["height"].shape == (1, H, W)


def test_save_material_to_folder_names_its_files_as_upstream(samples, monkeypatch, tmp_path):
    monkeypatch.setattr(M, "DEFER_IMAGE_DECODE", True)
    want = {tag: [f for f in GOLD["files__" + tag] if not f.startswith("normal.")] for tag in ("default", "override", "jpg")}   # no normal map here
    assert want["default"] == ["albedo.png", "height.png", "metallic.png", "roughness.png"]
    m = _material(samples, "height8")
    assert all(F.is_encoded(t) for t in m._raw.values())
    pio.save_material_to_folder(m, str(tmp_path / "a" / "b"))        # creates the folder
    assert sorted(os.listdir(tmp_path / "a" / "b")) == want["default"]
    m.save_to_folder(str(tmp_path / "c"))
    assert sorted(os.listdir(tmp_path / "c")) == want["default"]
    pio.save_material_to_folder(m, str(tmp_path / "d"), map_names=G.OVERRIDE)
    assert sorted(os.listdir(tmp_path / "d")) == want["override"]
    pio.save_material_to_folder(m, str(tmp_path / "e"), format="jpg")
    assert sorted(os.listdir(tmp_path / "e")) == want["jpg"]
    for name, key in (("albedo", "albedo"), ("roughness", "roughness"), ("height", "height8"), ("metallic", "metallic")):
        with Image.open(tmp_path / "c" / (name + ".png")) as im:
            assert np.array_equal(np.array(im), samples[key]), name
    m._raw["_extra"] = m._raw["roughness"]                           # io.py:225: leading underscores are dropped
    pio.save_material_to_folder(m, str(tmp_path / "f"))
    assert "extra.png" in os.listdir(tmp_path / "f")
    back = pio.load_material_from_folder(str(tmp_path / "c"))
    assert torch.equal(back._raw["albedo"], m._raw["albedo"]) and torch.equal(back._raw["height"], m._raw["height"])


def test_compat_resolves_the_export_names():
    from pypbr_amd import compat
    compat.install(force=True)
    try:
        from pypbr.io import save_material_to_folder
        from pypbr.materials import MaterialBase
        assert save_material_to_folder is pio.save_material_to_folder and MaterialBase is M.MaterialBase
        for name in ("to_pil", "to_numpy", "save_to_folder"):
            assert callable(getattr(MaterialBase, name)), name
    finally:
        compat.uninstall()
